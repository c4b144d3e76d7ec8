#!/usr/bin/env python3
"""bench.py -- Mpixels/s of the MI355X-native patolette path (BASELINE.json metric).

A "step" = one full quantisation (convert -> GQ -> LQ -> KMeans -> palette map) of one synthetic
image whose f64 planar pixels are ALREADY RESIDENT IN HBM when the timed region starts
(patolette_amd_device; the PCIe-inclusive host-to-host rate is in DESIGN.md / profiles/, never
`value`).  Default workload = the configuration the metric is quoted on ("256-color ICtCp +
KMeans"): BASELINE.json configs[2], 4096x4096, K=256, ICtCp, KMeans 32 it / 512^2 samples, dither off.

  python bench.py --gpus N --steps K --warmup W [--config c2|c3|c3full|c3sal|c4|c4map|c4km] [--dump-outputs DIR]
                  [--full [--no-cpu-baseline] [--no-extras] [--no-profile] [--extra-streams S]]

A plain run sets up, warms up, times the K steps and prints the line: nothing else.  --full adds, all outside the timed
region except the sampled kernel events: per-kernel HIP events (roofline, kernels), first_call, throughput_concurrent, the
extras of the c3 run (north_star_kernels, host_to_host, content, ...) and the CPU baseline with its parity record.

N > 1: one process per GPU (torch.distributed, backend nccl = RCCL); images are independent, so the
ranks shard the batch with NO data-path collective ("scaling": "weak": every rank quantises its own
image per step); barrier + max-over-ranks timing; the only collective is the final gather of the
index maps (u8) and palettes to rank 0, inside the timed region; rank 0 prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import queue
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (width, height, K, color_space, kmeans_niter, kmeans_max_samples, dither, weighted, description)
    "c2": (1920, 1080, 256, 2, 0, 512 ** 2, False, False, "BASELINE configs[1]: 1920x1080, 256 colors, ICtCp, KMeans off, dither off"),
    "c3": (4096, 4096, 256, 2, 32, 512 ** 2, False, False, "BASELINE configs[2]: 4096x4096, 256 colors, ICtCp + KMeans (32 it, 512^2 samples), dither off"),
    "c3full": (4096, 4096, 256, 2, 32, 4096 * 4096, False, False, "configs[2] stress: as c3 but kmeans_max_samples = N (all pixels clustered)"),
    "c4": (8192, 8192, 256, 1, 0, 512 ** 2, True, True, "BASELINE configs[3]: 8192x8192, 256 colors, CIELuv + weights + Riemersma dither"),
    "c4map": (8192, 8192, 256, 1, 0, 512 ** 2, False, True, "configs[3] without dither: 8192x8192, 256 colors, CIELuv + weights, NN map"),
    "c4km": (8192, 8192, 256, 2, 8, 8192 * 8192, False, False, "67 MP, 256 colors, ICtCp, KMeans over all 67 M pixels (8 it), NN map: the north-star kernels at full size"),
    # the Python binding's default weighting: 8-bit image in HBM, saliency weights (tile_size 512) derived on the device
    "c3sal": (4096, 4096, 256, 2, 32, 512 ** 2, False, "saliency", "configs[2] + saliency weights (tile_size 512) from an 8-bit image resident in HBM"),
}
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
EVENT_SAMPLE = 4                      # the roofline kernel carries HIP events on every 4th launch inside the timed region (4 and the
                                      # 9 launches per image are coprime: every split level is sampled over the steps)
DUMP_BYTES = 64 * 10 ** 6             # --dump-outputs writes at most this much in all


def dump_outputs(path, pals, maps, n):
    """--dump-outputs: what the timed path returned in its last step, one row per image of that step (every rank's, every
    stream's).  palette.npy = the f64 palettes as returned; index_map.npy = the u8 index maps as float32, whole where they fit in
    DUMP_BYTES, else the same fixed sample of pixels (seed 0, sorted) of every map, whose pixel numbers are index_map_pixels.npy."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    pals = np.stack(pals).astype(np.float64)
    np.save(os.path.join(path, "palette.npy"), pals)
    room = DUMP_BYTES - pals.nbytes
    if len(maps) * n * 4 <= room:
        np.save(os.path.join(path, "index_map.npy"), np.stack(maps).astype(np.float32))
        return
    s = min(n, 1 << 21, room // (4 * len(maps) + 8))
    px = np.sort(np.random.default_rng(0).choice(n, size=s, replace=False))
    np.save(os.path.join(path, "index_map.npy"), np.stack([m[px] for m in maps]).astype(np.float32))
    np.save(os.path.join(path, "index_map_pixels.npy"), px.astype(np.float64))


class Runner:
    """S concurrent images per step: one persistent host thread (own engine = HIP stream + workspace) each;
    ctypes drops the GIL during the call, so one image's host-side split-loop work overlaps another's kernels."""

    def __init__(self, L, native, cfg, S, local_rank, d_imgs, d_wts, map_ptr, pals):
        self.L, self.native, self.cfg, self.S = L, native, cfg, S
        self.d_imgs, self.d_wts, self.map_ptr, self.pals = d_imgs, d_wts, map_ptr, pals
        width, height, K, cs, niter, max_samples, dither, weighted, _ = cfg
        self.opts = native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
        self.qs = [queue.Queue() for _ in range(S)]
        self.done = queue.Queue()
        self.threads = []
        if S > 1:
            for j in range(S):
                t = threading.Thread(target=self._worker, args=(j, local_rank), daemon=True)
                t.start()
                self.threads.append(t)

    def one(self, i, j):
        import numpy as np
        width, height, K, cs, niter, max_samples, dither, weighted, _ = self.cfg
        pal = np.zeros((K, 3), dtype=np.float64, order="F")
        code = C.c_int(0)
        src = (i * self.S + j) % len(self.d_imgs)
        if weighted == "saliency":
            self.L.patolette_amd_u8_device(width, height, self.d_imgs[src], 3, None, 512.0, K, C.byref(self.opts),
                                           pal.ctypes.data_as(self.native.dp), None, self.map_ptr(i, j), 1, None, C.byref(code))
        else:
                self.L.patolette_amd_device(width, height, self.d_imgs[src], self.d_wts[src] if weighted else None, K,
                                        C.byref(self.opts), pal.ctypes.data_as(self.native.dp), self.map_ptr(i, j), 1, C.byref(code))
        if code.value != 0:
            raise RuntimeError("bench.py: quantisation failed: %s" % self.native.last_error())
        if self.pals is not None:
            self.pals[i * self.S + j] = pal

    def _worker(self, j, local_rank):
        self.L.patolette_amd_set_device(local_rank)
        while True:
            i = self.qs[j].get()
            if i is None:
                return
            try:
                self.one(i, j)
                self.done.put(None)
            except BaseException as e:      # noqa
                self.done.put(e)

    def step(self, i):
        if self.S == 1:
            self.one(i, 0)
            return
        for j in range(self.S):
            self.qs[j].put(i)
        for j in range(self.S):
            e = self.done.get()
            if e is not None:
                raise e

    def close(self):
        for q in self.qs[:len(self.threads)]:
            q.put(None)


def north_star_kernels(L, native):
    """The two kernels BASELINE.json's north_star sets a target for (>= 60 % of the HBM roofline on KMeans-assign and
    palette-map, 67 MP, 256 colours), measured here in the driver's own run: two untimed steps of the `c4km` configuration
    (8192x8192, ICtCp, KMeans over all 67 M pixels, NN map) with every kernel under HIP events.  avg_us = mean launch
    duration; frac = algorithmic bytes (16 B/sample assign, 25 B/px map: DESIGN.md section 4) / avg / 8 TB/s; traffic = HBM
    bytes per launch from the PMC passes kept in profiles/traffic_c4km.json (None if that file is absent)."""
    import numpy as np
    width, height, K, cs, niter, max_samples, dither, weighted, _ = CONFIGS["c4km"]
    n = width * height
    img = L.patolette_amd_malloc(3 * n * 8)
    dmap = L.patolette_amd_malloc(n)
    if not img or not dmap:
        return None
    try:
        assert L.patolette_amd_fill_image(img, n, 77) == 0
        opts = native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
        pal = np.zeros((K, 3), dtype=np.float64, order="F")
        code = C.c_int(0)

        def one():
            L.patolette_amd_device(width, height, img, None, K, C.byref(opts), pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
            if code.value != 0:
                raise RuntimeError("bench.py: c4km step failed: %s" % native.last_error())
        one()                                           # warm-up: workspace allocation, subsample-free path, clocks
        native.profile(True)
        steps = 2
        for _ in range(steps):
            one()
        L.patolette_amd_synchronize()
        prof = native.profile_results()
        native.profile(False)
        # the palette-map kernel once more on BASELINE configs[3]'s own geometry (`c4map`: CIELuv + weights, no KMeans): its palette
        # leaves more cells of the kernel's 32^3 table with five or more candidates than a KMeans-refined ICtCp palette does
        prof_c4map = None
        wt = L.patolette_amd_malloc(n * 8)
        if wt:
            try:
                assert L.patolette_amd_fill_weights(wt, n, 77) == 0
                _, _, K2, cs2, niter2, ms2, dither2, _, _ = CONFIGS["c4map"]
                opts2 = native.QuantizationOptions(dither2, False, cs2, niter2, ms2, False)

                def two():
                    L.patolette_amd_device(width, height, img, wt, K2, C.byref(opts2), pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
                    if code.value != 0:
                        raise RuntimeError("bench.py: c4map step failed: %s" % native.last_error())
                two()
                native.profile(True)
                for _ in range(steps):
                    two()
                L.patolette_amd_synchronize()
                prof_c4map = native.profile_results()
                native.profile(False)
            finally:
                L.patolette_amd_free(wt)
    finally:
        L.patolette_amd_free(img)
        L.patolette_amd_free(dmap)
        L.patolette_amd_release_workspace()             # ~11 GB of workspace for the 67 MP image: give it back
    traffic = {}
    tpath = os.path.join(ROOT, "profiles", "traffic_c4km.json")
    if os.path.exists(tpath):
        traffic = json.load(open(tpath)).get("kernels", {})
    # with exact candidate pruning these two kernels are HBM-bound, but not by much -- the VALU share is reported
    # beside the HBM fraction: vector instructions per launch (SQ_INSTS_VALU of the kept rocprofv3 --pmc pass, profiles/) x 4 cycles
    # per wave64 instruction on a 16-lane SIMD / (1024 SIMDs x the launch time measured here x the 2.4 GHz peak engine clock)
    valu = {}
    for tag in ("r05", "r04", "r03"):
        sq = os.path.join(ROOT, "profiles", "%s_c4km_sq_counters.txt" % tag)
        if not os.path.exists(sq):
            continue
        if os.path.exists(sq):
            for ln in open(sq):
                f = ln.split()
                if len(f) >= 9 and f[0] in ("k_km_assign_mid", "k_nn_map_mid"):
                    valu["k_km_assign" if f[0] == "k_km_assign_mid" else "k_nn_map"] = (float(f[8]), os.path.basename(sq))
            break
    out = {"config": CONFIGS["c4km"][8], "steps": steps, "peak_GBps": HBM_PEAK_GBS}
    for name in ("k_km_assign", "k_nn_map"):
        r = prof.get(name)
        if not r or not r["launches"]:
            continue
        avg_ms = r["total_ms"] / r["launches"]
        gbs = r["bytes"] / r["launches"] / (avg_ms * 1e-3) / 1e9
        out[name] = {"avg_us": round(avg_ms * 1e3, 2), "launches": r["launches"], "achieved_GBps": round(gbs, 1),
                     "frac": round(gbs / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": round(r["bytes"] / r["launches"], 1),
                     "traffic": traffic.get(name, {}).get("hbm_bytes_per_launch")}
        if name in valu:
            out[name]["valu_frac"] = round(valu[name][0] * 4.0 / (1024.0 * avg_ms * 1e-3 * 2.4e9), 3)
            out[name]["valu_insts_per_launch"] = valu[name][0]
            out[name]["valu_source"] = "profiles/%s (SQ_INSTS_VALU, a separate rocprofv3 --pmc pass, not this run)" % valu[name][1]
    r = (prof_c4map or {}).get("k_nn_map")
    if r and r["launches"]:
        avg_ms = r["total_ms"] / r["launches"]
        gbs = r["bytes"] / r["launches"] / (avg_ms * 1e-3) / 1e9
        out["k_nn_map_c4map"] = {"config": CONFIGS["c4map"][8], "avg_us": round(avg_ms * 1e3, 2), "launches": r["launches"],
                                 "achieved_GBps": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4),
                                 "algorithmic_bytes_per_launch": round(r["bytes"] / r["launches"], 1)}
    return out


CONTENT_PARITY_SIZE = (1536, 1024)          # the size at which the content workloads are held to the oracle (seconds of CPU each)


def content_images(width, height):
    """The three non-noise workloads of the `content` record, as planar f64 host arrays (name, pixels), one at a time: a smooth
    synthetic scene with saturated blobs and mild noise, the same scene posterised to eight levels per channel (a handful of
    distinct colours: 64 lanes adding to one histogram bucket), and noise with one colour covering 30 % of the image (one very
    long centroid chain).  tests/test_gpu_content.py holds the same generator's images to the oracle."""
    import numpy as np
    n = width * height
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    planes = [0.5 + 0.4 * np.sin(xx / (0.15 * width + 3.0) + 4.0), 0.5 + 0.4 * np.cos(yy / (0.12 * height + 3.0)),
              0.35 + 0.25 * np.sin((xx + yy) / (0.2 * (width + height) + 3.0))]
    for _ in range(3):
        cy, cx = rng.uniform(0.25, 0.75) * height, rng.uniform(0.25, 0.75) * width
        ry, rx = rng.uniform(0.05, 0.18) * height + 1, rng.uniform(0.05, 0.18) * width + 1
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        for pl, v in zip(planes, rng.uniform(0.0, 1.0, size=3)):
            pl[inside] = v
    del yy, xx
    scene = np.empty(3 * n)
    for j, pl in enumerate(planes):
        scene[j * n:(j + 1) * n] = np.clip(pl.reshape(-1).astype(np.float64) + rng.normal(0.0, 0.02, n), 0.0, 1.0)
    del planes
    yield "scene", scene
    yield "posterised", np.round(scene * 7.0) / 7.0
    del scene
    noise = rng.random(3 * n)
    m = int(0.3 * n)
    for j, v in enumerate((0.1, 0.2, 0.7)):
        noise[j * n:j * n + m] = v + 0.004 * rng.standard_normal(m)
    yield "dominant30", np.clip(noise, 0.0, 1.0)


def content_parity(L, native, ob, cfg, host, width, height):
    """One content image through the HIP path (device-resident entry, the configuration's options) and through the oracle.
    What is asserted in tests/test_gpu_content.py is reported here: palette rows (max relative difference, or the rows as a set
    when their order differs), index-map mismatches, and -- the weakest form -- whether the two quantised IMAGES agree."""
    import numpy as np
    _, _, K, cs, niter, max_samples, dither, weighted, _ = cfg
    n = width * height
    d = L.patolette_amd_malloc(3 * n * 8)
    dmap = L.patolette_amd_malloc(n)
    if not d or not dmap:
        return None
    try:
        assert L.patolette_amd_memcpy_h2d(d, host.ctypes.data_as(C.c_void_p), host.nbytes) == 0
        opts = native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
        pal = np.zeros((K, 3), dtype=np.float64, order="F")
        code = C.c_int(0)
        L.patolette_amd_device(width, height, d, None, K, C.byref(opts), pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
        L.patolette_amd_synchronize()
        if code.value != 0:
            return {"note": "HIP path exit code %d" % code.value}
        m8 = np.empty(n, dtype=np.uint8)
        assert L.patolette_amd_memcpy_d2h(m8.ctypes.data_as(C.c_void_p), dmap, n) == 0
    finally:
        L.patolette_amd_free(d)
        L.patolette_amd_free(dmap)
    ob.set_threads(os.cpu_count() or 1)
    try:
        ec, pal_o, map_o = ob.patolette(width, height, host, None, K, dither=dither, color_space=cs, kmeans_niter=niter, kmeans_max_samples=max_samples)
    finally:
        ob.set_threads(1)
    if ec != 0:
        return {"note": "oracle exit code %d" % ec}
    rec = compare_results(pal, m8.astype(np.int64), np.asarray(pal_o), np.asarray(map_o).astype(np.int64), "%dx%d" % (width, height))
    if not rec["verdict"].startswith("identical"):
        # not the oracle's result: is the difference PROVEN tie noise?  (tests/tie_prover.py: every decision of the HIP path's split
        # trace inside the rounding envelope of the exact optimum, the stages behind the quantisers replayed by the oracle)
        try:
            from tests import tie_prover
            ob.set_threads(os.cpu_count() or 1)
            why = tie_prover.explain_divergence(ob, native, L, width, height, host, None, K, cs, dither, niter, max_samples, pal, m8.astype(np.uintp))
            rec["tie_proof"] = {"proven": True, "first_differing_decision": list(why["first"][:2]) if why["first"] else None,
                                "decisions_checked": why["decisions"], "ties_in_hip_trace": why["ties_gpu"], "ties_in_oracle_trace": why["ties_oracle"]}
        except AssertionError as e:
            rec["tie_proof"] = {"proven": False, "why": str(e)[:300]}
        finally:
            ob.set_threads(1)
    return rec


def compare_results(pal, pmap, pal_o, map_o, size):
    """HIP result against the oracle's, strongest statement first."""
    import numpy as np
    used, used_o = pal[:, 0] != -1.0, pal_o[:, 0] != -1.0
    rec = {"size": size, "palette_rows": int(used.sum()), "palette_rows_oracle": int(used_o.sum())}
    same_rows = bool(np.array_equal(used, used_o))
    scale = max(1e-300, float(np.max(np.abs(pal_o[used_o])))) if used_o.any() else 1.0
    rec["palette_max_rel"] = float(np.max(np.abs(pal[used] - pal_o[used_o])) / scale) if same_rows and used.any() else None
    rec["map_mismatches"] = int(np.count_nonzero(pmap != map_o))
    if rec["palette_max_rel"] is not None and rec["palette_max_rel"] <= 1e-9 and rec["map_mismatches"] == 0:
        rec["verdict"] = "identical: palette rows in the reference's order within 1e-9 relative, index map bit for bit"
        return rec
    rows_g = sorted(map(tuple, np.round(pal[used], 9).tolist()))
    rows_o = sorted(map(tuple, np.round(pal_o[used_o], 9).tolist()))
    rec["palette_equal_as_a_set"] = rows_g == rows_o
    rec["palette_rows_differing"] = int(len(set(rows_g) ^ set(rows_o)) // 2) if len(rows_g) == len(rows_o) else None
    img_diff = float(np.max(np.abs(pal[pmap] - pal_o[map_o])))
    rec["quantised_image_max_abs_diff"] = img_diff
    rec["quantised_image_mean_sq_diff"] = float(np.mean((pal[pmap] - pal_o[map_o]) ** 2))
    if rows_g == rows_o and img_diff <= 1e-9:
        rec["verdict"] = "same palette as a set and same quantised image; the ORDER of the rows differs"
    elif img_diff <= 1e-9:
        rec["verdict"] = "same quantised image; palette rows differ where clusters are empty or tied"
    else:
        rec["verdict"] = "differs: see DESIGN.md 2 (cut decisions of the reference that hinge on the rounding of sequential f64 sums)"
    return rec


def content_times(L, native, cfg, ob=None):
    """The timed region runs on uniform noise (what BASELINE.json asks for) -- the best case of the LDS histograms and of the
    centroid chains.  Here the SAME configuration once each on content a photograph is closer to (content_images), device-resident
    like `value`, outside the timed region and never part of `value`.  With the oracle at hand each workload also carries a
    `parity` record taken at CONTENT_PARITY_SIZE, where the oracle needs seconds."""
    import numpy as np
    width, height, K, cs, niter, max_samples, dither, weighted, _ = cfg
    n = width * height
    d = L.patolette_amd_malloc(3 * n * 8)
    dmap = L.patolette_amd_malloc(n)
    if not d or not dmap:
        return None
    opts = native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
    pal = np.zeros((K, 3), dtype=np.float64, order="F")
    code = C.c_int(0)
    out = {"note": "same configuration and entry point as `value`, other image content; median of 3 after one warm-up; never part of `value`"}

    def run(host, name):
        assert L.patolette_amd_memcpy_h2d(d, host.ctypes.data_as(C.c_void_p), host.nbytes) == 0
        times = []
        for i in range(4):
            L.patolette_amd_synchronize()
            t0 = time.perf_counter()
            L.patolette_amd_device(width, height, d, None, K, C.byref(opts), pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
            L.patolette_amd_synchronize()
            if code.value != 0:
                return
            if i:
                times.append(time.perf_counter() - t0)
        st = native.last_stats()
        out[name] = {"ms": round(1e3 * sorted(times)[1], 3), "ms_lq": round(st["ms_lq"], 3), "ms_kmeans": round(st["ms_kmeans"], 3),
                     "split_evals": st["split_evals"]}
        if niter > 0:
            # the same image with the order-free centroid update (an option: include/patolette_amd.h), whose cost does not depend
            # on how the samples spread over the centroids
            before = L.patolette_amd_set_kmeans_update(1)
            try:
                t1 = []
                for i in range(3):
                    L.patolette_amd_synchronize()
                    t0 = time.perf_counter()
                    L.patolette_amd_device(width, height, d, None, K, C.byref(opts), pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
                    L.patolette_amd_synchronize()
                    if i:
                        t1.append(time.perf_counter() - t0)
                if code.value == 0:
                    out[name]["order_free_kmeans_update"] = {"ms": round(1e3 * min(t1), 3), "ms_kmeans": round(native.last_stats()["ms_kmeans"], 3)}
            finally:
                L.patolette_amd_set_kmeans_update(before)
    try:
        for name, host in content_images(width, height):
            run(host, name)
            del host
    finally:
        L.patolette_amd_free(d)
        L.patolette_amd_free(dmap)
    if ob is not None:
        pw, ph = CONTENT_PARITY_SIZE
        for name, host in content_images(pw, ph):
            if name in out:
                out[name]["parity"] = content_parity(L, native, ob, cfg, host, pw, ph)
    return out


def host_to_host(L, native, cfg, reps=3):
    """SURVEY.md 8(d) metric (ii): the same workload through the reference's own entry point `patolette()` -- host f64
    image in (pageable numpy memory), size_t map and f64 palette out, PCIe copies included.  Reported next to, never as,
    `value`."""
    import numpy as np
    width, height, K, cs, niter, max_samples, dither, weighted, _ = cfg
    n = width * height
    d = L.patolette_amd_malloc(3 * n * 8)
    if not d:
        return None
    host = np.empty(3 * n)
    try:
        assert L.patolette_amd_fill_image(d, n, 55) == 0
        assert L.patolette_amd_memcpy_d2h(host.ctypes.data_as(C.c_void_p), d, host.nbytes) == 0
    finally:
        L.patolette_amd_free(d)
    wts = None
    if weighted is True:                            # the library's own generator (SURVEY.md 8(d) weights), brought to the host
        dw = L.patolette_amd_malloc(n * 8)
        if not dw:
            return None
        wts = np.empty(n)
        try:
            assert L.patolette_amd_fill_weights(dw, n, 55) == 0
            assert L.patolette_amd_memcpy_d2h(wts.ctypes.data_as(C.c_void_p), dw, wts.nbytes) == 0
        finally:
            L.patolette_amd_free(dw)
    opts = native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
    pal = np.zeros((K, 3), dtype=np.float64, order="F")
    pmap = np.zeros(n, dtype=np.uintp)
    code = C.c_int(0)
    times = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        L.patolette(width, height, host.ctypes.data_as(native.dp), wts.ctypes.data_as(native.dp) if wts is not None else None, K,
                    C.byref(opts), pal.ctypes.data_as(native.dp), pmap.ctypes.data_as(native.zp), C.byref(code))
        dt = time.perf_counter() - t0
        if code.value != 0:
            return None
        if i > 0:
            times.append(dt)
    st = native.last_stats()
    best = sorted(times)[len(times) // 2]
    return {"value": round(n / best / 1e6, 2), "unit": "Mpx/s", "ms_per_image": round(best * 1e3, 3), "reps": reps,
            "entry": "patolette() (include/patolette.h), pageable host buffers, f64 planar in, size_t map out",
            "ms_upload": round(st["ms_upload"], 3), "ms_download": round(st["ms_download"], 3)}


def small_image(L, native, reps=7):
    """BASELINE configs[1] (1920x1080, 256 colours, ICtCp, KMeans off, dither off) device-resident like `value`: the size people
    actually quantise, where the split loop's nine host round trips and ~70 launches weigh as much as its sweeps."""
    import numpy as np
    width, height, K, cs, niter, max_samples, dither, weighted, desc = CONFIGS["c2"]
    n = width * height
    d = L.patolette_amd_malloc(3 * n * 8)
    dmap = L.patolette_amd_malloc(n)
    if not d or not dmap:
        return None
    try:
        assert L.patolette_amd_fill_image(d, n, 0) == 0
        opts = native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
        pal = np.zeros((K, 3), dtype=np.float64, order="F")
        code = C.c_int(0)

        def timed():
            times = []
            for i in range(reps + 2):
                L.patolette_amd_synchronize()
                t0 = time.perf_counter()
                L.patolette_amd_device(width, height, d, None, K, C.byref(opts), pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
                L.patolette_amd_synchronize()
                if code.value != 0:
                    return None, None
                if i >= 2:
                    times.append(time.perf_counter() - t0)
            return sorted(times)[len(times) // 2], native.last_stats()
        med, st = timed()
        if med is None:
            return None
        # the same call with the split loop driven by the host (a synchronisation, the host's turn and an upload per round): the A/B
        prev = L.patolette_amd_set_split_loop(0)
        try:
            med_h, st_h = timed()
        finally:
            L.patolette_amd_set_split_loop(prev)
    finally:
        L.patolette_amd_free(d)
        L.patolette_amd_free(dmap)
    return {"config": desc, "ms": round(1e3 * med, 3), "value": round(n / med / 1e6, 1), "unit": "Mpx/s", "reps": reps,
            "stages_ms": {k: round(v, 3) for k, v in st.items() if k.startswith("ms_") and v}, "lq_rounds": st["lq_rounds"],
            "split_evals": st["split_evals"], "split_loop": "device-driven (the default up to 40 Mpixel), global quantiser's decisions on the device: one host synchronisation per image before the map",
            "host_driven_split_loop": None if med_h is None else {"ms": round(1e3 * med_h, 3), "ms_lq": round(st_h["ms_lq"], 3),
                                                                    "lq_rounds": st_h["lq_rounds"], "split_evals": st_h["split_evals"]}}


def host_to_host_u8(L, native, cfg, reps=3):
    """The path a caller of the reference actually takes (README.md:147-158, 184-194: an 8-bit image in, an indexed image out)
    through the 8-bit adaptor `patolette_amd_u8`: pageable (H, W, 3) u8 pixels in, u8 index map + u8 palette
    out, PCIe copies included -- 3 B/px up and 1 B/px down instead of 24 + 8.  Without saliency weights (tile_size = 0, what
    `value` computes) and with them derived on the device (tile_size = 512, the reference's Python default).  Never `value`."""
    import numpy as np
    width, height, K, cs, niter, max_samples, dither, weighted, _ = cfg
    n = width * height
    img = np.random.default_rng(55).integers(0, 256, size=(height, width, 3), dtype=np.uint8)
    opts = native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
    pal = np.zeros((K, 3), dtype=np.float64, order="F")
    pal8 = np.zeros((K, 3), dtype=np.uint8)
    pmap = np.zeros(n, dtype=np.uint8 if K <= 256 else np.uint32)
    code = C.c_int(0)
    out = {"entry": "patolette_amd_u8() (include/patolette_amd.h), pageable host buffers, (H,W,3) u8 in, %s index map + u8 palette out" % pmap.dtype,
           "reps": reps}
    for tile in (0.0, 512.0):
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            L.patolette_amd_u8(width, height, img.ctypes.data_as(C.c_void_p), 3, None, C.c_double(tile), K, C.byref(opts),
                               pal.ctypes.data_as(native.dp), pal8.ctypes.data_as(C.c_void_p), pmap.ctypes.data_as(C.c_void_p),
                               pmap.dtype.itemsize, None, C.byref(code))
            dt = time.perf_counter() - t0
            if code.value != 0:
                return None
            if i > 0:
                times.append(dt)
        st = native.last_stats()
        best = sorted(times)[len(times) // 2]
        out["tile_size_%d" % int(tile)] = {"value": round(n / best / 1e6, 2), "unit": "Mpx/s", "ms_per_image": round(best * 1e3, 3),
                                           "ms_upload": round(st["ms_upload"], 3), "ms_download": round(st["ms_download"], 3),
                                           "ms_saliency": round(st["ms_saliency"], 3)}
    return out


def default_call(L, native, reps=3):
    """What a caller of the reference's Python binding gets with every default left alone (patolette.pyx:332-344: dither = True,
    ICtCp, tile_size = 512 -> saliency weights, KMeans 32 iterations on 512^2 samples, 256 colours): an 8-bit host image in, a u8
    index map out (`patolette_amd_u8`), PCIe included.  The reference runs this call single-threaded on the CPU; never `value`."""
    import numpy as np
    out = {"entry": "patolette_amd_u8(), pageable (H,W,3) u8 in, u8 map out; dither on, tile_size 512, KMeans 32 it, K = 256"}
    for (w, h) in ((1920, 1080), (4096, 4096)):
        n = w * h
        img = np.random.default_rng(77).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        opts = native.QuantizationOptions(True, False, 2, 32, 512 ** 2, False)
        pal = np.zeros((256, 3), dtype=np.float64, order="F")
        pal8 = np.zeros((256, 3), dtype=np.uint8)
        pmap = np.zeros(n, dtype=np.uint8)
        code = C.c_int(0)
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            L.patolette_amd_u8(w, h, img.ctypes.data_as(C.c_void_p), 3, None, C.c_double(512.0), 256, C.byref(opts),
                               pal.ctypes.data_as(native.dp), pal8.ctypes.data_as(C.c_void_p), pmap.ctypes.data_as(C.c_void_p), 1, None, C.byref(code))
            dt = time.perf_counter() - t0
            if code.value != 0:
                return None
            if i:
                times.append(dt)
        st = native.last_stats()
        best = sorted(times)[len(times) // 2]
        out["%dx%d" % (w, h)] = {"ms": round(1e3 * best, 3), "value": round(n / best / 1e6, 1), "unit": "Mpx/s",
                                 "stages_ms": {k: round(v, 3) for k, v in st.items() if k.startswith("ms_") and v},
                                 "dither_runs": st["dither_segments"], "dither_repairs": st["dither_repairs"]}
    return out


def dither_content(L, native, side=4096, reps=3):
    """The dither on image CONTENT other than noise (noise is the best case: the speculative runs meet the true chain soonest and the
    queries stay inside the record grid): map-stage time of a device-resident call with dither on (ICtCp, K = 256, KMeans off) on
    the tests' scene enlarged 2 x (smooth like a large photograph), analytic gradients with 2 % noise, without noise, and
    posterised to 8 levels per channel (large flat areas).  Untimed extra; bit-exactness of these content classes against the
    oracle is held by tests/test_gpu_dither_segments.py and tools/fuzz_dither_large.py at sizes the oracle does in seconds."""
    import numpy as np
    from tests.util import scene
    n = side * side
    img = L.patolette_amd_malloc(3 * n * 8)
    dmap = L.patolette_amd_malloc(n)
    if not img or not dmap:
        return None
    out = {"config": "%dx%d, K = 256, ICtCp, dither on, KMeans off; ms_map = conversions to Rec2020 + dither, device-resident" % (side, side)}
    try:
        opts = native.QuantizationOptions(True, False, 2, 0, 512 ** 2, False)
        pal = np.zeros((256, 3), dtype=np.float64, order="F")
        code = C.c_int(0)
        y, x = np.mgrid[0:side, 0:side].astype(np.float32)
        sm = np.stack([0.5 + 0.5 * np.sin(x / 337.0) * np.cos(y / 253.0), (x + y) / (2.0 * side), 0.5 + 0.5 * np.cos((x - y) / 571.0)]).astype(np.float64)
        del x, y

        def cases():
            yield "noise", None
            yield "scene_x2", np.ascontiguousarray(np.moveaxis(np.kron(scene(side // 2, side // 2, 4), np.ones((2, 2, 1))), 2, 0))
            yield "gradients_2pct_noise", np.clip(sm + 0.02 * np.random.default_rng(3).standard_normal(sm.shape), 0, 1)
            yield "gradients", sm
            yield "posterised_8_levels", np.round(sm * 7) / 7
        for name, planes in cases():
            if planes is None:
                assert L.patolette_amd_fill_image(img, n, 7) == 0
            else:
                flat = np.ascontiguousarray(planes.reshape(-1))
                assert L.patolette_amd_memcpy_h2d(img, flat.ctypes.data_as(C.c_void_p), flat.nbytes) == 0
                del flat
            ms = []
            for i in range(reps + 1):
                L.patolette_amd_device(side, side, img, None, 256, C.byref(opts), pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
                if code.value != 0:
                    return None
                st = native.last_stats()
                if i:
                    ms.append(st["ms_map"])
            out[name] = {"ms_map": round(sorted(ms)[len(ms) // 2], 3), "ns_per_px": round(1e6 * sorted(ms)[len(ms) // 2] / n, 4), "runs": st["dither_segments"],
                         "repairs": st["dither_repairs"], "passes": st["dither_rounds"], "through_walks": st["dither_through"],
                         "periodic_jumps": st["dither_jumps"], "solo_passes": st["dither_solo"]}
    finally:
        L.patolette_amd_free(img)
        L.patolette_amd_free(dmap)
    return out


def parity_record(L, native, cfg, d_img, d_wt, pal_timed, res_all, res_one, ob):
    """The metric's second half ("palette dE vs ref"): rank 0's image 0 (seed 0) of the timed region against the CPU oracle's
    result for the SAME full-size image -- the one the cpu_baseline leg has just computed.  The palette compared is the one a
    timed step returned; the index map (left in HBM during the timed region) is taken from one more, untimed, call on the same
    image and entry point, whose palette must be the timed step's bit for bit.  The oracle is the checker here, nothing else."""
    import numpy as np
    width, height, K, cs, niter, max_samples, dither, weighted, _ = cfg
    n = width * height
    ec, pal_o, map_o = res_all
    if ec != 0 or map_o is None:
        return {"note": "oracle exit code %d" % ec}
    dmap = L.patolette_amd_malloc(n)
    if not dmap:
        return None
    try:
        opts = native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
        pal = np.zeros((K, 3), dtype=np.float64, order="F")
        code = C.c_int(0)
        L.patolette_amd_device(width, height, d_img, d_wt, K, C.byref(opts), pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
        L.patolette_amd_synchronize()
        if code.value != 0:
            return {"note": "HIP path exit code %d" % code.value}
        m8 = np.empty(n, dtype=np.uint8)
        assert L.patolette_amd_memcpy_d2h(m8.ctypes.data_as(C.c_void_p), dmap, n) == 0
    finally:
        L.patolette_amd_free(dmap)
    pal_o = np.asarray(pal_o, dtype=np.float64)
    rows_o = int(np.sum(pal_o[:, 0] != -1.0))
    same_tail = bool(np.array_equal(pal == -1.0, pal_o == -1.0))
    used = pal_o[:, 0] != -1.0
    rel = float(np.max(np.abs(pal[used] - pal_o[used])) / max(1e-300, float(np.max(np.abs(pal_o[used]))))) if same_tail and rows_o else None
    # dE_ITP between the two palettes: 720 * sqrt(dI^2 + dT^2 + dP^2) with T = Ct / 2 -- the reference's ICtCp already halves Ct
    # (lib/src/color/ICtCp.c:78); the conversion used for this report is the oracle's
    de = None
    if same_tail and rows_o:
        a = ob.convert("srgb_to_ictcp", ob.planar(np.clip(pal[used], 0.0, 1.0))).reshape(3, -1)
        b = ob.convert("srgb_to_ictcp", ob.planar(np.clip(pal_o[used], 0.0, 1.0))).reshape(3, -1)
        de = float(np.max(720.0 * np.sqrt(np.sum((a - b) ** 2, axis=0))))
    mism = int(np.count_nonzero(m8 != np.asarray(map_o).astype(np.uint8))) if K <= 256 else None
    return {"image": "rank 0, image 0 (seed 0) of the timed region, %dx%d, full size" % (width, height),
            "against": "oracle/ (CPU restatement of the reference path) on this host, the cpu_baseline run",
            "pixels": n, "palette_rows": rows_o, "unused_rows_match": same_tail,
            "palette_max_rel": rel, "palette_max_deltaE_ITP": de, "map_mismatches": mism,
            "palette_of_timed_step_identical": (bool(np.array_equal(pal_timed, pal)) if pal_timed is not None else None),
            "oracle_all_core_equals_single_thread": bool(np.array_equal(res_all[1], res_one[1]) and np.array_equal(res_all[2], res_one[2])),
            "tolerance": "north_star: index map bit-exact, palette 1e-5 relative"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps measure and check everything else the line reports: per-kernel HIP events (roofline, "
                         "kernels), first_call, throughput_concurrent, the extras of the c3 run, cpu_baseline and parity")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps write what the last one returned (palettes, index maps) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline and parity")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the untimed extras of the c3 run: north_star_kernels, host_to_host, ...")
    ap.add_argument("--no-profile", action="store_true", help="with --full: do not record per-kernel HIP events in the timed region")
    ap.add_argument("--force-dist", action="store_true", help="take the torch.distributed (RCCL) path even with one rank")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="TEST MODE, never a measurement of scaling: the N ranks share the GPUs the box has (rank r on device r mod count) and the "
                         "final gather runs on the gloo backend through host staging (RCCL refuses two ranks on one device); everything else -- "
                         "sharding, per-step asynchronous gather, palette gather, barrier + max-over-ranks timing -- is the N > 1 code of the RCCL path")
    ap.add_argument("--check-gather", action="store_true",
                    help="after the timed region rank 0 quantises every rank's images itself, one call per image, and compares the gathered "
                         "maps and palettes with them (reported as gather_check)")
    ap.add_argument("--streams", type=int, default=1, help="images quantised concurrently per GPU and step in the timed region")
    ap.add_argument("--extra-streams", type=int, default=6,
                    help="with --full: after the timed region also measure throughput with this many concurrent images per GPU; reported "
                         "separately as throughput_concurrent, never as `value` (0 = skip)")
    ap.add_argument("--kmeans-update", type=int, default=0, choices=[0, 1],
                    help="1: the order-free centroid update (patolette_amd_set_kmeans_update(1)): NOT the reference's bits and OUTSIDE north_star's "
                         "1e-5 -- ~1e-6 of the colour range per iteration, ~1e-4 after the default 32 iterations at ~1000 members per centroid, "
                         "~0.02 %% of the index map follows (tests/test_gpu_kmeans_update.py); the line says so in config.kmeans_update and is "
                         "never the headline")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    profile = args.full and not args.no_profile

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: start the N ranks here (one process per GPU, RCCL), exactly as the driver's
        # `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N` does; rank 0 prints the line.
        import socket
        import subprocess
        from patolette_amd import _native
        have = _native.lib().patolette_amd_device_count()
        if have < args.gpus and not (args.oversubscribe and have >= 1):
            raise SystemExit("bench.py: --gpus %d but %d HIP device(s) visible" % (args.gpus, have))
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))

    dist = None
    torch = None
    if world > 1 or args.force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29577")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch
        import torch.distributed as dist
        if args.oversubscribe:
            local_rank = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="gloo" if args.oversubscribe else "nccl", rank=rank, world_size=world)
        if dist.get_world_size() != args.gpus:          # n_gpus in the line = the ranks RCCL actually saw
            raise SystemExit("bench.py: RCCL group of %d ranks, --gpus %d" % (dist.get_world_size(), args.gpus))
        world = dist.get_world_size()

    import numpy as np
    from patolette_amd import _native
    L = _native.lib()
    if L.patolette_amd_device_count() <= 0:
        raise SystemExit("bench.py: no HIP device visible (the HIP path has no CPU fallback)")
    if L.patolette_amd_set_device(local_rank) != 0:
        raise SystemExit("bench.py: cannot select device %d" % local_rank)

    if args.kmeans_update:
        L.patolette_amd_set_kmeans_update(1)
    cfg = CONFIGS[args.config]
    width, height, K, cs, niter, max_samples, dither, weighted, desc = cfg
    n = width * height
    S = max(1, args.streams)
    S2 = max(0, args.extra_streams) if args.full else 0
    # distinct images; more in flight than that re-use them (read-only).  The pool does not depend on --full: a plain run
    # quantises the same images
    pool = max(S, min(max(0, args.extra_streams), 3), min(3, args.steps))
    d_imgs, d_wts = [], []
    for i in range(pool):
        if weighted == "saliency":
            p = L.patolette_amd_malloc(3 * n)
            img8 = np.random.default_rng(100 * rank + i).integers(0, 256, size=3 * n, dtype=np.uint8)
            assert p and L.patolette_amd_memcpy_h2d(p, img8.ctypes.data_as(C.c_void_p), 3 * n) == 0
            d_imgs.append(p)
            continue
        p = L.patolette_amd_malloc(3 * n * 8)
        if not p:
            raise SystemExit("bench.py: hipMalloc failed")
        assert L.patolette_amd_fill_image(p, n, 100 * rank + i) == 0
        d_imgs.append(p)
        if weighted:
            q = L.patolette_amd_malloc(n * 8)
            assert L.patolette_amd_fill_weights(q, n, 100 * rank + i) == 0
            d_wts.append(q)
    pals = np.zeros(((args.steps + args.warmup) * S, K, 3), dtype=np.float64)
    if dist is not None:
        # index maps (u8, K <= 256) of every step stay in HBM in a torch tensor the library writes into
        # directly, so the final RCCL gather needs no staging copy
        maps_t = torch.empty((args.steps * S, n), dtype=torch.uint8, device="cuda")
        warm_t = torch.empty((max(S, S2, 1), n), dtype=torch.uint8, device="cuda")
        map_ptr = lambda i, j: (maps_t[(i - args.warmup) * S + j].data_ptr() if i >= args.warmup else warm_t[j].data_ptr())
        map_ptr2 = lambda i, j: warm_t[j].data_ptr()
        # what a collective is handed: the device tensor itself on RCCL; a host copy on gloo (--oversubscribe)
        wire = (lambda t: t.cpu()) if args.oversubscribe else (lambda t: t)
        wire_dev = "cpu" if args.oversubscribe else "cuda"
    else:
        d_maps = [L.patolette_amd_malloc(n) for _ in range(max(S, S2, 1))]      # K <= 256 -> u8 index map left in HBM
        map_ptr = lambda i, j: d_maps[j]
        map_ptr2 = map_ptr

    def barrier():
        L.patolette_amd_synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    run = Runner(L, _native, cfg, S, local_rank, d_imgs, d_wts, map_ptr, pals)
    # Kernel events: two hipEventRecord per launch cost ~7 us, ~250 launches per image.  The last warm-up step is
    # timed in full to find the dominant kernel; inside the timed region only that kernel carries events (the
    # roofline figure); the per-kernel table comes from one extra, untimed, fully timed step afterwards.
    dom_name = None
    for i in range(args.warmup):
        if profile and i == args.warmup - 1:
            _native.profile(True)
        run.step(i)
        if dist is not None:
            # a warm-up step is a whole step: its maps are gathered too (the first gather sets up RCCL's channels and buffers)
            part = wire(warm_t[:S])
            gl = [torch.empty_like(part) for _ in range(world)] if rank == 0 else None
            dist.gather(part, gl, dst=0)
            pw_t = torch.from_numpy(pals[i * S:(i + 1) * S]).to(wire_dev)
            gp = [torch.empty_like(pw_t) for _ in range(world)] if rank == 0 else None
            dist.gather(pw_t, gp, dst=0)
            torch.cuda.synchronize()
            del gl, gp
    if profile and args.warmup > 0:
        L.patolette_amd_synchronize()
        pw = _native.profile_results()
        if pw:
            dom_name = max(pw, key=lambda k: pw[k]["total_ms"])
        _native.profile(False)
    barrier()
    if profile:
        _native.profile(True, only=dom_name, sample=EVENT_SAMPLE)
    gathered, works = [], []
    t0 = time.perf_counter()
    for i in range(args.steps):
        run.step(args.warmup + i)
        if dist is not None:
            # The only collective of the job: the results go to rank 0 over RCCL/xGMI.  The u8 maps of step i (complete: the
            # library call has returned) are gathered asynchronously on RCCL's own stream while step i+1 computes.
            part = wire(maps_t[i * S:(i + 1) * S])
            gl = [torch.empty_like(part) for _ in range(world)] if rank == 0 else None
            gathered.append(gl)
            works.append(dist.gather(part, gl, dst=0, async_op=True))
    L.patolette_amd_synchronize()
    if dist is not None:
        pal_t = torch.from_numpy(pals[args.warmup * S:]).to(wire_dev)
        gl_p = [torch.empty_like(pal_t) for _ in range(world)] if rank == 0 else None
        works.append(dist.gather(pal_t, gl_p, dst=0, async_op=True))
        for w in works:
            w.wait()
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    stats = _native.last_stats()
    if args.dump_outputs and rank == 0:
        # taken before anything else runs: the untimed steps of --full reuse the result slots
        last = args.warmup + args.steps - 1
        if dist is None:
            maps = []
            for j in range(S):
                m8 = np.empty(n, dtype=np.uint8)
                assert L.patolette_amd_memcpy_d2h(m8.ctypes.data_as(C.c_void_p), map_ptr(last, j), n) == 0
                maps.append(m8)
            dump_outputs(args.dump_outputs, list(pals[last * S:(last + 1) * S]), maps, n)
        else:
            last_pals = [gl_p[r][(args.steps - 1) * S + j].cpu().numpy() for r in range(world) for j in range(S)]
            dump_outputs(args.dump_outputs, last_pals, [gathered[-1][r][j].cpu().numpy() for r in range(world) for j in range(S)], n)
    # the palette a TIMED step produced for rank 0's image 0 (seed 0): what `parity` below holds to the oracle
    pal_timed = None
    for i in range(args.steps):
        if ((args.warmup + i) * S) % len(d_imgs) == 0:
            pal_timed = pals[(args.warmup + i) * S].copy()
            break
    prof = _native.profile_results() if profile else {}
    _native.profile(False)
    prof_full = prof
    if profile and dom_name is not None:
        _native.profile(True)
        run.step(args.warmup + args.steps - 1)          # untimed: every kernel carries events
        L.patolette_amd_synchronize()
        prof_full = _native.profile_results()
        _native.profile(False)
    # ---- what a FIRST call of an image size costs (the subsample list made again in every call), outside the timed region ----
    cold = None
    if args.full and niter > 0 and S == 1:
        prev = L.patolette_amd_set_subsample_cache(0)
        try:
            tt = []
            for i in range(min(6, max(3, args.steps))):
                L.patolette_amd_synchronize()
                tc = time.perf_counter()
                run.step(args.warmup + i % max(1, args.steps))         # (the result slots of the timed steps are reused)
                L.patolette_amd_synchronize()
                tt.append(time.perf_counter() - tc)
        finally:
            L.patolette_amd_set_subsample_cache(prev)
        cold = {"ms_per_step": round(1e3 * sorted(tt)[len(tt) // 2], 3), "steps": len(tt),
                "note": "patolette_amd_set_subsample_cache(0): every call makes the KMeans subsample list (faiss rand_perm(N, 1234): 262 144 mt19937 "
                        "draws) again on the helper thread that starts at call entry, and uploads it; workspace already allocated"}
    run.close()
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=wire_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # ---- extra, separately reported: throughput with several images in flight per GPU (no kernel events) ----
    conc = None
    if S2 > 1:
        run2 = Runner(L, _native, cfg, S2, local_rank, d_imgs, d_wts, map_ptr2, None)
        run2.step(0)
        barrier()
        k2 = max(2, args.steps // 2)
        t1 = time.perf_counter()
        for i in range(k2):
            run2.step(i)
        L.patolette_amd_synchronize()
        e2 = time.perf_counter() - t1
        run2.close()
        if dist is not None:
            t = torch.tensor([e2], dtype=torch.float64, device=wire_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e2 = float(t.item())
        conc = {"images_in_flight_per_gpu": S2, "value": round(float(n) * k2 * S2 * world / e2 / 1e6, 3), "unit": "Mpx/s",
                "steps": k2, "note": "one host thread + HIP stream per image; host-side split-loop work of one image overlaps kernels of another"}
    if dist is not None:
        dist.barrier()

    gather_check = None
    if args.check_gather and dist is not None and rank == 0:
        # rank 0 makes every rank's images itself (the generator is a pure function of the seed), quantises them one call per
        # image, and holds what the collective delivered to that: maps bit for bit, palettes bit for bit
        tmp = L.patolette_amd_malloc(3 * n * 8)
        tmpw = L.patolette_amd_malloc(n * 8) if weighted is True else None
        tmpm = L.patolette_amd_malloc(n)
        opts_c = _native.QuantizationOptions(dither, False, cs, niter, max_samples, False)
        mism = compared = 0
        pal_ok = True
        try:
            ref_cache = {}
            for r in range(world):
                for i in range(args.steps):
                    for j in range(S):
                        src = ((args.warmup + i) * S + j) % pool
                        if (r, src) not in ref_cache:
                            assert L.patolette_amd_fill_image(tmp, n, 100 * r + src) == 0
                            if tmpw:
                                assert L.patolette_amd_fill_weights(tmpw, n, 100 * r + src) == 0
                            pal_c = np.zeros((K, 3), dtype=np.float64, order="F")
                            code_c = C.c_int(0)
                            L.patolette_amd_device(width, height, tmp, tmpw, K, C.byref(opts_c), pal_c.ctypes.data_as(_native.dp), tmpm, 1, C.byref(code_c))
                            L.patolette_amd_synchronize()
                            assert code_c.value == 0, _native.last_error()
                            m_c = np.empty(n, dtype=np.uint8)
                            assert L.patolette_amd_memcpy_d2h(m_c.ctypes.data_as(C.c_void_p), tmpm, n) == 0
                            ref_cache[(r, src)] = (pal_c.copy(), m_c)
                        pal_c, m_c = ref_cache[(r, src)]
                        got_m = gathered[i][r][j].cpu().numpy()
                        got_p = gl_p[r][i * S + j].cpu().numpy()
                        mism += int(np.count_nonzero(got_m != m_c))
                        pal_ok = pal_ok and bool(np.array_equal(got_p, pal_c))
                        compared += 1
        finally:
            for p_ in (tmp, tmpw, tmpm):
                if p_:
                    L.patolette_amd_free(p_)
        gather_check = {"maps_compared": compared, "ranks": world, "map_mismatches": mism, "palettes_identical": pal_ok,
                        "against": "one patolette_amd_device call per image on rank 0"}

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    total_px = float(n) * args.steps * world * S
    value = total_px / elapsed / 1e6
    # ---- roofline of the dominant kernel (most accumulated time in the timed region) ----
    roofline = None
    kernels = {}
    if prof:
        full_steps = 1 if prof_full is not prof else args.steps
        for name, r in prof_full.items():
            if r["launches"] and r["total_ms"] > 0:
                kernels[name] = {"ms_per_step": r["total_ms"] / full_steps, "launches_per_step": r["launches"] / full_steps,
                                 "GBps": r["bytes"] / (r["total_ms"] * 1e-3) / 1e9}
        dom = max(prof, key=lambda k: prof[k]["total_ms"])
        r = prof[dom]
        achieved = r["bytes"] / (r["total_ms"] * 1e-3) / 1e9
        traffic = traffic_source = None
        tpath = os.path.join(ROOT, "profiles", "traffic_%s.json" % args.config)
        if os.path.exists(tpath):       # HBM bytes per launch from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command
            tj = json.load(open(tpath))
            if dom in tj.get("kernels", {}):
                traffic = tj["kernels"][dom]["hbm_bytes_per_launch"]
                # counters cannot be read inside this process: the figure is the one kept from the PMC passes, and says so
                traffic_source = "profiles/traffic_%s.json (%s): rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, not this run" % (
                    args.config, tj.get("collected", "collection date not recorded"))
        roofline = {"kernel": dom, "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                    "avg_launch_us": round(1e3 * r["total_ms"] / r["launches"], 3),
                    "algorithmic_bytes_per_launch": round(r["bytes"] / r["launches"], 1),
                    "time_share": round(kernels.get(dom, {"ms_per_step": 0.0})["ms_per_step"] / max(1e-9, sum(v["ms_per_step"] for v in kernels.values())), 3)}

    # ---- extras of the default run, all outside the timed region ----
    ns_kernels = h2h = h2h_u8 = content = small = dflt = dcontent = None
    if args.full and not args.no_extras and world == 1 and args.config == "c3":
        small = small_image(L, _native)
        dcontent = dither_content(L, _native)
        h2h = host_to_host(L, _native, cfg)
        h2h_u8 = host_to_host_u8(L, _native, cfg)
        dflt = default_call(L, _native)
        ob_c = None
        if not args.no_cpu_baseline:                          # the oracle as the checker of the content workloads (never timed here)
            from oracle import binding as ob_c
        content = content_times(L, _native, cfg, ob_c)
        ns_kernels = north_star_kernels(L, _native)

    # ---- CPU baseline: the oracle (plain-C restatement of the reference path) on this host, same workload ----
    # all-core = the loops the reference's dependencies thread (faiss search / compute_centroids, FLANN's NN search) on every
    # core of the box, the rest single-threaded as in the reference; single_thread = everything on one core.
    cpu = None
    parity = None
    dither_cmp = None
    if args.full and not args.no_cpu_baseline and world == 1:
        from oracle import binding as ob
        ncores = os.cpu_count() or 1
        sw, sh = width, height                                # the full workload (default config: ~10 + ~17 s; c4 / c4map: ~1 min a run)
        if n > 4096 * 4096 and niter > 0 and max_samples > 512 ** 2:
            sw, sh = 4096, 4096                               # c4km: eight Lloyd iterations over 67 M samples take the CPU many minutes
        sn = sw * sh
        flat = ob.image(sn, 0)
        wt = ob.weights(sn, 0) if weighted is True else None
        kms = min(max_samples, sn) if max_samples > 512 ** 2 else max_samples

        def cpu_run(threads):
            ob.set_threads(threads)
            t1 = time.perf_counter()
            w_ = wt
            if weighted == "saliency":               # the reference derives these on the CPU inside quantize(): part of the job
                from oracle import saliency
                w_ = saliency.get_weights(np.ascontiguousarray(flat.reshape(3, sn).T).reshape(sh, sw, 3), 512.0)
            ec, pal_, map_ = ob.patolette(sw, sh, flat, w_, K, dither=dither, color_space=cs, kmeans_niter=niter, kmeans_max_samples=kms)
            dt_ = time.perf_counter() - t1
            ob.set_threads(1)
            return dt_, {k: round(v, 2) for k, v in ob.last_timings().items()}, (ec, pal_, map_)
        dt_all, st_all, res_all = cpu_run(ncores)
        dt_one, st_one, res_one = cpu_run(1)
        if sn == n and weighted != "saliency":
            parity = parity_record(L, _native, cfg, d_imgs[0], d_wts[0] if weighted is True else None, pal_timed, res_all, res_one, ob)
        elif weighted != "saliency":
            # the CPU sample is smaller than the workload: the HIP path quantises the SAME sample (seed 0, same options) once, untimed,
            # and that result is held to the oracle's
            sub_cfg = (sw, sh) + tuple(cfg[2:])
            d_s = L.patolette_amd_malloc(3 * sn * 8)
            d_sw = L.patolette_amd_malloc(sn * 8) if weighted is True else None
            try:
                assert d_s and L.patolette_amd_fill_image(d_s, sn, 0) == 0
                if d_sw:
                    assert L.patolette_amd_fill_weights(d_sw, sn, 0) == 0
                parity = parity_record(L, _native, sub_cfg, d_s, d_sw, None, res_all, res_one, ob)
                if isinstance(parity, dict) and "image" in parity:
                    parity["image"] = "the cpu_baseline sample: %dx%d, seed 0, same options as the workload (the full %dx%d image would take the oracle %.0fx as long)" % (sw, sh, width, height, n / sn)
            finally:
                for q_ in (d_s, d_sw):
                    if q_:
                        L.patolette_amd_free(q_)
        else:
            parity = {"note": "the oracle derives its own saliency weights (unpinned restatement): no comparison in this run; see tests/test_gpu_saliency.py"}
        scale = "the full %dx%d workload" % (sw, sh) if sn == n else "%dx%d of the same workload (the %dx%d image would take %.0fx as long)" % (sw, sh, width, height, n / sn)
        if dither:
            # the mapping stage side by side: the GPU's chain cut into runs walked side by side, one lane or one wavefront each (speculative warm-up,
            # verified boundaries, repairs: map.hip DitherSeg) against the oracle's one chain on one host core.  The oracle
            # searches the palette by brute force (exact, 256 f64 distances per pixel); the reference's FLANN kd-tree
            # (nearest.c:115-148) is not in this image and would be faster on the CPU side.
            dither_cmp = {"gpu_ns_per_px": round(1e6 * stats["ms_map"] / n, 3), "gpu_pixels": n, "gpu_ms_map": round(stats["ms_map"], 3),
                          "runs": stats.get("dither_segments"), "repairs": stats.get("dither_repairs"), "verification_passes": stats.get("dither_rounds"),
                          "cpu_ns_per_px_one_core": round(1e9 * st_one["map"] / sn, 2), "cpu_pixels": sn,
                          "note": "GPU: ms_map of the last timed step / pixels (pixel + palette conversion to linear Rec2020, the Riemersma runs and their "
                                  "boundary checks); CPU: the oracle's map stage (brute-force exact nearest colour, single thread, serial by construction) "
                                  "on the %dx%d image" % (sw, sh)}
        cpu = {"value": round(sn / dt_all / 1e6, 4), "unit": "Mpx/s", "cores": ncores, "kind": "port",
               "sample": "oracle (plain-C restatement of the reference path; KMeans assign/update and the NN map on %d threads as faiss / FLANN "
                         "thread them, everything else single-threaded as in the reference) on %s, %.1f s; stages %s" % (ncores, scale, dt_all, st_all),
               "single_thread": {"value": round(sn / dt_one / 1e6, 4), "cores": 1, "seconds": round(dt_one, 1), "stages": st_one}}

    out = {
        "metric": ("Mpixels/sec quantized (256-color ICtCp + KMeans) at %s; palette \u0394E vs ref" % ("1 GPU" if world == 1 else "%d GPUs" % world))
                  if args.config.startswith("c3") else "Mpixels/sec quantized; palette \u0394E vs ref",
        "value": round(value, 3), "unit": "Mpx/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": desc, "kmeans_update": ("order-free exact sums (OPTION, NOT a parity result: palette ~1e-4 of the colour range from the reference's after 32 "
                                                        "iterations -- outside north_star's 1e-5 --, ~0.02 % of the index map differs)"
                                                        if args.kmeans_update else "reference (sequential f32 chains, bit-exact)"),
                   "width": width, "height": height, "palette_size": K, "images_per_step_per_gpu": S,
                   "input": "uniform random sRGB (splitmix64), planar f64, resident in HBM; index map left in HBM as u8",
                   "cached_between_steps": "the dither's curve order (rank along the Hilbert curve -> pixel number: a pure function of width and height) and "
                                           "the KMeans subsample index list (faiss rand_perm(N, seed 1234): a pure function of N) stay on the device "
                                           "between calls; a first call makes it on a helper thread beside conversion and the quantisers -- "
                                           "`first_call` is the same step with the list made again in every call; a pool of <= 3 distinct images "
                                           "rotates through the steps",
                   "kernel_events_in_timed_region": ("none" if not profile else
                                                     ("dominant kernel only (%s), every %d-th launch (two event records cost ~12 us per launch); "
                                                      "per-kernel table from one extra untimed step" % (dom_name, EVENT_SAMPLE)
                                                      if dom_name else "all kernels")),
                   "final_gather": ("none (1 GPU)" if dist is None else
                                    "TEST MODE --oversubscribe: %d ranks on %d device(s), gloo gather through host copies -- the N > 1 code path, not a scaling figure" % (world, L.patolette_amd_device_count())
                                    if args.oversubscribe else
                                    "RCCL gather of u8 maps (per step, asynchronous, overlapping the next step) + f64 palettes to rank 0, inside the timed region")},
        "first_call": cold, "dither": dither_cmp, "parity": parity, "gather_check": gather_check, "roofline": roofline, "cpu_baseline": cpu, "north_star_kernels": ns_kernels, "small_image": small, "host_to_host": h2h, "host_to_host_u8": h2h_u8, "default_call": dflt, "dither_content": dcontent, "content": content, "throughput_concurrent": conc,
        "stages_ms_last_step": {k: round(v, 3) for k, v in stats.items() if k.startswith("ms_")},
        "run": {k: v for k, v in stats.items() if not k.startswith("ms_")},
        "kernels": {k: {kk: round(vv, 3) for kk, vv in v.items()} for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_step"])},
    }
    if dist is not None:
        dist.destroy_process_group()
    # the JSON line is the last thing on stdout: RCCL's banner sits in the C library's stdout buffer until it is flushed
    sys.stdout.flush()
    try:
        C.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
