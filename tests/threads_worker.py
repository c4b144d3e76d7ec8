"""Worker of tests/test_gpu_threads.py: one child process per scenario, caller threads that overlap in time.

    python threads_worker.py <scenario> <out.npz> [args]

The job table below is what every scenario runs.  A job is one seeded call of one entry point; `run_job` returns everything the
call reports as named arrays.  The `serial` scenario walks the table once on one thread and saves the arrays as they are; every
other scenario saves what its threads got under "<thread>/<pass>/<job>/<field>" -- arrays above one MiB as their SHA-256
(`digest`), so that a soak of eighteen walks stays a few tens of megabytes -- and the parent compares them with the serial file.
No scenario judges a result itself: the child only reports (and exits non-zero at once when a thread does not come back).

Inputs are made as the other modules make them (oracle.binding.image / weights, tests.util.scene, seeded numpy generators); the
table and its inputs are built on the main thread before any caller thread starts and are only read afterwards.
"""
import ctypes as C
import hashlib
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

THREADS = 6
JOIN_TIMEOUT = 900.0          # seconds a thread may take before the child gives up (the parent's own limit is usually shorter)
BIG = 1 << 20                 # arrays above this many bytes travel as their digest
POISON, COUNT, LOG = 1, 2, 4
REMAP_BOTH_MISSING = "patolette_amd_remap: pass exactly one of palette and palette_u8"


def digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(("%s %s " % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


class Job:
    """entry: host | device | u8 | rgba | frames | remap | batch_u8.  `oracle`: small enough for the CPU oracle to answer in
    seconds (the parent compares those with it)."""

    def __init__(self, name, entry, oracle, **kw):
        self.name, self.entry, self.oracle = name, entry, oracle
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def _colors(n, seed):
    from oracle import binding as ob
    return ob.image(n, seed).reshape(3, n).T.copy()


def _scene_u8(h, w, seed):
    from tests.util import scene
    return np.round(scene(h, w, seed) * 255).astype(np.uint8)


def _noise_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _blobs(h, w, seed, frac=0.35):
    """A random-blob mask (True = transparent), as tests/test_gpu_rgba.py makes it."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    while m.mean() < frac:
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(2, max(3, min(h, w) // 5))
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return m


def _byte_palette(rows, seed):
    """`rows` distinct byte colours, as tests/test_gpu_remap.py makes them."""
    codes = np.random.default_rng(seed).choice(1 << 24, size=rows, replace=False)
    return np.stack([codes >> 16, (codes >> 8) & 255, codes & 255], axis=1).astype(np.uint8)


_TABLE = None


def table():
    """The jobs, inputs included; built once."""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    from oracle import binding as ob
    jobs = []

    def host(name, w, h, K, seed, oracle=True, weights=False, **opts):
        kw = dict(dither=False, color_space=2, tile_size=0.0, kmeans_niter=0, kmeans_max_samples=512 ** 2)
        kw.update(opts)
        jobs.append(Job(name, "host", oracle, w=w, h=h, K=K, img=_colors(w * h, seed), wts=ob.weights(w * h, seed) if weights else None,
                        kw=kw))

    # K <= 12: the global quantiser's decisions on the host; sRGB, no dither, no KMeans
    host("host_k8_srgb", 160, 120, 8, 31, color_space=0)
    # 13 <= K <= 256: the device-driven loop; CIELuv, dither, explicit weights, sampled KMeans (76 800 pixels > 4096 samples)
    host("host_k64_luv_dither_weights_kmsampled", 320, 240, 64, 32, weights=True, dither=True, color_space=1, kmeans_niter=3,
         kmeans_max_samples=4096)
    # K > 256: the host-driven loop; ICtCp, KMeans over every pixel
    host("host_k300_kmfull", 256, 192, 300, 33, kmeans_niter=2, kmeans_max_samples=1 << 30)
    # saliency-derived weights (tile_size > 0) on a scene
    h, w = 150, 200
    jobs.append(Job("host_k32_tile", "host", False, w=w, h=h, K=32, wts=None,
                    img=(_scene_u8(h, w, 34).reshape(-1, 3).astype(np.float64) / 255.0),
                    kw=dict(dither=False, color_space=2, tile_size=512.0, kmeans_niter=0, kmeans_max_samples=512 ** 2)))
    # K = 256 with KMeans over every pixel: the KMeans kernels with the largest tables (and the cold same-job scenario)
    host("host_k256_kmfull", 384, 256, 256, 35, oracle=False, kmeans_niter=3, kmeans_max_samples=1 << 30)
    # inputs and map in HBM
    jobs.append(Job("device_k40_weights", "device", True, w=512, h=384, K=40, img=_colors(512 * 384, 36), wts=ob.weights(512 * 384, 36),
                    kw=dict(dither=False, color_space=2, tile_size=0.0, kmeans_niter=2, kmeans_max_samples=512 ** 2)))
    # the 8-bit entry, dithered, at a size where one lane walks each run (checked by the parent: dither_layout_in_use)
    jobs.append(Job("u8_k64_dither_lanes", "u8", True, K=64, img=_scene_u8(384, 512, 37), wts=None,
                    kw=dict(dither=True, color_space=2, tile_size=0.0, kmeans_niter=0, kmeans_max_samples=512 ** 2)))
    # RGBA with a blob mask, dithered
    im = np.concatenate([_scene_u8(96, 128, 38), np.zeros((96, 128, 1), np.uint8)], axis=2)
    tr = _blobs(96, 128, 38)
    im[..., 3] = np.where(tr, 127, 255)
    jobs.append(Job("rgba_k24_blobs_dither", "rgba", True, K=24, img=im, transparent=tr, wts=None,
                    kw=dict(dither=True, color_space=2, tile_size=0.0, kmeans_niter=0, kmeans_max_samples=512 ** 2)))
    # five frames, one palette, dithered
    fr = np.ascontiguousarray(np.stack([_scene_u8(64, 96, 39 + 7 * i) for i in range(5)]))
    jobs.append(Job("frames5_k16_dither", "frames", True, K=16, img=fr, wts=None,
                    kw=dict(dither=True, color_space=2, tile_size=0.0, kmeans_niter=6, kmeans_max_samples=4096)))
    # remap, nearest, 2^22 pixels and 64 rows: the fused byte kernel and the once-per-device bounds box
    jobs.append(Job("remap_nearest_fused", "remap", False, img=_noise_u8((2048, 2048, 3), 40), palette=_byte_palette(64, 40), dither=False))
    # remap, dithered, three frames
    fr3 = np.ascontiguousarray(np.stack([_scene_u8(64, 96, 41 + 7 * i) for i in range(3)]))
    jobs.append(Job("remap_dither_frames3", "remap", True, img=fr3, palette=_byte_palette(16, 41), dither=True))
    # above 2 Mpixel through the host entry: the chunked upload and its helper thread; sampled KMeans
    host("host_k128_chunked", 1536, 1408, 128, 42, oracle=False, kmeans_niter=2)
    # the batch entry from a caller thread: the library's own workers beside the caller threads
    jobs.append(Job("batch_u8_x3_k32", "batch_u8", False, K=32, img=[_noise_u8((200, 300, 3), 43 + i) for i in range(3)], wts=None,
                    kw=dict(dither=False, color_space=2, tile_size=0.0, kmeans_niter=2, kmeans_max_samples=512 ** 2)))
    _TABLE = jobs
    return jobs


def job(name):
    for j in table():
        if j.name == name:
            return j
    raise KeyError(name)


def setup_process(L):
    """The one process-wide knob every child (and the parent's checks) sets before any call: one lane per dither run from
    65 536 pixels on, so that a small image takes the layout large images take by default."""
    L.patolette_amd_dither_layout(1)


def _state(native, L, K, out, trace=True):
    """what the calling thread's engine reports about the call just made"""
    st = native.last_stats()
    out["stats"] = np.array([st["n_clusters"], st["n_base_clusters"], st["kmeans_samples"], st["dither_segments"]], dtype=np.int64)
    if trace:
        tr = native.last_split_trace()
        out["header"] = np.array([tr["n_base"], tr["n_clusters"], int(tr["stopped_early"]), len(tr["splits"])] + list(tr["gq_cuts"]),
                                 dtype=np.int64)
        out["centers"] = native.last_cluster_centers()
    buf = np.zeros(3 * max(1, K))
    n = L.patolette_amd_last_map_palette(buf.ctypes.data_as(native.dp), max(1, K))
    out["map_palette"] = buf.reshape(3, max(1, K))[:, :n].T.copy()


def run_job(j):
    """One call on the calling thread's engine -> {field: array}.  A failed call raises."""
    import patolette_amd as p
    from patolette_amd import _native as native
    L = native.lib()
    out = {}
    if j.entry == "host":
        ok, pal, pmap, msg = p.quantize(j.w, j.h, j.img, j.K, weights=j.wts, **j.kw)
        assert ok, "%s: %s / %s" % (j, msg, native.last_error())
        out.update(pal=np.array(pal), map=np.array(pmap))
        _state(native, L, j.K, out)
    elif j.entry == "device":
        n = j.w * j.h
        d_img, d_w, d_map = L.patolette_amd_malloc(3 * n * 8), L.patolette_amd_malloc(n * 8), L.patolette_amd_malloc(n)
        try:
            assert d_img and d_w and d_map, "%s: device allocation failed" % j
            flat = np.ascontiguousarray(j.img.T).reshape(-1)
            assert L.patolette_amd_memcpy_h2d(d_img, flat.ctypes.data_as(C.c_void_p), flat.nbytes) == 0
            assert L.patolette_amd_memcpy_h2d(d_w, j.wts.ctypes.data_as(C.c_void_p), j.wts.nbytes) == 0
            k = j.kw
            opts = native.QuantizationOptions(k["dither"], False, k["color_space"], k["kmeans_niter"], k["kmeans_max_samples"], False)
            pal = np.zeros((j.K, 3), dtype=np.float64, order="F")
            code = C.c_int(9)
            L.patolette_amd_device(j.w, j.h, d_img, d_w, j.K, C.byref(opts), pal.ctypes.data_as(native.dp), d_map, 1, C.byref(code))
            assert code.value == 0, "%s: %s" % (j, native.last_error())
            pmap = np.empty(n, dtype=np.uint8)
            assert L.patolette_amd_memcpy_d2h(pmap.ctypes.data_as(C.c_void_p), d_map, n) == 0
        finally:
            for d in (d_img, d_w, d_map):
                if d:
                    L.patolette_amd_free(d)
        out.update(pal=pal, map=pmap)
        _state(native, L, j.K, out)
    elif j.entry == "u8":
        ok, pal8, pmap, quant, pal, msg = p.quantize_u8(j.img, j.K, weights=j.wts, **j.kw)
        assert ok, "%s: %s / %s" % (j, msg, native.last_error())
        out.update(pal=np.array(pal), pal8=pal8, map=pmap, quant=quant)
        _state(native, L, j.K, out)
    elif j.entry == "rgba":
        ok, prgba, pmap, quant, pal, tidx, msg = p.quantize_rgba(j.img, j.K, weights=j.wts, **j.kw)
        assert ok, "%s: %s / %s" % (j, msg, native.last_error())
        out.update(pal=np.array(pal), pal8=prgba, map=pmap, quant=quant, tidx=np.array([tidx], dtype=np.int64))
        _state(native, L, j.K, out)
    elif j.entry == "frames":
        ok, pal8, maps, quant, pal, msg = p.quantize_frames(j.img, j.K, weights=j.wts, **j.kw)
        assert ok, "%s: %s / %s" % (j, msg, native.last_error())
        out.update(pal=np.array(pal), pal8=pal8, map=maps, quant=quant)
        _state(native, L, j.K, out)
    elif j.entry == "remap":
        ok, pmap, quant, msg = p.remap(j.img, j.palette, dither=j.dither)
        assert ok, "%s: %s / %s" % (j, msg, native.last_error())
        out.update(map=pmap, quant=quant)
        _state(native, L, j.palette.shape[0], out, trace=False)     # (no quantiser ran: the header promises its stats are 0)
    else:
        assert j.entry == "batch_u8"
        res = p.quantize_u8_batch(j.img, j.K, weights=None, **j.kw)
        for i, r in enumerate(res):
            assert r[0], "%s image %d: %s" % (j, i, r[-1])
            out.update({"pal_%d" % i: np.array(r[4]), "pal8_%d" % i: r[1], "map_%d" % i: r[2], "quant_%d" % i: r[3]})
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


class Sink:
    """what the child writes: arrays by key, large ones as digests unless `full`"""

    def __init__(self, full=False):
        self.full, self.d, self.mu = full, {}, threading.Lock()

    def put(self, prefix, res):
        with self.mu:
            for k, v in res.items():
                if self.full or v.nbytes <= BIG:
                    self.d["%s/%s" % (prefix, k)] = v
                else:
                    self.d["%s/%s#sha256" % (prefix, k)] = digest(v)

    def note(self, key, value):
        with self.mu:
            self.d[key] = np.asarray(value)

    def save(self, path):
        np.savez(path, **self.d)


_BARRIERS = []


def _barrier(parties):
    b = threading.Barrier(parties)
    _BARRIERS.append(b)
    return b


def _abort_barriers():
    """a thread that failed will not arrive: the ones waiting for it fail too instead of waiting out their limit"""
    for b in _BARRIERS:
        b.abort()


def run_threads(targets, sink):
    """Start one thread per target, join each with a limit.  A thread that raised is recorded ("errors") and the child goes on
    to write its file; a thread that does not come back ends the child at once, non-zero."""
    errors = []

    def wrap(fn, tag):
        def go():
            try:
                fn()
            except BaseException as ex:     # noqa: B902  (reported, not swallowed)
                import traceback
                _abort_barriers()
                errors.append("%s: %s\n%s" % (tag, ex, traceback.format_exc()))
        return go
    ts = [threading.Thread(target=wrap(fn, tag), name=tag, daemon=True) for tag, fn in targets]
    for t in ts:
        t.start()
    join_all(ts)
    return errors


def join_all(ts):
    deadline = time.monotonic() + JOIN_TIMEOUT
    for t in ts:
        t.join(max(0.0, deadline - time.monotonic()))
        if t.is_alive():
            sys.stderr.write("threads_worker: thread %s did not come back within %.0f s\n" % (t.name, JOIN_TIMEOUT))
            sys.stderr.flush()
            os._exit(3)


def finish(sink, errors, out_path, t0):
    sink.note("wall_seconds", time.monotonic() - t0)
    sink.note("errors", np.array(errors, dtype=np.str_) if errors else np.zeros(0, dtype=np.str_))
    sink.save(out_path)
    for e in errors:
        sys.stderr.write("threads_worker: %s\n" % e)
    print("THREADS-WORKER-DONE %d errors" % len(errors))
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(1 if errors else 0)       # (no interpreter teardown with idle engines in the pool: nothing more to learn from it)


def _lib():
    from patolette_amd import _native as native
    return native, native.lib()


# ---- scenarios ----------------------------------------------------------------------------------------------------------------
def sc_serial(out_path, args):
    """the table once on the main thread"""
    jobs = table()
    native, L = _lib()
    t0 = time.monotonic()
    setup_process(L)
    sink = Sink(full=True)
    for j in jobs:
        sink.put(j.name, run_job(j))
    sink.note("late_growths", L.patolette_amd_debug_late_growths())
    finish(sink, [], out_path, t0)


def _walk(sink, tag, jobs, start, passes, barrier=None):
    def go():
        for r in range(passes):
            for i in range(len(jobs)):
                j = jobs[(start + i) % len(jobs)]
                if barrier is not None and r == 0 and i == 0:
                    barrier.wait(JOIN_TIMEOUT)          # every thread's FIRST library call at the same moment
                sink.put("%s/%d/%s" % (tag, r, j.name), run_job(j))
    return go


def sc_cold_mixed(out_path, args):
    """six threads, first call together on six different jobs, then the rest of the table"""
    jobs = table()
    native, L = _lib()                       # loading and typing the library is no call into it ...
    t0 = time.monotonic()
    setup_process(L)                         # ... and this one stores an int
    sink, barrier = Sink(), _barrier(THREADS)
    step = len(jobs) // THREADS
    errors = run_threads([("t%d" % t, _walk(sink, "t%d" % t, jobs, t * step, 1, barrier)) for t in range(THREADS)], sink)
    finish(sink, errors, out_path, t0)


def sc_cold_same(out_path, args):
    """six threads, first call together on the SAME job (args[0]), twice each"""
    j = job(args[0])
    native, L = _lib()
    t0 = time.monotonic()
    setup_process(L)
    sink, barrier = Sink(), _barrier(THREADS)
    errors = run_threads([("t%d" % t, _walk(sink, "t%d" % t, [j], 0, 2, barrier)) for t in range(THREADS)], sink)
    finish(sink, errors, out_path, t0)


def sc_soak(out_path, args):
    """six threads, each from its own offset, R passes, fresh memory poisoned and late growths counted"""
    passes = int(args[0]) if args else 3
    jobs = table()
    native, L = _lib()
    t0 = time.monotonic()
    setup_process(L)
    prev = L.patolette_amd_debug_workspace(0)
    L.patolette_amd_debug_workspace(prev | POISON | COUNT | LOG)       # (a late growth is named on stderr)
    late0 = L.patolette_amd_debug_late_growths()
    sink = Sink()
    step = len(jobs) // THREADS
    errors = run_threads([("t%d" % t, _walk(sink, "t%d" % t, jobs, t * step + 1, passes)) for t in range(THREADS)], sink)
    sink.note("late_growths", L.patolette_amd_debug_late_growths() - late0)
    L.patolette_amd_debug_workspace(prev)
    finish(sink, errors, out_path, t0)


def _hip_runtime():
    """the HIP runtime libpatolette_amd.so has loaded, for hipMemGetInfo (the library exports no such query)"""
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if "libamdhip64" in os.path.basename(path):
                return C.CDLL(path)
    raise RuntimeError("libamdhip64 is not mapped into this process")


def _free_bytes(hip):
    free, total = C.c_size_t(0), C.c_size_t(0)
    rc = hip.hipMemGetInfo(C.byref(free), C.byref(total))
    assert rc == 0, "hipMemGetInfo -> %d" % rc
    return free.value


def sc_churn(out_path, args):
    """Two long-lived threads walk the table while short-lived threads run one job each and exit and the main thread releases the
    workspace again and again, making a call of its own after every release.  Then, with everything released, two threads run
    the largest quantisation and exit; free device memory is recorded before they start (`free_before_tail`), after they have
    exited (`free_idle`) and after one more release (`free_end`)."""
    jobs = table()
    small = [j for j in jobs if j.oracle]
    native, L = _lib()
    t0 = time.monotonic()
    setup_process(L)
    assert L.patolette_amd_device_count() >= 1
    hip = _hip_runtime()
    sink = Sink()
    errors = []
    long_ts = []
    for t in range(2):
        tag = "long%d" % t
        fn = _walk(sink, tag, jobs, t * (len(jobs) // 2), 2)
        long_ts.append(threading.Thread(target=_guard(fn, tag, errors), name=tag, daemon=True))
    for t in long_ts:
        t.start()
    rounds = 0
    while rounds < 4 or (any(t.is_alive() for t in long_ts) and rounds < 12):
        pair = []
        for s in range(2):
            j = small[(2 * rounds + s) % len(small)]
            tag = "short%d" % (2 * rounds + s)
            fn = (lambda j=j, tag=tag: sink.put("%s/0/%s" % (tag, j.name), run_job(j)))
            pair.append(threading.Thread(target=_guard(fn, tag, errors), name=tag, daemon=True))
        for t in pair:
            t.start()
        join_all(pair)                                   # both have exited: their engines are back in the pool, idle
        L.patolette_amd_release_workspace()              # ... and go, with the main thread's own; the long-lived threads' are in use
        j = small[rounds % len(small)]
        try:
            sink.put("main%d/0/%s" % (rounds, j.name), run_job(j))      # the call after a release
        except BaseException as ex:     # noqa: B902
            errors.append("main%d: %s" % (rounds, ex))
        rounds += 1
    join_all(long_ts)
    sink.note("release_rounds", rounds)
    L.patolette_amd_release_workspace()
    # two more threads run the largest quantisation and exit: their engines, sized for it, are back in the pool, idle
    sink.note("free_before_tail", _free_bytes(hip))
    big = job("host_k128_chunked")
    tail = []
    for t in range(2):
        tag = "tail%d" % t
        fn = (lambda tag=tag: sink.put("%s/0/%s" % (tag, big.name), run_job(big)))
        tail.append(threading.Thread(target=_guard(fn, tag, errors), name=tag, daemon=True))
    for t in tail:
        t.start()
    join_all(tail)
    sink.note("tail_pixels", big.w * big.h)
    sink.note("free_idle", _free_bytes(hip))
    L.patolette_amd_release_workspace()
    sink.note("free_end", _free_bytes(hip))
    j = small[0]
    sink.put("after/0/%s" % j.name, run_job(j))
    finish(sink, errors, out_path, t0)


def _guard(fn, tag, errors):
    def go():
        try:
            fn()
        except BaseException as ex:     # noqa: B902
            import traceback
            _abort_barriers()
            errors.append("%s: %s\n%s" % (tag, ex, traceback.format_exc()))
    return go


STATE_JOBS = ("host_k64_luv_dither_weights_kmsampled", "host_k8_srgb", "device_k40_weights", "host_k300_kmfull")


def sc_state(out_path, args):
    """Threads A and B in lockstep.  A: invariant sums on, a call that fails on its arguments, then good calls.  B: invariant sums
    off, good calls with another K at the same moments.  Each reads its own last_error / last_stats / last_split_trace only after
    BOTH have finished the step, so a state shared between them would show the other's call.  Before the threads start, the main
    thread runs the same jobs with invariant sums on ("serial_invariant"): what A must get."""
    jobs = [job(n) for n in STATE_JOBS]
    native, L = _lib()
    t0 = time.monotonic()
    setup_process(L)
    sink, bar = Sink(), _barrier(2)

    def bad_call():
        img = _noise_u8((32, 48, 3), 1)
        pmap = np.zeros((32, 48), dtype=np.uint8)
        code = C.c_int(9)
        L.patolette_amd_remap_u8(1, 48, 32, img.ctypes.data_as(C.c_void_p), 3, None, None, 16, 0, pmap.ctypes.data_as(C.c_void_p), 1,
                                 None, C.byref(code))
        return code.value

    def thread(tag, invariant, order, fails):
        def go():
            sink.note("%s/invariant_before" % tag, L.patolette_amd_set_invariant_sums(invariant))
            bar.wait(JOIN_TIMEOUT)
            if fails:
                sink.note("%s/bad_exit_code" % tag, bad_call())
            else:
                sink.put("%s/0/%s" % (tag, jobs[1].name), run_job(jobs[1]))
            bar.wait(JOIN_TIMEOUT)                        # both calls are over
            sink.note("%s/last_error_after_step1" % tag, np.str_(native.last_error()))
            bar.wait(JOIN_TIMEOUT)
            for r, i in enumerate(order):                 # the two threads are always in DIFFERENT jobs (another K, another path)
                bar.wait(JOIN_TIMEOUT)
                j = jobs[i]
                # the call; the per-thread state is read once the OTHER thread's call is over too: it must still be this call's
                sink.put("%s/%d/%s" % (tag, r + 1, j.name), run_job_split(j, lambda: bar.wait(JOIN_TIMEOUT)))
            sink.note("%s/invariant_after" % tag, L.patolette_amd_set_invariant_sums(invariant))
        return go

    # what A must get: the same jobs on one thread with the setting on (the main thread's own setting; no other thread sees it)
    L.patolette_amd_set_invariant_sums(1)
    for j in jobs:
        sink.put("serial_invariant/0/%s" % j.name, run_job(j))
    L.patolette_amd_set_invariant_sums(0)
    errors = run_threads([("A", thread("A", 1, (0, 1, 2, 3), True)), ("B", thread("B", 0, (1, 0, 3, 2), False))], sink)
    finish(sink, errors, out_path, t0)


def run_job_split(j, between):
    """run_job for the host / device entries with `between()` called after the call returned and before the thread's state is
    read: the arrays come from the call, the stats / trace / map palette from what the engine reports afterwards."""
    native, L = _lib()
    res = run_job(j)
    between()
    late = {}
    _state(native, L, j.K, late)
    for k, v in late.items():
        res[k] = np.ascontiguousarray(v)
    return res


def sc_two_devices(out_path, args):
    """three threads on device 0, three on device 1, each walking the table once"""
    jobs = table()
    native, L = _lib()
    t0 = time.monotonic()
    setup_process(L)
    sink, barrier = Sink(), _barrier(THREADS)
    step = len(jobs) // THREADS

    def on(dev, fn):
        def go():
            assert L.patolette_amd_set_device(dev) == 0
            fn()
        return go
    errors = run_threads([("t%d" % t, on(t % 2, _walk(sink, "t%d" % t, jobs, t * step, 1, barrier))) for t in range(THREADS)], sink)
    finish(sink, errors, out_path, t0)


SCENARIOS = dict(serial=sc_serial, cold_mixed=sc_cold_mixed, cold_same=sc_cold_same, soak=sc_soak, churn=sc_churn, state=sc_state,
                 two_devices=sc_two_devices)

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](sys.argv[2], sys.argv[3:])
