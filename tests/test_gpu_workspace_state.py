"""A result must not depend on what the engine's workspace held before the call.

Every calling thread works on a pooled engine whose buffers are kept between calls (pipeline.hip Engine).  A batch must return
what separate calls return, and a call must return the same bits whether its engine is fresh (right after
patolette_amd_release_workspace), stale (its buffers hold another, larger image's state, so nothing regrows) or one of six
pooled engines on their first call in flight together.  patolette_amd_debug_workspace (tests only) makes such a dependence
visible: bit 0 fills fresh f64 / f32 memory and the node table's floating-point fields with NaN (integers are never touched),
bit 1 counts growths that free or move an allocation while the engine's streams still hold queued work.

Each situation below runs once; the configurations cover the branches where the workspace is used differently: K <= 12 (the
global quantiser's decisions on the host), 13 <= K <= 256 (k_gq_control and the device-driven split loop), K > 256 (the
host-driven loop); KMeans off, sampled and over every pixel; dither on and off; explicit, saliency-derived and no weights; the
host, device and 8-bit entry points; an image above 2 Mpixel (the chunked upload)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON, COUNT = 1, 2


@pytest.fixture
def ws(gpu):
    """Late growths counted for the test's duration (whatever the environment set stays on); the previous flags come back."""
    prev = gpu.patolette_amd_debug_workspace(0)
    gpu.patolette_amd_debug_workspace(prev | COUNT)

    def set_poison(on):
        cur = gpu.patolette_amd_debug_workspace(0)
        gpu.patolette_amd_debug_workspace((cur | POISON) if on or prev & POISON else (cur & ~POISON))
    yield set_poison
    gpu.patolette_amd_debug_workspace(prev)


def _release(gpu):
    gpu.patolette_amd_release_workspace()


def _colors(n, seed):
    from oracle import binding as ob
    return ob.image(n, seed).reshape(3, n).T.copy()


class Cfg:
    def __init__(self, name, entry, w, h, K, seed, dither=False, kmeans_niter=0, kmeans_max_samples=512 ** 2, weights=False,
                 tile_size=0.0, color_space=2):
        self.name, self.entry, self.w, self.h, self.K, self.seed = name, entry, w, h, K, seed
        self.dither, self.kmeans_niter, self.kmeans_max_samples = dither, kmeans_niter, kmeans_max_samples
        self.weights, self.tile_size, self.color_space = weights, tile_size, color_space
        n = w * h
        if entry == "u8":
            rng = np.random.default_rng(seed)
            self.img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        else:
            self.img = _colors(n, seed)
        from oracle import binding as ob
        self.wts = ob.weights(n, seed) if weights else None

    def kw(self):
        return dict(dither=self.dither, color_space=self.color_space, tile_size=self.tile_size, kmeans_niter=self.kmeans_niter,
                    kmeans_max_samples=self.kmeans_max_samples)

    def __repr__(self):
        return self.name


CONFIGS = [
    # K <= 12: the global quantiser's decisions on the host; KMeans off, no weights, no dither
    Cfg("host_k8_plain", "host", 160, 120, 8, 11),
    # 13 <= K <= 256: k_gq_control + device-driven loop; sampled KMeans (N > 512^2), dither, explicit weights
    Cfg("host_k64_dither_weights_kmsampled", "host", 640, 480, 64, 12, dither=True, kmeans_niter=3, weights=True),
    # K = 256 through the 8-bit entry; KMeans over every pixel, saliency weights
    Cfg("u8_k256_saliency_kmfull", "u8", 300, 200, 256, 13, kmeans_niter=4, kmeans_max_samples=1 << 30, tile_size=512.0),
    # K > 256: the host-driven split loop
    Cfg("host_k300_hostloop", "host", 256, 192, 300, 14, color_space=1),
    # the device entry (inputs and map in HBM), weighted
    Cfg("device_k40_weights", "device", 512, 384, 40, 15, weights=True, kmeans_niter=2),
    # above 2 Mpixel: the chunked upload with the conversion behind it; sampled KMeans
    Cfg("host_k128_chunked", "host", 1536, 1408, 128, 16, kmeans_niter=2),
    # the 8-bit entry above 2 Mpixel, dithered, K <= 12
    Cfg("u8_k12_chunked_dither", "u8", 1536, 1408, 12, 17, dither=True),
]


def _single(gpu, native, cfg):
    """One call on this thread's engine: everything the call reports, for a bit-for-bit comparison."""
    import patolette_amd as p
    n = cfg.w * cfg.h
    if cfg.entry == "host":
        ok, pal, pmap, msg = p.quantize(cfg.w, cfg.h, cfg.img, cfg.K, weights=cfg.wts, **cfg.kw())
        assert ok, msg
    elif cfg.entry == "u8":
        ok, _p8, pmap, _q, pal, msg = p.quantize_u8(cfg.img, cfg.K, weights=cfg.wts, want_quantized=False, **cfg.kw())
        assert ok, msg
        pmap = pmap.reshape(-1)
    else:
        d_img = gpu.patolette_amd_malloc(3 * n * 8)
        d_w = gpu.patolette_amd_malloc(n * 8) if cfg.wts is not None else None
        d_map = gpu.patolette_amd_malloc(n)
        try:
            flat = np.ascontiguousarray(cfg.img.T).reshape(-1)
            assert gpu.patolette_amd_memcpy_h2d(d_img, flat.ctypes.data_as(C.c_void_p), flat.nbytes) == 0
            if d_w:
                assert gpu.patolette_amd_memcpy_h2d(d_w, cfg.wts.ctypes.data_as(C.c_void_p), cfg.wts.nbytes) == 0
            k = cfg.kw()
            opts = native.QuantizationOptions(k["dither"], False, k["color_space"], k["kmeans_niter"], k["kmeans_max_samples"], False)
            pal = np.zeros((cfg.K, 3), dtype=np.float64, order="F")
            code = C.c_int(9)
            gpu.patolette_amd_device(cfg.w, cfg.h, d_img, d_w, cfg.K, C.byref(opts), pal.ctypes.data_as(native.dp), d_map, 1,
                                     C.byref(code))
            assert code.value == 0, native.last_error()
            pmap = np.empty(n, dtype=np.uint8)
            assert gpu.patolette_amd_memcpy_d2h(pmap.ctypes.data_as(C.c_void_p), d_map, n) == 0
        finally:
            for d in (d_img, d_w, d_map):
                if d:
                    gpu.patolette_amd_free(d)
    tr = native.last_split_trace()
    st = native.last_stats()
    header = (tr["n_base"], tr["n_clusters"], tr["stopped_early"], tuple(tr["gq_cuts"]), len(tr["splits"]))
    return dict(pal=np.array(pal), map=np.array(pmap).astype(np.int64), centers=native.last_cluster_centers(), header=header,
                n_clusters=st["n_clusters"], n_base=st["n_base_clusters"])


def _batch(cfg, copies=6):
    """The image `copies` times through the batch entry (six engines in flight)."""
    import patolette_amd as p
    if cfg.entry == "u8":
        res = p.quantize_u8_batch([cfg.img] * copies, cfg.K, weights=[cfg.wts] * copies if cfg.wts is not None else None,
                                  want_quantized=False, **cfg.kw())
        out = []
        for r in res:
            assert r[0], r[-1]
            out.append((np.array(r[4]), r[2].reshape(-1).astype(np.int64)))
        return out
    res = p.quantize_batch(cfg.w, cfg.h, [cfg.img] * copies, cfg.K, weights=[cfg.wts] * copies if cfg.wts is not None else None,
                           **cfg.kw())
    out = []
    for r in res:
        assert r[0], r[3]
        out.append((np.array(r[1]), np.array(r[2]).astype(np.int64)))
    return out


def _same(a, b):
    """bit for bit: palette, map, centres, trace header, counts"""
    diffs = []
    if a["pal"].tobytes() != b["pal"].tobytes():
        diffs.append("palette (max diff %.3g)" % np.nanmax(np.abs(a["pal"] - b["pal"])))
    if not np.array_equal(a["map"], b["map"]):
        diffs.append("map (%d mismatches)" % int(np.sum(a["map"] != b["map"])))
    if a["centers"].shape != b["centers"].shape or a["centers"].tobytes() != b["centers"].tobytes():
        diffs.append("cluster centres")
    for k in ("header", "n_clusters", "n_base"):
        if a[k] != b[k]:
            diffs.append("%s %s vs %s" % (k, a[k], b[k]))
    return diffs


def _same_batch(ref, got):
    diffs = []
    for i, (pal, pmap) in enumerate(got):
        if pal.tobytes() != ref["pal"].tobytes():
            diffs.append("image %d palette (max diff %.3g)" % (i, np.nanmax(np.abs(pal - ref["pal"]))))
        if not np.array_equal(pmap, ref["map"]):
            diffs.append("image %d map (%d mismatches)" % (i, int(np.sum(pmap != ref["map"]))))
    return diffs


# a larger image with another palette size and other options: after it, every buffer of the engine holds real state of
# another image and (for the configurations above) nothing regrows
OTHER = dict(w=1600, h=1440, K=200, seed=99)


def _other(gpu):
    import patolette_amd as p
    n = OTHER["w"] * OTHER["h"]
    from oracle import binding as ob
    ok, _pal, _map, msg = p.quantize(OTHER["w"], OTHER["h"], _colors(n, OTHER["seed"]), OTHER["K"], dither=True, color_space=0,
                                     tile_size=512.0, kmeans_niter=3, kmeans_max_samples=1 << 30, weights=None)
    assert ok, msg
    ok, *_rest = p.quantize_u8(np.random.default_rng(98).integers(0, 256, size=(OTHER["h"], OTHER["w"], 3), dtype=np.uint8), 300,
                               dither=True, tile_size=0, kmeans_niter=2, weights=ob.weights(n, 98))
    assert ok


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c.name for c in CONFIGS])
def test_result_independent_of_workspace_history(gpu, native, ws, cfg):
    late0 = gpu.patolette_amd_debug_late_growths()
    # (a) fresh: the call allocates every buffer itself
    _release(gpu)
    fresh = _single(gpu, native, cfg)
    # (b) stale: the same thread's engine right after a larger image with other K and options
    _other(gpu)
    stale = _single(gpu, native, cfg)
    d = _same(fresh, stale)
    assert not d, "%s: stale engine differs from a fresh one: %s" % (cfg, d)
    # (c) pooled: six engines, each on its first call, in flight together
    if cfg.entry != "device":
        _release(gpu)
        d = _same_batch(fresh, _batch(cfg))
        assert not d, "%s: batch on fresh pooled engines differs from a fresh single call: %s" % (cfg, d)
    # (d) as (a) and (c) with fresh memory poisoned: a read of memory nothing wrote turns into a NaN or a different decision
    ws(True)
    try:
        _release(gpu)
        poisoned = _single(gpu, native, cfg)
        d = _same(fresh, poisoned)
        assert not d, "%s: poisoned fresh workspace changes the result: %s" % (cfg, d)
        if cfg.entry != "device":
            _release(gpu)
            d = _same_batch(fresh, _batch(cfg))
            assert not d, "%s: batch on poisoned fresh engines differs: %s" % (cfg, d)
    finally:
        ws(False)
    assert gpu.patolette_amd_debug_late_growths() == late0, "%s: a workspace buffer was replaced while work was queued" % cfg


# one case per path anchored to the oracle (KMeans off: palettes to 1e-9, maps bit for bit)
@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c.entry == "host" and c.kmeans_niter == 0 and c.tile_size == 0],
                         ids=lambda c: c.name)
def test_fresh_result_matches_oracle(gpu, native, ob, ws, cfg):
    _release(gpu)
    got = _single(gpu, native, cfg)
    n = cfg.w * cfg.h
    flat = np.ascontiguousarray(cfg.img.T).reshape(-1)
    ec, pal_o, pmap_o = ob.patolette(cfg.w, cfg.h, flat, cfg.wts, cfg.K, dither=cfg.dither, color_space=cfg.color_space,
                                     kmeans_niter=0)
    assert ec == 0
    assert np.allclose(got["pal"], pal_o, rtol=0, atol=1e-9, equal_nan=True), np.nanmax(np.abs(got["pal"] - pal_o))
    assert int(np.sum(got["map"] != pmap_o.astype(np.int64))) == 0
    assert got["n_clusters"] <= cfg.K and n > 0


def test_device_loop_table_full_falls_back_to_host_loop(gpu, native, ob, ws):
    """patolette_amd_debug_fault(4): the device-driven loop reports its node table full after three rounds; the call starts over
    on the host-driven loop (quantize_clusters, rc == -2) over whatever the device loop left in the node table, and must still
    return the oracle's bits and the unfaulted call's."""
    cfg = Cfg("fallback", "host", 320, 240, 96, 21)
    _release(gpu)
    clean = _single(gpu, native, cfg)
    prev = gpu.patolette_amd_debug_fault(4)
    try:
        faulted = _single(gpu, native, cfg)
        _release(gpu)
        faulted_fresh = _single(gpu, native, cfg)
    finally:
        gpu.patolette_amd_debug_fault(prev)
    assert not _same(clean, faulted), _same(clean, faulted)
    assert not _same(clean, faulted_fresh), _same(clean, faulted_fresh)
    flat = np.ascontiguousarray(cfg.img.T).reshape(-1)
    ec, pal_o, pmap_o = ob.patolette(cfg.w, cfg.h, flat, None, cfg.K, dither=False, color_space=cfg.color_space, kmeans_niter=0)
    assert ec == 0
    assert np.allclose(faulted["pal"], pal_o, rtol=0, atol=1e-9), np.max(np.abs(faulted["pal"] - pal_o))
    assert int(np.sum(faulted["map"] != pmap_o.astype(np.int64))) == 0


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
def test_round6_geometry_batch_equals_separate_calls(gpu, native, ws, poison):
    """The geometry of the round-6 failure in one process: twelve 4096^2 images (patolette_amd_fill_image seeds 300 + i, as
    tests/dist_worker_nccl.py makes them), K = 256, 32 KMeans iterations, no weights, no dither, batched right after
    release_workspace (the first six images are pooled engines' first calls), against separate calls on this thread."""
    import patolette_amd as p
    w = h = 4096
    n, K, count = w * h, 256, 12
    ws(poison)
    try:
        d = gpu.patolette_amd_malloc(3 * n * 8)
        images = []
        try:
            for i in range(count):
                assert gpu.patolette_amd_fill_image(d, n, 300 + i) == 0
                flat = np.empty(3 * n)
                assert gpu.patolette_amd_memcpy_d2h(flat.ctypes.data_as(C.c_void_p), d, flat.nbytes) == 0
                images.append(flat.reshape(3, n).T)
        finally:
            gpu.patolette_amd_free(d)
        kw = dict(dither=False, tile_size=0, kmeans_niter=32)
        late0 = gpu.patolette_amd_debug_late_growths()
        _release(gpu)
        res = p.quantize_batch(w, h, images, K, **kw)
        _release(gpu)
        bad = []
        for i, r in enumerate(res):
            one = p.quantize(w, h, images[i], K, **kw)
            assert r[0] and one[0]
            if r[1].tobytes() != one[1].tobytes() or not np.array_equal(r[2], one[2]):
                bad.append("image %d: palette max diff %.3g, map mismatches %d" % (
                    i, np.nanmax(np.abs(r[1] - one[1])), int(np.sum(r[2] != one[2]))))
        assert not bad, bad
        assert gpu.patolette_amd_debug_late_growths() == late0
    finally:
        ws(False)
