"""quantize_rgba / patolette_amd_rgba: RGBA images with a transparent palette slot and an alpha-aware dither.

  * every pixel opaque (or alpha_threshold 0): bit for bit quantize_u8 of the RGB bytes, transparent_index -1;
  * some transparent: rows 1.. are the oracle's patolette() of the opaque pixels (row-scan order, their weights) with one colour
    less; the map is 0 on transparent pixels and 1 + the oracle's map elsewhere; quantized = palette_rgba[map];
  * dithered: the reference's Riemersma walk with transparent pixels skipped like out-of-image positions -- against the Python
    restatement (tests/rgba_ref.py) under both layouts, run cuts inside and next to transparent stretches, and at full size against
    the oracle's walk of a narrower image at the same Hilbert level;
  * saliency weights, workspace independence, errors."""
import ctypes as C

import numpy as np
import pytest

from tests import rgba_ref
from tests.util import scene

pytestmark = pytest.mark.gpu


def _rgba(h, w, seed, kind="noise"):
    rng = np.random.default_rng(seed)
    if kind == "scene":
        rgb = np.round(scene(h, w, seed) * 255).astype(np.uint8)
    else:
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    return np.concatenate([rgb, a], axis=2)


def _blobs(h, w, seed, frac=0.35):
    """A random-blob mask: True = transparent."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    while m.mean() < frac:
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(2, max(3, min(h, w) // 5))
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return m


def _masks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    border = (yy < 3) | (yy >= h - 3) | (xx < 4) | (xx >= w - 4)
    one_t = np.zeros((h, w), bool); one_t[h // 2, w // 3] = True
    one_o = np.ones((h, w), bool); one_o[h // 3, w // 2] = False
    return {"blobs": _blobs(h, w, 1), "checker": ((yy + xx) & 1) == 1, "border": border, "one_transparent": one_t,
            "one_opaque": one_o, "all_transparent": np.ones((h, w), bool)}


def _with_mask(img, transparent, thr=128):
    out = img.copy()
    out[..., 3] = np.where(transparent, thr - 1, 255)
    return out


def _check_consistent(ok, prgba, pmap, quant, tidx, n_opaque, n):
    assert ok
    assert np.array_equal(quant, prgba[pmap.astype(np.int64)])
    if n_opaque < n:
        assert tidx == 0 and tuple(prgba[0]) == (0, 0, 0, 0)
    else:
        assert tidx == -1


# ---- 1. no transparent pixel: quantize_u8 bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("dither", [False, True])
@pytest.mark.parametrize("cs", [0, 1, 2])
@pytest.mark.parametrize("tile", [0, 512])
def test_all_opaque_equals_u8(gpu, dither, cs, tile):
    import patolette_amd as p
    img = _rgba(60, 80, 7 + cs, "scene")
    for thr, im in ((128, _with_mask(img, np.zeros(img.shape[:2], bool))), (0, img)):
        kw = dict(dither=dither, color_space=cs, tile_size=tile, kmeans_niter=3, kmeans_max_samples=2048)
        ok, prgba, pmap, quant, pal, tidx, _ = p.quantize_rgba(im, 24, alpha_threshold=thr, **kw)
        ok8, pal8, pmap8, quant8, palf8, _ = p.quantize_u8(np.ascontiguousarray(im[..., :3]), 24, **kw)
        assert ok and ok8 and tidx == -1
        assert np.array_equal(pal, palf8) and np.array_equal(pmap, pmap8)
        assert np.array_equal(quant[..., :3], quant8) and np.all(quant[..., 3] == 255)
        used = pal[:, 0] != -1
        assert np.array_equal(prgba[:, :3], pal8) and np.all(prgba[used, 3] == 255) and np.all(prgba[~used] == 0)


def test_torch_tensor_equals_numpy(gpu):
    """A torch CUDA tensor goes through patolette_amd_rgba_device: the numpy path's results, map and image left in HBM -- all
    opaque and masked, dither on and off.  Own process: torch loads its HIP runtime before libpatolette_amd.so does."""
    import subprocess
    import sys
    from tests.util import ROOT
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
assert torch.cuda.is_available()
import patolette_amd as p
from tests.test_gpu_rgba import _rgba, _blobs, _with_mask
img = _rgba(50, 70, 3, "scene")
for tr in (np.zeros((50, 70), bool), _blobs(50, 70, 3, 0.3)):
    im = _with_mask(img, tr)
    for dither in (False, True):
        for K in (16, 300):
            ref = p.quantize_rgba(im, K, dither=dither, tile_size=512, kmeans_niter=2)
            got = p.quantize_rgba(torch.from_numpy(im).cuda(), K, dither=dither, tile_size=512, kmeans_niter=2)
            assert ref[0] and got[0] and got[2].is_cuda and got[3].is_cuda
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[4], ref[4]) and got[5] == ref[5]
            assert np.array_equal(got[2].cpu().numpy().astype(np.int64), ref[2].astype(np.int64))
            assert np.array_equal(got[3].cpu().numpy(), ref[3])
print("TORCH-RGBA-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "TORCH-RGBA-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 2. masked, no dither, against the oracle -------------------------------------------------------------------------------
def _oracle_masked(ob, img, transparent, K, weights, niter, cs=2, dither=False):
    opaque = ~transparent.reshape(-1)
    rows = img[..., :3].reshape(-1, 3)[opaque].astype(np.float64) / 255
    m = rows.shape[0]
    w = None if weights is None else np.ascontiguousarray(weights.reshape(-1)[opaque])
    ec, pal, pmap = ob.patolette(m, 1, ob.planar(rows), w, K - 1, dither=dither, color_space=cs, kmeans_niter=niter,
                                 kmeans_max_samples=1024)
    assert ec == 0
    return pal, pmap


@pytest.mark.parametrize("mask", ["blobs", "checker", "border", "one_transparent", "one_opaque", "all_transparent"])
@pytest.mark.parametrize("K", [2, 16, 256, 300])
def test_masked_nodither_matches_oracle(gpu, ob, mask, K):
    import patolette_amd as p
    h, w = 48, 64
    img = _rgba(h, w, 11 + K, "scene")
    tr = _masks(h, w)[mask]
    im = _with_mask(img, tr)
    niter = 0 if K in (2, 256) else 3
    wts = np.random.default_rng(K).random(h * w) + 0.5 if K in (16, 256) else None
    ok, prgba, pmap, quant, pal, tidx, msg = p.quantize_rgba(im, K, dither=False, tile_size=0, kmeans_niter=niter,
                                                             kmeans_max_samples=1024, weights=wts)
    n_op = int((~tr).sum())
    _check_consistent(ok, prgba, pmap, quant, tidx, n_op, h * w)
    assert pal.shape == (K, 3) and np.all(pal[0] == 0)
    flat_map = pmap.reshape(-1).astype(np.int64)
    assert np.all(flat_map[tr.reshape(-1)] == 0)
    if n_op == 0:
        assert np.all(pal[1:] == -1) and np.all(prgba == 0)
        return
    pal_o, pmap_o = _oracle_masked(ob, im, tr, K, wts, niter)
    np.testing.assert_allclose(pal[1:], pal_o, rtol=0, atol=1e-9)
    assert np.array_equal(flat_map[~tr.reshape(-1)], pmap_o.astype(np.int64) + 1)
    assert np.all(quant.reshape(-1, 4)[~tr.reshape(-1), 3] == 255)


def test_threshold_edges(gpu, ob):
    import patolette_amd as p
    h, w, K, thr = 40, 56, 12, 77
    img = _rgba(h, w, 5, "scene")
    tr = _blobs(h, w, 9)
    im = img.copy()
    im[..., 3] = np.where(tr, thr - 1, thr)                          # alpha thr - 1 is transparent, alpha thr opaque
    ok, prgba, pmap, quant, pal, tidx, _ = p.quantize_rgba(im, K, alpha_threshold=thr, dither=False, tile_size=0, kmeans_niter=0)
    _check_consistent(ok, prgba, pmap, quant, tidx, int((~tr).sum()), h * w)
    pal_o, pmap_o = _oracle_masked(ob, im, tr, K, None, 0)
    np.testing.assert_allclose(pal[1:], pal_o, rtol=0, atol=1e-9)
    assert np.array_equal(pmap.reshape(-1)[~tr.reshape(-1)].astype(np.int64), pmap_o.astype(np.int64) + 1)
    # 256: everything transparent; 0: nothing
    ok, prgba, pmap, _, pal, tidx, _ = p.quantize_rgba(im, K, alpha_threshold=256, dither=False, tile_size=0, kmeans_niter=0)
    assert ok and tidx == 0 and np.all(pmap == 0) and np.all(pal[1:] == -1)
    ok, _, _, _, _, tidx, _ = p.quantize_rgba(im, K, alpha_threshold=0, dither=False, tile_size=0, kmeans_niter=0)
    assert ok and tidx == -1


# ---- 3. masked dither against the restatement, both layouts ------------------------------------------------------------------
def _rec2020_rows(ob, im, cs):
    n = im.shape[0] * im.shape[1]
    flat = ob.planar(im[..., :3].reshape(-1, 3).astype(np.float64) / 255)
    if cs == 2:
        flat = ob.convert("ictcp_to_rec2020", ob.convert("srgb_to_ictcp", flat))
    elif cs == 1:
        flat = ob.convert("cieluv_to_rec2020", ob.convert("srgb_to_cieluv", flat))
    else:
        flat = ob.convert("srgb_to_rec2020", flat)
    return flat.reshape(3, n).T.copy()


def _map_palette(gpu, K):
    buf = np.zeros(3 * K)
    n = gpu.patolette_amd_last_map_palette(buf.ctypes.data_as(C.POINTER(C.c_double)), K)
    return buf.reshape(3, K)[:, :n].T.copy()


@pytest.fixture
def knobs(gpu):
    yield gpu
    gpu.patolette_amd_dither_config(0, -1)
    gpu.patolette_amd_dither_layout(-1)
    gpu.patolette_amd_debug_dither_stall_passes(-1)


def _dither_case(gpu, ob, im, tr, K, cs, layouts_cfgs):
    import patolette_amd as p
    h, w = tr.shape
    want = None
    for layout, segs, warm, stall in layouts_cfgs:
        gpu.patolette_amd_dither_layout(layout)
        gpu.patolette_amd_dither_config(segs, warm)
        gpu.patolette_amd_debug_dither_stall_passes(stall)
        ok, prgba, pmap, quant, pal, tidx, _ = p.quantize_rgba(im, K, dither=True, color_space=cs, tile_size=0, kmeans_niter=0)
        _check_consistent(ok, prgba, pmap, quant, tidx, int((~tr).sum()), h * w)
        flat_map = pmap.reshape(-1).astype(np.int64)
        assert np.all(flat_map[tr.reshape(-1)] == 0)
        if want is None:
            pal2020 = _map_palette(gpu, K)
            ref = rgba_ref.masked_dither(ob, _rec2020_rows(ob, im, cs), w, h, pal2020, ~tr.reshape(-1))
            want = np.where(tr.reshape(-1), 0, ref + 1)
        bad = int(np.sum(flat_map != want))
        assert bad == 0, (layout, segs, warm, bad)
        st = p.last_stats()
        assert st["dither_segments"] >= 1


@pytest.mark.parametrize("K", [4, 16, 256, 300])
def test_masked_dither_wavefronts(knobs, ob, K):
    h, w = 80, 96
    img = _rgba(h, w, 21 + K, "scene")
    tr = _blobs(h, w, 4, 0.3)
    tr[10:14, :] = True                                              # long transparent stretches across the curve
    img[40:70, 10:60, :3] = (200, 37, 90)                            # flat content off the palette: walk-through repairs
    im = _with_mask(img, tr)
    cfgs = [(0, 0, -1, -1), (0, 7, 40, -1), (0, 23, 16, -1), (0, 1, -1, -1)]
    _dither_case(knobs, ob, im, tr, K, 2, cfgs)


@pytest.mark.parametrize("K", [16, 256])
def test_masked_dither_lanes(knobs, ob, K):
    h, w = 256, 320                                                  # M >= 65 536 opaque pixels: the lane layout can be forced
    img = _rgba(h, w, 31 + K, "scene")
    tr = _blobs(h, w, 8, 0.1)
    img[100:180, 50:200, :3] = (13, 200, 140)                        # flat, off the palette: stalls, solo passes
    im = _with_mask(img, tr)
    assert (~tr).sum() >= 65536
    cfgs = [(1, 0, -1, -1), (1, 600, 24, -1), (1, 301, 64, 0), (0, 0, -1, -1)]
    _dither_case(knobs, ob, im, tr, K, 1 if K == 16 else 2, cfgs)
    knobs.patolette_amd_dither_layout(1)
    knobs.patolette_amd_dither_config(0, -1)
    assert knobs.patolette_amd_dither_layout_in_use(int((~tr).sum()), 1, K - 1) == 1


# ---- 4. full size: the lane layout by default, against the oracle's walk of the narrow image ------------------------------
def test_masked_dither_full_size(knobs, ob):
    import patolette_amd as p
    h, w, wn, K = 2304, 4096, 3700, 64
    assert rgba_ref.hilbert_level(w, h) == rgba_ref.hilbert_level(wn, h) and wn * h >= 1 << 23
    img = _rgba(h, w, 2, "scene")
    tr = np.zeros((h, w), bool)
    tr[:, wn:] = True
    im = _with_mask(img, tr)
    ok, prgba, pmap, quant, pal, tidx, _ = p.quantize_rgba(im, K, dither=True, tile_size=0, kmeans_niter=0)
    _check_consistent(ok, prgba, pmap, quant, tidx, wn * h, w * h)
    assert knobs.patolette_amd_dither_layout_in_use(wn * h, 1, K - 1) == 1
    pal2020 = _map_palette(knobs, K)
    narrow = np.ascontiguousarray(im[:, :wn, :])
    flat = _rec2020_rows(ob, narrow, 2)
    want = ob.dither(ob.planar(flat), wn, h, pal2020).astype(np.int64) + 1
    got = pmap[:, :wn].reshape(-1).astype(np.int64)
    assert int(np.sum(got != want)) == 0
    assert np.all(pmap[:, wn:] == 0)
    # a random-blob mask: both layouts are exact, so they agree
    tr2 = _blobs(h // 4, w // 4, 3, 0.2).repeat(4, axis=0).repeat(4, axis=1)
    im2 = _with_mask(img, tr2)
    maps = []
    for layout in (1, 0):
        knobs.patolette_amd_dither_layout(layout)
        ok, _, pm, _, _, _, _ = p.quantize_rgba(im2, K, dither=True, tile_size=0, kmeans_niter=0, want_quantized=False)
        assert ok
        maps.append(pm)
    assert np.array_equal(maps[0], maps[1])


# ---- 5. saliency ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dither", [False, True])
def test_saliency_weights_of_full_image(gpu, dither):
    import patolette_amd as p
    h, w = 90, 120
    img = _rgba(h, w, 17, "scene")
    im = _with_mask(img, _blobs(h, w, 2, 0.25))
    ok, prgba, pmap, quant, pal, _, _ = p.quantize_rgba(im, 20, dither=dither, tile_size=512, kmeans_niter=2)
    sw = p.saliency_weights(w, h, im[..., :3].reshape(-1, 3).astype(np.float64) / 255, 512)
    ok2, prgba2, pmap2, quant2, pal2, _, _ = p.quantize_rgba(im, 20, dither=dither, tile_size=0, weights=sw, kmeans_niter=2)
    assert ok and ok2
    assert np.array_equal(pal, pal2) and np.array_equal(pmap, pmap2) and np.array_equal(quant, quant2)


# ---- 6. workspace --------------------------------------------------------------------------------------------------------
def test_workspace_history_does_not_matter(gpu):
    import patolette_amd as p
    prev = gpu.patolette_amd_debug_workspace(3)
    try:
        a = _with_mask(_rgba(120, 150, 4, "scene"), _blobs(120, 150, 6, 0.3))
        b = _with_mask(_rgba(70, 64, 5, "scene"), _blobs(70, 64, 7, 0.2))
        calls = [dict(dither=True, tile_size=512, kmeans_niter=3), dict(dither=False, tile_size=0, kmeans_niter=3,
                                                                         color_space=1, weights=np.linspace(1, 2, 150 * 120))]
        gpu.patolette_amd_release_workspace()
        late0 = gpu.patolette_amd_debug_late_growths()
        fresh = [p.quantize_rgba(a, 40, **kw) for kw in calls]
        p.quantize_rgba(b, 300, dither=True, tile_size=0, kmeans_niter=0)
        pooled = [p.quantize_rgba(a, 40, **kw) for kw in calls]
        assert gpu.patolette_amd_debug_late_growths() == late0
        for x, y in zip(fresh, pooled):
            assert x[0] and y[0]
            for i in (1, 2, 3, 4):
                assert np.array_equal(x[i], y[i])
    finally:
        gpu.patolette_amd_debug_workspace(prev)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    import patolette_amd as p
    img = _with_mask(_rgba(20, 30, 1), _blobs(20, 30, 1, 0.3))
    ok, *_, msg = p.quantize_rgba(img, 1, dither=False, tile_size=0)
    assert not ok and msg == "Palette size should be greater than 0."
    solid = img.copy(); solid[..., 3] = 255
    ok, prgba, pmap, _, _, tidx, _ = p.quantize_rgba(solid, 1, dither=False, tile_size=0)    # one colour, nothing transparent
    assert ok and tidx == -1 and np.all(pmap == 0)
    with pytest.raises(ValueError):
        p.quantize_rgba(img[..., :3], 8)
    with pytest.raises(ValueError):
        p.quantize_rgba(img, 8, alpha_threshold=257)
    with pytest.raises(ValueError):
        p.quantize_rgba(img, 8, alpha_threshold=-1)
    ok, prgba, pmap, quant, pal, tidx, _ = p.quantize_rgba(img, 8, palette_only=True, tile_size=0)
    assert ok and pmap is None and quant is None and tidx == 0 and np.all(pal[0] == 0)
    code = C.c_int(0)
    from patolette_amd import _native
    opts = _native.QuantizationOptions(False, False, 2, 0, 0, False)
    gpu.patolette_amd_rgba(30, 20, img.ctypes.data_as(C.c_void_p), 300, None, 0.0, 8, C.byref(opts), None, None, None, 1, None,
                           None, C.byref(code))
    assert code.value == -1 and "alpha_threshold" in _native.last_error()
