"""remap(dither="ordered") / patolette_amd_remap_ordered_u8 on the device against tests/ordered_ref.py (numpy on the CPU oracle).

Every comparison with the reference is bit for bit over all pixels, none excluded.  The device's pow is within 0.52 ulp of glibc's,
not equal to it, so such a comparison means something only away from exact ties: every case first asserts that the REFERENCE's
smallest relative gap (d2 - d1) / d2 between the best and the second-best row is at least 1e-9 -- seven orders above what an ulp in
a pow moves a distance by.  If another seed trips that condition, change the seed, not the bar.

Sizes: (40, 56) and (263, 301) -- width no multiple of the 8x8 tile, pixel count no multiple of the block; rows up to
kOrderedChunk + 5, where the palette passes through LDS in two chunks and the winner of some pixels lies in the second."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import ordered_ref, remap_ref
from tests.test_gpu_remap import LANE_ODD, SMALL, _image, _palette
from tests.util import ROOT, scene

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-9

with open(os.path.join(ROOT, "patolette_amd", "csrc", "ordered.h")) as _fh:
    CHUNK = int(re.search(r"constexpr int kOrderedChunk = (\d+);", _fh.read()).group(1))


@pytest.fixture(autouse=True)
def _profile_off(gpu):
    yield
    _native.profile(False)


@functools.lru_cache(maxsize=None)
def _case(kind, size, frames, channels, rows, seed=1):
    image, pal = _image(kind, size, frames, channels), _palette(rows, seed=seed)
    image.setflags(write=False)
    pal.setflags(write=False)
    return image, pal


@functools.lru_cache(maxsize=None)
def _reference(kind, size, frames, channels, rows, spread, seed=1):
    """(map, quantized) of the reference for _case(...), computed once; the gap condition is asserted here."""
    from oracle import binding as ob
    image, pal = _case(kind, size, frames, channels, rows, seed)
    m, q, gap = ordered_ref.remap(ob, image, pal, spread)
    print("ordered reference: %s %s frames %d rows %d spread %.6g: smallest relative gap %.3g" % (kind, size, frames, rows, spread, gap))
    assert gap >= MIN_GAP
    m.setflags(write=False)
    q.setflags(write=False)
    return m, q


def _same(m, q, m_ref, q_ref):
    mism = int(np.sum(np.asarray(m).astype(np.int64) != m_ref))
    print("ordered: %d of %d differ from the reference" % (mism, m_ref.size))
    assert m.shape == m_ref.shape and mism == 0
    assert np.array_equal(q, q_ref)


@pytest.mark.parametrize("size", [SMALL, LANE_ODD], ids=["small", "odd"])
@pytest.mark.parametrize("kind", ["scene", "noise"])
@pytest.mark.parametrize("rows", [1, 2, 7, 16, 256, 257, 1000, CHUNK + 5])
def test_rows_and_sizes(gpu, rows, kind, size):
    image, pal = _case(kind, size, 1, 3, rows)
    spread = patolette_amd.ordered_spread(pal)
    m_ref, q_ref = _reference(kind, size, 1, 3, rows, spread)
    _native.profile(True)
    ok, m, q, msg = patolette_amd.remap(image, pal, dither="ordered")
    names = set(_native.profile_results())
    _native.profile(False)
    assert ok, msg
    assert m.dtype == (np.uint8 if rows <= 256 else np.uint16) and q.dtype == np.uint8
    _same(m, q, m_ref, q_ref)
    assert "k_ordered_map" in names
    assert not names & {"k_convert_u8", "k_nn_map", "k_nn_map_u8"}
    if rows > CHUNK:
        assert np.any(m_ref >= CHUNK) and np.any(m_ref < CHUNK)     # winners in both chunks
    if rows > 1:
        assert spread > 0 and len(np.unique(m_ref)) > 1


@pytest.mark.parametrize("channels", [3, 4])
def test_frames_restart_the_pattern(gpu, channels):
    size = (37, 53)                                                   # 37 * 53 = 1961 is no multiple of 64: a stack-relative origin shows
    frames, pal = _case("scene", size, 3, channels, 16, 2)
    spread = patolette_amd.ordered_spread(pal)
    m_ref, q_ref = _reference("scene", size, 3, channels, 16, spread, 2)
    ok, m, q, msg = patolette_amd.remap(frames, pal, dither="ordered")
    assert ok, msg
    _same(m, q, m_ref, q_ref)
    for i in range(3):
        ok, mi, qi, msg = patolette_amd.remap(frames[i], pal, dither="ordered")
        assert ok, msg
        assert np.array_equal(m[i], mi) and np.array_equal(q[i], qi)


@pytest.mark.parametrize("kind", ["scene", "noise"])
def test_spread(gpu, kind):
    image, pal = _case(kind, LANE_ODD, 1, 3, 16, 2)
    ok, m0, q0, msg = patolette_amd.remap(image, pal, dither="ordered", spread=0)
    assert ok, msg
    ok, m_nn, q_nn, msg = patolette_amd.remap(image, pal, dither=False)
    assert ok, msg
    assert np.array_equal(m0, m_nn) and np.array_equal(q0, q_nn)    # spread 0 is the nearest map, bit for bit
    m_ref, q_ref = _reference(kind, LANE_ODD, 1, 3, 16, 4.0, 2)      # +-2 at the tile's ends: both clamps
    v = ordered_ref.shifted(image, 4.0)
    assert np.any(v == 0.0) and np.any(v == 1.0) and np.any((v > 0.0) & (v < 1.0))
    ok, m4, q4, msg = patolette_amd.remap(image, pal, dither="ordered", spread=4.0)
    assert ok, msg
    _same(m4, q4, m_ref, q_ref)
    ok, md, qd, msg = patolette_amd.remap(image, pal, dither="ordered")
    ok2, ms, qs, msg2 = patolette_amd.remap(image, pal, dither="ordered", spread=patolette_amd.ordered_spread(pal))
    assert ok and ok2, msg + msg2
    assert np.array_equal(md, ms) and np.array_equal(qd, qs)
    assert np.any(md != m0)


def test_palette_forms(gpu):
    image, pal = _case("scene", SMALL, 1, 3, 16, 2)
    spread = 0.2
    m_ref, q_ref = _reference("scene", SMALL, 1, 3, 16, spread, 2)
    palf = pal.astype(np.float64) / 255.0
    filled = np.full((20, 3), -1.0)
    filled[:16] = palf
    for form in (pal, np.ascontiguousarray(palf), np.asfortranarray(palf), filled, np.asfortranarray(filled)):
        ok, m, q, msg = patolette_amd.remap(image, form, dither="ordered", spread=spread)
        assert ok, msg
        _same(m, q, m_ref, q_ref)
    # a duplicated row: an exact tie, which the lowest index wins -- the map is that of the palette without the copy
    for at in (3, 15):
        dup = np.concatenate([pal, pal[at:at + 1]])
        ok, m, q, msg = patolette_amd.remap(image, dup, dither="ordered", spread=spread)
        assert ok, msg
        assert np.any(m_ref == at) and not np.any(m == 16)
        _same(m, q, m_ref, q_ref)
    n = len(pal)
    got = np.zeros((n, 3), order="F")
    assert gpu.patolette_amd_last_map_palette(got.ctypes.data_as(_native.dp), n) == n + 1      # (the last call's: with the copy)
    from oracle import binding as ob
    want = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(palf)), n)
    big = np.zeros((n + 1, 3), order="F")
    assert gpu.patolette_amd_last_map_palette(big.ctypes.data_as(_native.dp), n + 1) == n + 1
    assert np.allclose(big[:n], want, rtol=1e-12, atol=1e-15)         # the palette in ICtCp (host pow against glibc's: an ulp or two)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_elements_and_outputs(gpu):
    h, w = SMALL
    image, pal = _case("scene", SMALL, 1, 3, 16, 2)
    spread = 0.2
    m_ref, q_ref = _reference("scene", SMALL, 1, 3, 16, spread, 2)
    code = C.c_int(7)
    for eb, dt in ((1, np.uint8), (2, np.uint16), (4, np.uint32), (8, np.uint64)):
        pmap = np.zeros((h, w), dtype=dt)
        quant = np.zeros((h, w, 3), dtype=np.uint8)
        gpu.patolette_amd_remap_ordered_u8(1, w, h, _vp(image), 3, None, _vp(pal), 16, spread, _vp(pmap), eb, _vp(quant), C.byref(code))
        assert code.value == 0
        _same(pmap, quant, m_ref, q_ref)
    st = patolette_amd.last_stats()
    assert st["ms_total"] > 0 and st["ms_map"] > 0
    assert all(st[key] == 0 for key in st if key.startswith("dither_"))
    assert st["n_clusters"] == 0 and st["ms_kmeans"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0
    quant = np.zeros((h, w, 3), dtype=np.uint8)
    gpu.patolette_amd_remap_ordered_u8(1, w, h, _vp(image), 3, None, _vp(pal), 16, spread, None, 0, _vp(quant), C.byref(code))
    assert code.value == 0 and np.array_equal(quant, q_ref)           # a NULL map with `quantized` only
    ok, m, q, msg = patolette_amd.remap(image, pal, dither="ordered", spread=spread, want_quantized=False)
    assert ok and q is None, msg
    assert np.array_equal(m, m_ref)
    wide = _palette(300)                                              # 4-byte elements on the device, uint16 in numpy
    spread300 = patolette_amd.ordered_spread(wide)
    image_n, _ = _case("noise", SMALL, 1, 3, 16, 2)
    from oracle import binding as ob
    m300, q300, gap = ordered_ref.remap(ob, image_n, wide, spread300)
    assert gap >= MIN_GAP
    ok, m, q, msg = patolette_amd.remap(image_n, wide, dither="ordered")
    assert ok and m.dtype == np.uint16, msg
    _same(m, q, m300, q300)


def test_errors_and_recovery(gpu):
    h, w = SMALL
    image, pal8 = _case("scene", SMALL, 1, 3, 16, 2)
    palf = np.asfortranarray(pal8.astype(np.float64) / 255.0)
    pmap = np.zeros((h, w), dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(_native.dp)   # noqa: E731

    def call(frames=1, width=w, height=h, channels=3, palette=None, palette_u8=None, rows=16, elem=1, spread=0.2):
        code = C.c_int(7)
        gpu.patolette_amd_remap_ordered_u8(frames, width, height, _vp(image), channels, None if palette is None else dp(palette),
                                           _vp(palette_u8), rows, spread, _vp(pmap), elem, None, C.byref(code))
        return code.value

    assert call(palette_u8=pal8) == 0
    first = pmap.copy()
    assert len(np.unique(first)) > 1

    def good():
        pmap[:] = 255
        assert call(palette_u8=pal8) == 0
        assert np.array_equal(pmap, first)

    for spread in (float("nan"), float("inf"), -0.25, -0.0 - 1e-300):
        assert call(palette_u8=pal8, spread=spread) == -1
        assert _native.last_error().startswith("patolette_amd_remap:") and "spread" in _native.last_error()
        good()
    assert call(palette_u8=pal8, spread=-0.0) == 0                    # -0.0 is not negative
    assert call(palette=palf, palette_u8=pal8) == -1 and "exactly one" in _native.last_error()
    assert call() == -1 and "exactly one" in _native.last_error()
    good()
    bad = palf.copy(order="F")
    bad[3, 1] = np.nan
    assert call(palette=bad) == -1 and "finite" in _native.last_error()
    assert call(palette=np.full((16, 3), -1.0, order="F")) == -1 and "unused-row" in _native.last_error()
    good()
    assert call(palette_u8=_palette(257), rows=257, elem=1) == -1
    assert call(palette_u8=pal8, elem=3) == -1
    assert call(palette_u8=pal8, channels=2) == -1
    assert call(palette_u8=pal8, channels=5) == -1
    assert call(palette_u8=pal8, rows=0) == -1
    assert call(palette_u8=pal8, width=0) == -2
    assert call(palette_u8=pal8, frames=0) == -2
    assert call(palette_u8=pal8, frames=1 << 31) == -4 and "too big" in _native.last_error()   # the nearest remap's cap and text
    good()
    with pytest.raises(ValueError):
        patolette_amd.remap(image, np.full((4, 3), -1.0), dither="ordered")
    with pytest.raises(ValueError):
        patolette_amd.remap(image, pal8, dither="ordered", spread=-1.0)
    good()


def test_workspace_history(gpu):
    image, pal = _case("scene", LANE_ODD, 1, 3, 64)
    other = _image("noise", (96, 80), 1, 3)
    gpu.patolette_amd_release_workspace()
    ok, fresh, fresh_q, msg = patolette_amd.remap(image, pal, dither="ordered")
    assert ok, msg
    gpu.patolette_amd_release_workspace()
    prev = gpu.patolette_amd_debug_workspace(1 | 2)
    try:
        before = gpu.patolette_amd_debug_late_growths()
        ok, *_ = patolette_amd.quantize_u8(other, 16, dither=True, tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
        assert ok
        ok, m, q, msg = patolette_amd.remap(image, pal, dither="ordered")
        assert ok, msg
        ok, *_ = patolette_amd.remap(other, pal, dither=True)
        assert ok
        ok, m2, q2, msg = patolette_amd.remap(image, pal, dither="ordered")
        assert ok, msg
        assert gpu.patolette_amd_debug_late_growths() == before
    finally:
        gpu.patolette_amd_debug_workspace(prev)
        gpu.patolette_amd_release_workspace()
    assert np.array_equal(m, fresh) and np.array_equal(q, fresh_q)
    assert np.array_equal(m2, fresh) and np.array_equal(q2, fresh_q)


def test_torch_flavour(gpu):
    """A torch CUDA tensor goes through patolette_amd_remap_ordered_u8_device: the numpy flavour's map, outputs on the input's device.
    Own process: torch loads its HIP runtime before libpatolette_amd.so does."""
    import subprocess
    import sys
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
if not torch.cuda.is_available():
    print("TORCH-NO-DEVICE")
    sys.exit(0)
import patolette_amd as p
from tests.test_gpu_remap import _image, _palette, SMALL, LANE_ODD
for image, rows in ((_image("scene", LANE_ODD, 3, 4), 16), (_image("noise", SMALL, 1, 3), 300)):
    pal = _palette(rows)
    ok, m, q, msg = p.remap(image, pal, dither="ordered")
    assert ok, msg
    t = torch.from_numpy(image).cuda()
    ok, mt, qt, msg = p.remap(t, pal, dither="ordered")
    assert ok, msg
    assert mt.device == t.device and qt.device == t.device
    assert mt.dtype == (torch.uint8 if rows <= 256 else torch.int32) and tuple(mt.shape) == m.shape
    assert np.array_equal(mt.cpu().numpy().astype(np.int64), m.astype(np.int64))
    assert np.array_equal(qt.cpu().numpy(), q)
    ok, mt2, qt2, msg = p.remap(t, pal.astype(np.float64) / 255.0, dither="ordered", want_quantized=False)
    assert ok and qt2 is None and np.array_equal(mt2.cpu().numpy(), mt.cpu().numpy())
    ok, mt0, _, msg = p.remap(t, pal, dither="ordered", spread=0.0)
    ok2, mn, _, msg2 = p.remap(t, pal, dither=False)
    assert ok and ok2 and np.array_equal(mt0.cpu().numpy(), mn.cpu().numpy())
print("TORCH-ORDERED-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-ORDERED-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_composition(gpu):
    """quantize_frames / quantize_u8 with dither="ordered" are two calls: the palette of the same call with dither=False, then the
    ordered remap onto that f64 palette.  The palette is the one the FULL dither=False call returns, in sRGB.  The palette_only call's
    is not that: as in the reference (patolette.c:267-325 converts the palette back to sRGB inside `if (!palette_only)`) it stays in the
    quantisation's colour space, ICtCp by default, and a remap would read its rows as sRGB colours -- so it is not the recipe here,
    and the last lines pin the difference down."""
    kw = dict(tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
    frames = _image("scene", SMALL, 3, 3)
    _native.profile(True)
    ok, pal8, maps, quant, pal, msg = patolette_amd.quantize_frames(frames, 32, dither="ordered", **kw)
    names = set(_native.profile_results())
    _native.profile(False)
    assert ok, msg
    assert "k_ordered_map" in names and not names & {"k_nn_map", "k_nn_map_u8", "k_dither"}     # the palette call maps nothing
    ok, p8, _, _, p64, msg = patolette_amd.quantize_frames(frames, 32, dither=False, **kw)
    assert ok, msg
    ok, m2, q2, msg = patolette_amd.remap(frames, p64, dither="ordered")
    assert ok, msg
    assert np.array_equal(pal, p64) and np.array_equal(pal8, p8)
    assert np.array_equal(pal8, remap_ref.pal8(pal))                  # palette_u8 is the clip-and-truncate of the f64 palette
    assert maps.shape == (3,) + SMALL and maps.dtype == np.uint8 and quant.shape == (3,) + SMALL + (3,)
    assert np.array_equal(maps, m2) and np.array_equal(quant, q2)
    assert np.array_equal(pal8[maps], quant)
    assert len(np.unique(maps)) > 8
    image = frames[1]
    for space in (patolette_amd.ColorSpace_ICtCp, patolette_amd.ColorSpace_CIELuv, patolette_amd.ColorSpace_sRGB):
        ok, pal8, pmap, quant, pal, msg = patolette_amd.quantize_u8(image, 32, dither="ordered", spread=0.1, color_space=space, **kw)
        assert ok, msg
        ok, p8, _, _, p64, msg = patolette_amd.quantize_u8(image, 32, dither=False, color_space=space, **kw)
        assert ok, msg
        ok, m2, q2, msg = patolette_amd.remap(image, p64, dither="ordered", spread=0.1)
        assert ok, msg
        assert np.array_equal(pal, p64) and np.array_equal(pal8, p8)
        assert np.array_equal(pmap, m2) and np.array_equal(quant, q2) and np.array_equal(pal8[pmap], quant)
        # the quantized image is close to the image: the palette's rows were taken as the sRGB colours they are
        rmse = float(np.sqrt(np.mean((quant.astype(np.float64) - image[..., :3]) ** 2)))
        print("colour space %d: RMSE of the ordered quantized image %.2f code values" % (space, rmse))
        # (a palette read in the wrong space: beyond 100 on this scene, 14 .. 16 with the right one; colour space sRGB is left out:
        # there the reference's dither=False palette has been through ICtCp -> sRGB without ever being ICtCp, patolette.c:322-323)
        assert rmse < 40.0 or space == patolette_amd.ColorSpace_sRGB
    ok, p8o, m_none, q_none, p64o, msg = patolette_amd.quantize_u8(image, 32, dither="ordered", palette_only=True, **kw)
    ok2, _, _, _, p64po, msg2 = patolette_amd.quantize_u8(image, 32, dither=False, palette_only=True, **kw)
    assert ok and ok2 and m_none is None and q_none is None and np.array_equal(p64o, p64po), msg + msg2
    ok, _, _, _, p64i, msg = patolette_amd.quantize_u8(image, 32, dither=False, **kw)
    assert ok and not np.allclose(p64po, p64i, atol=0.02)            # palette_only: ICtCp rows, not the sRGB palette
    ok, _, m_no_q, q_no, _, msg = patolette_amd.quantize_u8(image, 32, dither="ordered", spread=0.1, want_quantized=False, **kw)
    ok2, _, pmap, _, _, msg2 = patolette_amd.quantize_u8(image, 32, dither="ordered", spread=0.1, **kw)
    assert ok and ok2 and q_no is None and np.array_equal(m_no_q, pmap), msg + msg2


def test_purpose_frames_that_barely_differ_get_maps_that_barely_differ(gpu):
    """What the mode is for: two frames one code value apart.  The Riemersma walk re-rolls the frame behind the first changed choice;
    the ordered map changes only where a pixel sits near a boundary."""
    rng = np.random.default_rng(11)
    a = np.round(scene(64, 64, 5) * 255).astype(np.int64)
    b = np.clip(a + rng.integers(-1, 2, size=a.shape), 0, 255)
    frames = np.stack([a, b]).astype(np.uint8)
    pal = _palette(16, seed=2)
    share = {}
    for dither in ("ordered", True):
        ok, m, _, msg = patolette_amd.remap(frames, pal, dither=dither)
        assert ok, msg
        share[dither] = float(np.mean(m[0] != m[1]))
    print("share of the map that changes between two frames one code value apart: ordered %.4f, Riemersma %.4f" % (share["ordered"], share[True]))
    assert share["ordered"] < share[True]
