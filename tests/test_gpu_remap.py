"""remap / patolette_amd_remap_u8 on the device against tests/remap_ref.py (the CPU oracle): every comparison is bit for bit.

Sizes: SMALL takes the wavefront layout of the dither, LANE (and the odd LANE_ODD) the lane layout once patolette_amd_dither_layout(1)
asks for it from 65 536 pixels on (palettes of 8 .. 256 rows).  Where the lane layout runs, a remap gathers the bytes along the curve
(k_dither_gather_u8), and from 2^22 pixels on the nearest map converts them inside its LDS-table kernel (k_nn_map_u8): no f64 image is
written.  patolette_amd_debug_remap_two_pass(1) forces the route every other case takes, and the two must agree bit for bit."""
import ctypes as C

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import remap_ref
from tests.util import scene

pytestmark = pytest.mark.gpu

SMALL, LANE, LANE_ODD = (40, 56), (256, 256), (263, 301)


@pytest.fixture(autouse=True)
def _lanes_from_64k(gpu):
    gpu.patolette_amd_dither_layout(1)
    yield
    gpu.patolette_amd_dither_layout(-1)
    gpu.patolette_amd_debug_remap_two_pass(0)
    _native.profile(False)


def _content(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "scene":
        return np.round(scene(h, w, seed) * 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "two":
        img = np.empty((h, w, 3), dtype=np.uint8)
        img[:] = (200, 30, 40)
        img[rng.random((h, w)) < 0.4] = (10, 120, 250)
        return img
    assert kind == "flat"
    img = np.empty((h, w, 3), dtype=np.uint8)
    img[:] = (90, 140, 33)
    return img


def _image(kind, size, frames, channels, seed=5):
    h, w = size
    fr = np.stack([_content(kind, h, w, seed + 7 * i) for i in range(frames)])
    if channels == 4:
        alpha = np.random.default_rng(seed).integers(0, 256, size=fr.shape[:-1] + (1,), dtype=np.uint8)
        fr = np.concatenate([fr, alpha], axis=-1)
    return fr if frames > 1 else fr[0]


def _palette(rows, seed=1):
    """`rows` distinct byte colours"""
    rng = np.random.default_rng(seed)
    codes = rng.choice(1 << 24, size=rows, replace=False)
    return np.stack([codes >> 16, (codes >> 8) & 255, codes & 255], axis=1).astype(np.uint8)


def _lane_layout(L, image, rows):
    shape = image.shape[:-1]
    n = shape[-1] * shape[-2]
    if image.ndim == 4 and shape[0] > 1:
        return n >= 64 and bool(L.patolette_amd_dither_layout_in_use(shape[0] * n, 1, rows))
    return bool(L.patolette_amd_dither_layout_in_use(shape[-1], shape[-2], rows))


def _used_rows(palette):
    return remap_ref.palette_rows(palette).shape[0]


def _check(L, ob, image, palette, dither):
    """remap == remap_ref; and where the fused kernel applies: it ran, the forced two-pass route did not run it, same bits."""
    m_ref, q_ref = remap_ref.remap(ob, image, palette, dither=dither)
    L.patolette_amd_debug_remap_two_pass(0)
    _native.profile(True)
    ok, m, q, msg = patolette_amd.remap(image, palette, dither=dither)
    names = set(_native.profile_results())
    _native.profile(False)
    assert ok, msg
    assert m.shape == m_ref.shape and q.shape == q_ref.shape and q.dtype == np.uint8
    rows = np.asarray(palette).shape[0]
    assert m.dtype == (np.uint8 if rows <= 256 else np.uint16 if rows <= 65536 else np.uint32)
    mism = int(np.sum(m.astype(np.int64) != m_ref))
    print("remap: dither %d rows %d shape %s: %d of %d differ from the reference; kernels %s" % (dither, rows, m.shape, mism, m.size, sorted(names)))
    assert mism == 0
    assert np.array_equal(q, q_ref)
    used = _used_rows(palette)
    if dither:
        fused, kernel, plain = _lane_layout(L, image, used), "k_dither_gather_u8", "k_dither_gather"
    else:                                                          # the LDS-table map kernel: 2^22 pixels and more, 8 .. 256 rows
        fused, kernel, plain = m.size >= (1 << 22) and 8 <= used <= 256, "k_nn_map_u8", "k_nn_map"
    assert (kernel in names) == fused
    if fused:
        assert "k_convert_u8" not in names and plain not in names
        L.patolette_amd_debug_remap_two_pass(1)
        _native.profile(True)
        ok2, m2, q2, _ = patolette_amd.remap(image, palette, dither=dither)
        names2 = set(_native.profile_results())
        _native.profile(False)
        L.patolette_amd_debug_remap_two_pass(0)
        assert ok2
        assert kernel not in names2 and "k_convert_u8" in names2 and plain in names2
        assert np.array_equal(m2, m) and np.array_equal(q2, q)
    else:
        assert "k_convert_u8" in names
    return m, q


@pytest.mark.parametrize("size", [SMALL, LANE_ODD], ids=["small", "lane-odd"])
@pytest.mark.parametrize("rows", [2, 7, 16, 256, 257, 1000])
@pytest.mark.parametrize("dither", [0, 1])
def test_rows_and_layouts(gpu, ob, dither, rows, size):
    image = _image("scene", size, 1, 3)
    if dither and 8 <= rows <= 256:
        assert _lane_layout(gpu, image, rows) == (size != SMALL)
    _check(gpu, ob, image, _palette(rows), dither)


def _dark_scene(h, w, channels):
    img = _image("scene", (h, w), 1, channels)
    img[..., :3] //= 4                                            # every pixel in the darkest 1/64 of the cube
    return img


@pytest.mark.parametrize("case", ["noise", "noise-rgba-u32", "dark-scene-bright-palette", "flat", "frames-odd"])
def test_large_nearest(gpu, ob, case):
    """4 Mi pixels and more: the nearest map runs around its LDS table, fused with the conversion by default.  Besides noise over the
    whole cube: a palette lying outside the pixels' bounding box, a degenerate box (one colour), 4-byte map elements (more than 256
    rows given, 256 used), frames whose pixel count is no multiple of the kernel's tile."""
    if case == "noise":
        image, pal = _image("noise", (2048, 2048), 1, 3), _palette(256, seed=3)
    elif case == "noise-rgba-u32":
        image = _image("noise", (2048, 2048), 1, 4)
        pal = np.full((300, 3), -1.0)
        pal[:256] = _palette(256, seed=4).astype(np.float64) / 255.0
    elif case == "dark-scene-bright-palette":
        image = _dark_scene(2048, 2048, 3)
        pal = (128 + _palette(64, seed=5) // 2).astype(np.uint8)  # every entry far outside the pixels' box
    elif case == "flat":
        image, pal = _image("flat", (2048, 2048), 1, 3), _palette(16, seed=6)
    else:
        image, pal = _image("scene", (1111, 1277), 3, 3), _palette(200, seed=7)
    m, _ = _check(gpu, ob, image, pal, 0)
    assert m.size >= 1 << 22


@pytest.mark.parametrize("size", [SMALL, LANE], ids=["small", "lane"])
@pytest.mark.parametrize("frames,channels", [(1, 3), (1, 4), (3, 3), (3, 4)])
@pytest.mark.parametrize("kind", ["scene", "noise", "two", "flat"])
@pytest.mark.parametrize("dither", [0, 1])
def test_content_channels_frames(gpu, ob, dither, kind, frames, channels, size):
    _check(gpu, ob, _image(kind, size, frames, channels), _palette(16, seed=2), dither)


@pytest.mark.parametrize("size", [SMALL, LANE_ODD], ids=["small", "lane-odd"])
@pytest.mark.parametrize("kind,K", [("scene", 24), ("two", 12), ("noise", 300)])
@pytest.mark.parametrize("dither", [0, 1])
def test_f64_palette_of_quantize_u8(gpu, ob, dither, kind, K, size):
    image = _image(kind, size, 1, 3)
    ok, pal8, _, _, pal, msg = patolette_amd.quantize_u8(image, K, dither=bool(dither), tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
    assert ok, msg
    assert pal.shape == (K, 3)
    if kind == "two":
        assert np.all(pal[-1] == -1.0)                             # fewer colours than K: trailing rows are the unused fill
    m, q = _check(gpu, ob, image, pal, dither)
    assert int(m.max()) < _used_rows(pal)
    assert np.array_equal(q, pal8[m])                              # pal8 of an f64 palette is that call's palette_u8
    _check(gpu, ob, image, np.ascontiguousarray(pal), dither)      # any layout of the float palette
    _check(gpu, ob, image, pal8, dither)


@pytest.mark.parametrize("size", [SMALL, LANE], ids=["small", "lane"])
@pytest.mark.parametrize("dither", [0, 1])
def test_idempotence(gpu, dither, size):
    image = _image("scene", size, 1, 3)
    ok, pal8, pmap, quant, _, msg = patolette_amd.quantize_u8(image, 32, dither=bool(dither), tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
    assert ok, msg
    distinct = len({tuple(r) for r in pal8}) == 32                 # then an index is defined by its colour and the map comes back too
    for d in (0, 1):
        ok, m, q, msg = patolette_amd.remap(quant, pal8, dither=bool(d))
        assert ok, msg
        assert np.array_equal(q, quant)
        assert not distinct or np.array_equal(m, pmap)


@pytest.mark.parametrize("size", [SMALL, LANE], ids=["small", "lane"])
@pytest.mark.parametrize("dither", [0, 1])
def test_streaming(gpu, ob, dither, size):
    frames = _image("scene", size, 5, 3)
    ok, pal8, _, _, _, msg = patolette_amd.quantize_frames(frames[:2], 48, dither=bool(dither), tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
    assert ok, msg
    m, q = _check(gpu, ob, frames[2:], pal8, dither)
    ok, m_all, q_all, msg = patolette_amd.remap(frames, pal8, dither=bool(dither))
    assert ok, msg
    assert np.array_equal(m_all[2:], m)
    for i in range(frames.shape[0]):
        ok, mi, qi, msg = patolette_amd.remap(frames[i], pal8, dither=bool(dither))
        assert ok, msg
        assert np.array_equal(m_all[i], mi) and np.array_equal(q_all[i], qi)


@pytest.mark.parametrize("frames", [1, 3])
def test_fused_dither_gives_the_image_up(gpu, ob, frames):
    """A lane walk that is told to give up at its first failing boundary (the test knobs of the dither): the remap converts the image
    after all and the wavefront layout walks it -- once, not the lane walk a second time.  Same map."""
    image, pal = _image("scene", LANE_ODD, frames, 3), _palette(16, seed=2)   # (a few per cent of a scene's run boundaries fail the first check)
    m_ref, q_ref = remap_ref.remap(ob, image, pal, dither=True)
    cap, passes = gpu.patolette_amd_debug_dither_solo_cap(0), gpu.patolette_amd_debug_dither_stall_passes(0)
    try:
        _native.profile(True)
        ok, m, q, msg = patolette_amd.remap(image, pal, dither=True)
        res = _native.profile_results()
        _native.profile(False)
    finally:
        gpu.patolette_amd_debug_dither_solo_cap(cap)
        gpu.patolette_amd_debug_dither_stall_passes(passes)
    assert ok, msg
    assert np.array_equal(m.astype(np.int64), m_ref) and np.array_equal(q, q_ref)
    assert res["k_dither_gather_u8"]["launches"] == 1 and "k_dither_gather" not in res      # one lane walk, given up ...
    assert res["k_convert_u8"]["launches"] == 1                                              # ... then the planes, for the wavefronts


def test_outputs_are_optional(gpu):
    image = _image("scene", SMALL, 1, 3)
    pal = _palette(16)
    ok, m, q, _ = patolette_amd.remap(image, pal, dither=True)
    ok2, m2, q2, _ = patolette_amd.remap(image, pal, dither=True, want_quantized=False)
    assert ok and ok2 and q2 is None and np.array_equal(m, m2)
    h, w = SMALL
    quant = np.zeros((h, w, 3), dtype=np.uint8)
    code = C.c_int(7)
    gpu.patolette_amd_remap_u8(1, w, h, image.ctypes.data_as(C.c_void_p), 3, None, pal.ctypes.data_as(C.c_void_p), 16, 1, None, 0,
                               quant.ctypes.data_as(C.c_void_p), C.byref(code))
    assert code.value == 0 and np.array_equal(quant, q)
    for eb, dt in ((2, np.uint16), (4, np.uint32), (8, np.uint64)):
        wide = np.zeros((h, w), dtype=dt)
        gpu.patolette_amd_remap_u8(1, w, h, image.ctypes.data_as(C.c_void_p), 3, None, pal.ctypes.data_as(C.c_void_p), 16, 1,
                                   wide.ctypes.data_as(C.c_void_p), eb, None, C.byref(code))
        assert code.value == 0 and np.array_equal(wide, m)
    st = patolette_amd.last_stats()
    assert st["ms_total"] > 0 and st["ms_map"] > 0 and st["dither_segments"] >= 1
    assert st["n_clusters"] == 0 and st["ms_kmeans"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0


def test_torch_flavour(gpu):
    """A torch CUDA tensor goes through patolette_amd_remap_u8_device: the numpy flavour's map, outputs on the input's device.  Own
    process: torch loads its HIP runtime before libpatolette_amd.so does."""
    import subprocess
    import sys
    from tests.util import ROOT
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
if not torch.cuda.is_available():
    print("TORCH-NO-DEVICE")
    sys.exit(0)
import patolette_amd as p
from patolette_amd import _native
from tests.test_gpu_remap import _image, _palette, SMALL, LANE
_native.lib().patolette_amd_dither_layout(1)
for image, rows in ((_image("scene", LANE, 3, 4), 16), (_image("noise", SMALL, 1, 3), 300)):
    pal = _palette(rows)
    for dither in (False, True):
        ok, m, q, msg = p.remap(image, pal, dither=dither)
        assert ok, msg
        t = torch.from_numpy(image).cuda()
        ok, mt, qt, msg = p.remap(t, pal, dither=dither)
        assert ok, msg
        assert mt.device == t.device and qt.device == t.device
        assert mt.dtype == (torch.uint8 if rows <= 256 else torch.int32) and tuple(mt.shape) == m.shape
        assert np.array_equal(mt.cpu().numpy().astype(np.int64), m.astype(np.int64))
        assert np.array_equal(qt.cpu().numpy(), q)
        ok, mt2, qt2, msg = p.remap(t, pal.astype(np.float64) / 255.0, dither=dither, want_quantized=False)
        assert ok and qt2 is None and np.array_equal(mt2.cpu().numpy(), mt.cpu().numpy())
print("TORCH-REMAP-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-REMAP-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_errors_and_recovery(gpu):
    h, w = SMALL
    image = _image("scene", SMALL, 1, 3)
    pal8 = _palette(16)
    palf = np.asfortranarray(pal8.astype(np.float64) / 255.0)
    pmap = np.zeros((h, w), dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    dp = lambda a: a.ctypes.data_as(_native.dp)   # noqa: E731

    def call(frames=1, width=w, height=h, channels=3, palette=None, palette_u8=None, rows=16, elem=1, dither=1):
        code = C.c_int(7)
        gpu.patolette_amd_remap_u8(frames, width, height, vp(image), channels, None if palette is None else dp(palette),
                                   None if palette_u8 is None else vp(palette_u8), rows, dither, vp(pmap), elem, None, C.byref(code))
        return code.value

    def good():
        assert call(palette_u8=pal8) == 0
        ok, m, _, msg = patolette_amd.remap(image, pal8)
        assert ok and np.array_equal(m, pmap), msg

    good()
    assert call(palette=np.full((16, 3), -1.0, order="F")) == -1
    assert "unused-row" in _native.last_error()
    good()
    bad = palf.copy(order="F")
    bad[3, 1] = np.nan
    assert call(palette=bad) == -1 and "finite" in _native.last_error()
    good()
    assert call(palette=palf, palette_u8=pal8) == -1 and "exactly one" in _native.last_error()
    assert call() == -1 and "exactly one" in _native.last_error()
    good()
    big = _palette(257)
    assert call(palette_u8=big, rows=257, elem=1) == -1
    assert call(palette_u8=pal8, elem=3) == -1
    assert call(palette_u8=pal8, channels=2) == -1
    assert call(palette_u8=pal8, rows=0) == -1
    assert call(palette_u8=pal8, width=0) == -2
    assert call(palette_u8=pal8, frames=0) == -2
    assert call(palette_u8=pal8, frames=1 << 31, dither=1) == -4 and "2^31" in _native.last_error()
    good()
    with pytest.raises(ValueError):
        patolette_amd.remap(image, np.full((4, 3), -1.0))
    good()


def test_workspace_history(gpu):
    image = _image("scene", LANE_ODD, 1, 3)
    other = _image("noise", (96, 80), 1, 3)
    pal = _palette(64)
    for dither in (False, True):
        for two_pass in (0, 1):
            gpu.patolette_amd_debug_remap_two_pass(two_pass)
            gpu.patolette_amd_release_workspace()
            ok, fresh, fresh_q, msg = patolette_amd.remap(image, pal, dither=dither)
            assert ok, msg
            gpu.patolette_amd_release_workspace()
            prev = gpu.patolette_amd_debug_workspace(1 | 2)
            try:
                before = gpu.patolette_amd_debug_late_growths()
                ok, *_ = patolette_amd.quantize_u8(other, 16, dither=dither, tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
                assert ok
                ok, m, q, msg = patolette_amd.remap(image, pal, dither=dither)
                assert ok, msg
                assert gpu.patolette_amd_debug_late_growths() == before
            finally:
                gpu.patolette_amd_debug_workspace(prev)
                gpu.patolette_amd_release_workspace()
            assert np.array_equal(m, fresh) and np.array_equal(q, fresh_q)
