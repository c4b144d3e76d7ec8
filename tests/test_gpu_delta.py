"""frame_deltas / patolette_amd_frame_deltas on the device against tests/delta_ref.py (numpy on the CPU oracle).

Every comparison with the reference is bit for bit over all elements of deltas, shown, rects and changed, none excluded.  The device's
pow is within 0.52 ulp of glibc's, not equal to it, so a lossy comparison means something only away from the threshold: every lossy
case first asserts that the REFERENCE's smallest relative gap |D - tol^2| / tol^2 over every distance it evaluated is at least 1e-9
-- the bar of test_gpu_ordered.py, for the same reason.  If another input trips it, change the seed, not the bar.

The input maps are the reference's own nearest and ordered maps of the clip, made on the CPU: no other device stage is involved.
Sizes: (40, 56); (37, 53), whose 1961 pixels are no multiple of 64; (263, 301), no multiple of the block and with rows that wrap
inside a wavefront; (1, 70) and (65, 1) for the geometry of one-pixel-wide rectangles.  Where the pixel count is a multiple of 4 a lane
owns four positions and moves them as one vector: (40, 56), and (36, 301) with an odd width and eleven blocks; the other sizes take
the one-position kernel.  (36, 301) on the CPU oracle: the smallest gap is 4.79e-5 (16 rows, nearest, 0.02) and both outcomes occur
from 16 rows on."""
import ctypes as C
import functools

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import delta_ref
from tests.test_gpu_remap import _image, _palette
from tests.util import ROOT

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-9
SIZES = {"small": ((40, 56), 5), "odd64": ((37, 53), 4), "wrap": ((263, 301), 6), "quad": ((36, 301), 4)}
PREFIX = "patolette_amd_frame_deltas:"


@pytest.fixture(autouse=True)
def _defaults_again(gpu):
    yield
    _native.profile(False)
    gpu.patolette_amd_debug_delta_quad(-1)


def _dtype(rows):
    return np.uint8 if rows <= 256 else np.uint16


@functools.lru_cache(maxsize=None)
def _clip(size, F):
    frames = delta_ref.clip(size[0], size[1], F)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _maps(size, F, rows, kind):
    """(the palette, the reference's maps of the clip in the numpy flavour's element type), computed once."""
    from oracle import binding as ob
    pal = _palette(rows, seed=2)
    maps = delta_ref.maps_of(ob, _clip(size, F), pal, kind).astype(_dtype(rows))
    pal.setflags(write=False)
    maps.setflags(write=False)
    return pal, maps


@functools.lru_cache(maxsize=None)
def _reference(size, F, rows, kind, tolerance, T=None):
    """The reference's (deltas, shown, rects, changed, tested, kept) for _maps(...), computed once; the gap condition is asserted here."""
    from oracle import binding as ob
    pal, maps = _maps(size, F, rows, kind)
    d, s, r, c, gap, tested, kept = delta_ref.frame_deltas(ob, maps, pal, T=T, frames=_clip(size, F), tolerance=tolerance)
    print("delta reference: %s F %d rows %d %s tolerance %g: %d distances, %d kept, smallest relative gap %.3g"
          % (size, F, rows, kind, tolerance, tested, kept, gap))
    if tolerance > 0:
        assert gap >= MIN_GAP
    for a in (d, s, r, c):
        a.setflags(write=False)
    return d, s, r, c, tested, kept


def _same(got, ref):
    """got: (deltas, rects, changed, shown) of the device; ref: _reference's tuple."""
    d, r, c, s = got
    d_ref, s_ref, r_ref, c_ref = ref[:4]
    wrong = [int(np.sum(np.asarray(a).astype(np.int64) != b)) for a, b in ((d, d_ref), (s, s_ref), (r, r_ref), (c, c_ref))]
    print("deltas / shown / rects / changed: %s of %s differ from the reference" % (wrong, [d_ref.size, s_ref.size, r_ref.size, c_ref.size]))
    assert d.shape == d_ref.shape and s.shape == s_ref.shape and r.shape == r_ref.shape and c.shape == c_ref.shape
    assert wrong == [0, 0, 0, 0]
    assert r.dtype == np.int32 and c.dtype == np.int64


@pytest.mark.parametrize("tolerance", [0.0, 0.02, 0.05])
@pytest.mark.parametrize("kind", ["nearest", "ordered"])
@pytest.mark.parametrize("rows", [2, 16, 255, 300])
@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_rows_and_tolerances(gpu, name, rows, kind, tolerance):
    size, F = SIZES[name]
    pal, maps = _maps(size, F, rows, kind)
    ref = _reference(size, F, rows, kind, tolerance)
    if tolerance > 0 and rows >= 16:
        assert 0 < ref[5] < ref[4]                                    # both outcomes occur
    for quad in (-1, 1) if size[0] * size[1] % 4 == 0 else (-1,):     # small frames take one position per lane unless told otherwise
        gpu.patolette_amd_debug_delta_quad(quad)
        ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, pal, frames=_clip(size, F), tolerance=tolerance, want_shown=True)
        assert ok, msg
        assert d.dtype == maps.dtype and s.dtype == maps.dtype
        _same((d, r, c, s), ref)
        assert np.array_equal(delta_ref.replay(d, rows), s)
    if tolerance == 0:
        assert np.array_equal(s, maps)
    if rows == 255:
        assert maps.dtype == np.uint8 and np.any(d == 255)            # the last free index of a byte


@pytest.mark.parametrize("size", [(1, 70), (65, 1)])
def test_one_pixel_wide(gpu, size):
    """Geometry only (the exact mode): three different scenes one pixel wide, so that most of the line changes from frame to frame."""
    from oracle import binding as ob
    maps = delta_ref.maps_of(ob, _image("scene", size, 3, 3), _palette(16, seed=2), "nearest").astype(np.uint8)
    ref = delta_ref.frame_deltas(ob, maps, 16)
    ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, 16, want_shown=True)
    assert ok, msg
    _same((d, r, c, s), ref)
    thin, long = (3, 2) if size[0] == 1 else (2, 3)
    assert np.all(c[1:] > 8) and np.all(r[:, thin] == 1) and np.all(r[1:, long] > 8)


@pytest.mark.parametrize("size", [(1024, 2048), (1024, 2044)])
def test_where_lanes_take_four_positions(gpu, size):
    """2^21 pixels: where the launcher's own rule moves to four positions per lane on an MI355X, and a size just below.  The exact
    mode on random maps (it reads no colours), against the reference; forced either way the results are the same."""
    rng = np.random.default_rng(3)
    first = rng.integers(0, 16, size=size, dtype=np.uint8)
    maps = np.stack([first, np.where(rng.random(size) < 0.1, rng.integers(0, 16, size=size, dtype=np.uint8), first), first])
    maps[2, 5:9, 7] = 15 - maps[1, 5:9, 7]
    ref = delta_ref.frame_deltas(None, maps, 16)
    for quad in (-1, 0, 1):
        gpu.patolette_amd_debug_delta_quad(quad)
        ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, 16, want_shown=True)
        assert ok, msg
        _same((d, r, c, s), ref)


def test_one_frame_an_unchanged_frame_and_an_explicit_index(gpu):
    from oracle import binding as ob
    size, F = SIZES["odd64"]
    pal, maps = _maps(size, F, 16, "ordered")
    ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps[:1], pal, want_shown=True)
    assert ok, msg
    assert np.array_equal(d, maps[:1]) and np.array_equal(s, maps[:1])
    assert r.tolist() == [[0, 0, size[1], size[0]]] and c.tolist() == [size[0] * size[1]]
    twice = np.concatenate([maps[:2], maps[1:2], maps[2:]])
    frames = np.concatenate([_clip(size, F)[:2], _clip(size, F)[1:2], _clip(size, F)[2:]])
    for tolerance in (0.0, 0.05):
        ref = delta_ref.frame_deltas(ob, twice, pal, T=255, frames=frames, tolerance=tolerance)
        assert tolerance == 0 or ref[4] >= MIN_GAP
        ok, d, r, c, s, msg = patolette_amd.frame_deltas(twice, pal, transparent_index=255, frames=frames, tolerance=tolerance, want_shown=True)
        assert ok, msg
        _same((d, r, c, s), ref)
        assert r[2].tolist() == [0, 0, 0, 0] and c[2] == 0 and np.all(d[2] == 255)
        assert np.array_equal(delta_ref.replay(d, 255), s)
    ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, pal)
    assert ok and s is None, msg
    assert np.array_equal(d, _reference(size, F, 16, "ordered", 0.0)[0])


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c_call(gpu, maps, elem, rows, T, frames=None, channels=3, palette=None, palette_u8=None, tolerance=0.0, delta=None, shown=None, rects=None,
            changed=None, dims=None):
    F, h, w = dims if dims is not None else maps.shape
    code = C.c_int(7)
    gpu.patolette_amd_frame_deltas(F, w, h, _vp(maps), elem, rows, T, _vp(frames), channels,
                                   None if palette is None else palette.ctypes.data_as(_native.dp), _vp(palette_u8), tolerance, _vp(delta),
                                   _vp(shown), None if rects is None else rects.ctypes.data_as(C.POINTER(C.c_int32)),
                                   None if changed is None else changed.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(code))
    return code.value


def test_elements_aliasing_and_outputs_through_the_c_entry(gpu):
    size, F = SIZES["small"]
    pal, maps = _maps(size, F, 16, "ordered")
    frames = _clip(size, F)
    for tolerance in (0.0, 0.05):
        kw = dict(frames=frames, palette_u8=pal, tolerance=tolerance) if tolerance else {}
        for eb, dt, T in ((1, np.uint8, 16), (2, np.uint16, 65535), (4, np.uint32, 2 ** 32 - 1), (8, np.uint64, 2 ** 40 + 3)):
            ref = _reference(size, F, 16, "ordered", tolerance)
            m = maps.astype(dt)
            d, s = np.zeros_like(m), np.zeros_like(m)
            r, c = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.uint64)
            assert _c_call(gpu, m, eb, 16, T, delta=d, shown=s, rects=r, changed=c, **kw) == 0
            d_ref = np.where(ref[0] == 16, T, ref[0]).astype(dt)      # the reference's deltas with this T
            assert np.array_equal(d, d_ref) and np.array_equal(s, ref[1].astype(dt))
            assert np.array_equal(r, ref[2]) and np.array_equal(c.astype(np.int64), ref[3])
            # delta_maps aliasing palette_maps
            inout = m.copy()
            assert _c_call(gpu, inout, eb, 16, T, delta=inout, **kw) == 0
            assert np.array_equal(inout, d_ref)
        # every output NULL but one
        ref = _reference(size, F, 16, "ordered", tolerance)
        d, s = np.zeros_like(maps), np.zeros_like(maps)
        r, c = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.uint64)
        assert _c_call(gpu, maps, 1, 16, 16, delta=d, **kw) == 0 and np.array_equal(d, ref[0])
        assert _c_call(gpu, maps, 1, 16, 16, shown=s, **kw) == 0 and np.array_equal(s, ref[1])
        assert _c_call(gpu, maps, 1, 16, 16, rects=r, **kw) == 0 and np.array_equal(r, ref[2])
        assert _c_call(gpu, maps, 1, 16, 16, changed=c, **kw) == 0 and np.array_equal(c.astype(np.int64), ref[3])
        assert _c_call(gpu, maps, 1, 16, 16, **kw) == 0


def test_palette_forms(gpu):
    from oracle import binding as ob
    size, F = SIZES["small"]
    pal, maps = _maps(size, F, 16, "nearest")
    frames = _clip(size, F)
    ref = _reference(size, F, 16, "nearest", 0.05)
    palf = pal.astype(np.float64) / 255.0
    for form in (pal, np.ascontiguousarray(palf), np.asfortranarray(palf)):
        ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, form, frames=frames, tolerance=0.05, want_shown=True)
        assert ok, msg
        _same((d, r, c, s), ref)
    filled = np.full((20, 3), -1.0)                                   # trailing unused rows: dropped; the default index is the row count as given
    filled[:16] = palf
    ref20 = delta_ref.frame_deltas(ob, maps, filled, frames=frames, tolerance=0.05)
    assert ref20[4] >= MIN_GAP and np.array_equal(ref20[1], ref[1]) and np.any(ref20[0] == 20)
    for form in (filled, np.asfortranarray(filled)):
        ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, form, frames=frames, tolerance=0.05, want_shown=True)
        assert ok, msg
        _same((d, r, c, s), ref20)
    rgba = np.concatenate([frames, np.full(frames.shape[:3] + (1,), 7, dtype=np.uint8)], axis=-1)     # a 4th byte is ignored
    ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, pal, frames=rgba, tolerance=0.05, want_shown=True)
    assert ok, msg
    _same((d, r, c, s), ref)


def test_errors_and_recovery(gpu):
    size, F = SIZES["small"]
    h, w = size
    pal, maps = _maps(size, F, 16, "ordered")
    frames = _clip(size, F)
    palf = np.asfortranarray(pal.astype(np.float64) / 255.0)
    ref = _reference(size, F, 16, "ordered", 0.05)
    d = np.zeros_like(maps)
    r = np.zeros((F, 4), dtype=np.int32)

    def lossy(m=maps, **kw):
        args = dict(frames=frames, palette_u8=pal, tolerance=0.05, delta=d, rects=r)
        args.update(kw)
        return _c_call(gpu, m, args.pop("elem", 1), args.pop("rows", 16), args.pop("T", 16), **args)

    def good():
        d[:] = 99
        r[:] = -1
        assert lossy() == 0
        assert np.array_equal(d, ref[0]) and np.array_equal(r, ref[2])

    def failed(code, *words):
        assert code == -1
        text = _native.last_error()
        assert text.startswith(PREFIX) and all(word in text for word in words), text
        good()

    good()
    # an element that is no row: the kernel's flag, in both modes
    bad = maps.copy()
    bad[3, 17, 5] = 16
    failed(lossy(m=bad), "palette_rows")
    failed(_c_call(gpu, bad, 1, 16, 16, delta=d), "palette_rows")
    bad = maps.copy()
    bad[0, 0, 0] = 200                                                # ... on the canvas from the first frame on
    failed(lossy(m=bad), "palette_rows")
    filled = np.full((20, 3), -1.0, order="F")                        # ... and one that names a dropped row
    filled[:16] = palf
    bad = maps.copy()
    bad[2, 39, 55] = 17
    failed(lossy(m=bad, palette_u8=None, palette=filled, rows=20, T=20), "dropped")
    with pytest.raises(ValueError, match="palette_rows"):
        patolette_amd.frame_deltas(bad, pal[:16], frames=frames, tolerance=0.05)
    good()
    # -1: the arguments
    failed(lossy(elem=3), "map_elem_bytes")
    failed(lossy(elem=0), "map_elem_bytes")
    failed(lossy(channels=2), "channels")
    failed(lossy(channels=5), "channels")
    failed(lossy(T=15), "transparent_index")
    failed(lossy(T=256), "one row less")                              # not representable in a byte
    failed(_c_call(gpu, maps, 1, 256, 256, delta=d), "one row less")  # 256 rows leave a byte no free index
    failed(_c_call(gpu, maps.astype(np.uint16), 2, 16, 65536, delta=d), "one row less")
    for tolerance in (-0.01, float("nan"), float("inf"), -float("inf")):
        failed(lossy(tolerance=tolerance), "tolerance")
    failed(lossy(palette=palf), "exactly one")
    failed(lossy(palette_u8=None), "exactly one")
    failed(lossy(frames=None), "pixels")
    failed(lossy(rows=0), "palette_rows")
    nan = palf.copy(order="F")
    nan[3, 1] = np.nan
    failed(lossy(palette_u8=None, palette=nan), "finite")
    failed(lossy(palette_u8=None, palette=np.full((16, 3), -1.0, order="F")), "unused-row")
    code = C.c_int(7)
    gpu.patolette_amd_frame_deltas(F, w, h, None, 1, 16, 16, None, 3, None, None, 0.0, _vp(d), None, None, None, C.byref(code))
    failed(code.value, "no maps")
    assert lossy(tolerance=-0.0) == 0                                 # -0.0 is not negative: the exact mode
    # -2 and -4
    assert lossy(dims=(0, h, w)) == -2
    assert lossy(dims=(F, 0, w)) == -2
    assert lossy(dims=(F, h, 0)) == -2
    good()
    assert lossy(dims=(1 << 31, h, w)) == -4 and _native.last_error().startswith(PREFIX) and "too big" in _native.last_error()
    assert lossy(dims=(1, 50000, 50000)) == -4
    good()
    ok, *rest, msg = patolette_amd.frame_deltas(np.zeros((2, 0, 5), dtype=np.uint8), 16)
    assert not ok and rest == [None] * 4 and msg == "Image dimensions should be greater than 0."


def test_last_stats(gpu):
    size, F = SIZES["small"]
    pal, maps = _maps(size, F, 16, "ordered")
    for tolerance in (0.0, 0.05):
        ok, *_ = patolette_amd.frame_deltas(maps, pal, frames=_clip(size, F), tolerance=tolerance, want_shown=True)
        assert ok
        st = patolette_amd.last_stats()
        assert st["ms_total"] > 0 and st["ms_map"] > 0 and st["ms_upload"] > 0 and st["ms_download"] > 0
        assert st["ms_total"] >= st["ms_map"]
        assert all(st[key] == 0 for key in st if not key.startswith("ms_"))
        assert st["ms_convert"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0 and st["ms_kmeans"] == 0 and st["ms_saliency"] == 0


def test_one_kernel(gpu):
    size, F = SIZES["wrap"]
    pal, maps = _maps(size, F, 255, "nearest")
    for tolerance in (0.0, 0.02):
        _native.profile(True)
        ok, *_ = patolette_amd.frame_deltas(maps, pal, frames=_clip(size, F), tolerance=tolerance)
        prof = _native.profile_results()
        _native.profile(False)
        assert ok
        assert prof["k_frame_deltas"]["launches"] == 1
        assert not set(prof) & {"k_convert_u8", "k_convert", "k_nn_map", "k_nn_map_u8", "k_ordered_map", "k_dither"}


def test_workspace_history(gpu):
    size, F = SIZES["wrap"]
    pal, maps = _maps(size, F, 300, "nearest")
    frames = _clip(size, F)
    other = _image("noise", (96, 80), 1, 3)
    small_pal, small_maps = _maps(SIZES["small"][0], SIZES["small"][1], 16, "ordered")

    def run():
        ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, pal, frames=frames, tolerance=0.02, want_shown=True)
        assert ok, msg
        return d, r, c, s

    gpu.patolette_amd_release_workspace()
    fresh = run()
    _same(fresh, _reference(size, F, 300, "nearest", 0.02))
    gpu.patolette_amd_release_workspace()
    prev = gpu.patolette_amd_debug_workspace(1 | 2)
    try:
        before = gpu.patolette_amd_debug_late_growths()
        ok, *_ = patolette_amd.quantize_u8(other, 16, dither=True, tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
        assert ok
        ok, *_ = patolette_amd.frame_deltas(small_maps, small_pal, frames=_clip(*SIZES["small"]), tolerance=0.05, want_shown=True)
        assert ok
        first = run()
        ok, *_ = patolette_amd.remap(other, small_pal, dither="ordered")
        assert ok
        second = run()
        assert gpu.patolette_amd_debug_late_growths() == before
    finally:
        gpu.patolette_amd_debug_workspace(prev)
        gpu.patolette_amd_release_workspace()
    for got in (first, second):
        assert all(np.array_equal(a, b) for a, b in zip(got, fresh))


def test_torch_flavour(gpu):
    """Torch CUDA tensors go through patolette_amd_frame_deltas_device: the numpy flavour's results, deltas and shown on the maps'
    device.  Own process: torch loads its HIP runtime before libpatolette_amd.so does."""
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
from oracle import binding as ob
from tests import delta_ref
from tests.test_gpu_remap import _palette
for size, F, rows in (((263, 301), 6, 16), ((37, 53), 4, 300), ((40, 56), 5, 255), ((36, 301), 4, 300)):
    frames, pal = delta_ref.clip(size[0], size[1], F), _palette(rows, seed=2)
    maps = delta_ref.maps_of(ob, frames, pal, "nearest")
    m_np = maps.astype(np.uint8 if rows <= 256 else np.uint16)
    m_t = torch.from_numpy(maps.astype(np.uint8 if rows <= 256 else np.int32)).cuda()
    f_t = torch.from_numpy(frames).cuda()
    for tol in (0.0, 0.05):
        p._native.lib().patolette_amd_debug_delta_quad(-1)
        ok, d, r, c, s, msg = p.frame_deltas(m_np, pal, frames=frames, tolerance=tol, want_shown=True)
        assert ok, msg
        p._native.lib().patolette_amd_debug_delta_quad(1)           # four positions per lane where the tensors allow it
        ok, dt, rt, ct, st, msg = p.frame_deltas(m_t, pal, frames=f_t, tolerance=tol, want_shown=True)
        assert ok, msg
        assert dt.device == m_t.device and st.device == m_t.device and dt.dtype == m_t.dtype and tuple(dt.shape) == d.shape
        assert isinstance(rt, np.ndarray) and isinstance(ct, np.ndarray)
        assert np.array_equal(dt.cpu().numpy().astype(np.int64), d.astype(np.int64))
        assert np.array_equal(st.cpu().numpy().astype(np.int64), s.astype(np.int64))
        assert np.array_equal(rt, r) and np.array_equal(ct, c)
    ok, dt2, rt2, ct2, none, msg = p.frame_deltas(m_t, rows)
    assert ok and none is None, msg
    ok, d0, r0, c0, _, msg = p.frame_deltas(m_np, rows)
    assert ok and np.array_equal(dt2.cpu().numpy().astype(np.int64), d0.astype(np.int64)) and np.array_equal(rt2, r0)
    try:
        p.frame_deltas(m_t, pal, frames=frames, tolerance=0.05)
        raise SystemExit("host frames with device maps were accepted")
    except ValueError:
        pass
print("TORCH-DELTA-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-DELTA-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_composition(gpu):
    """The pipeline the entry is for: quantize_frames(..., 255, dither="ordered") -> frame_deltas with the frames and a tolerance."""
    from oracle import binding as ob
    size, F = SIZES["small"]
    frames = _clip(size, F)
    ok, pal8, maps, _, pal, msg = patolette_amd.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2,
                                                                kmeans_max_samples=4096, want_quantized=False)
    assert ok, msg
    assert maps.dtype == np.uint8
    ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, pal8, frames=frames, tolerance=0.05, want_shown=True)
    assert ok, msg
    assert np.array_equal(delta_ref.replay(d, 255), s)                # replaying the deltas equals shown
    ref = delta_ref.frame_deltas(ob, maps, pal8, frames=frames, tolerance=0.05)
    print("composition: %d distances, %d kept, smallest relative gap %.3g; changed %s" % (ref[5], ref[6], ref[4], c.tolist()))
    if ref[4] >= MIN_GAP:
        _same((d, r, c, s), ref)
    # pal8[shown] is within the guarantee: the frame's own choice, or within the tolerance of the frame's source pixel -- up to what
    # the device's pow may move a distance by (0.52 ulp per pow: far below 1e-9 relative)
    dist2 = delta_ref.distances2(ob, frames, pal8, s)
    assert np.all((s == maps) | (dist2 <= 0.05 * 0.05 * (1 + 1e-9)))
    assert np.any((s != maps))                                        # the lossy mode held something
    assert np.all(c[1:] < c[0]) and pal8[s].shape == frames.shape
