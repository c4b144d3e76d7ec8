"""measure / patolette_amd_measure on the device against tests/measure_ref.py (numpy on the CPU oracle).

Every integer output -- count, sse and max_se per palette row and per frame -- is compared bit for bit with the reference, none
excluded.  The two ICtCp figures are compared to relative 1e-9, the bar the project holds its palettes to: the device's pow is within
0.52 ulp of libm's, not equal to it, and d_sum is a sum in the kernel's own (fixed) order.  On the CPU oracle the reference's nearest
and ordered maps of the cases below give d_max between 5.8e-5 and 1.2e-2 and d_sum between 1.9e-3 and 325 per frame (the random and
the one-row maps more), and another summation order (numpy's pairwise, ascending, descending) moves the d_sum of 79 163 positions by
about 1e-14 relative, so the bar has about five orders of margin; every such case first asserts that its reference d_sum is at least
1e-3 and its d_max at least 1e-6, so that a relative bar means something.

Shapes (frames of delta_ref.clip): (40, 56) x 1 -- 2240 positions, one full tile of 2048 and a part; (37, 53) x 3 -- 1961 positions,
no multiple of 64, frames start inside a wavefront; (263, 301) x 2 -- 39 tiles per frame, so the fold over tiles and the slots;
(1, 1) x 1; (301, 1) x 2.  Palettes: random bytes with 1, 2, 16, 255, 256, 300 and 1029 rows (the last beyond the LDS chunk), as
bytes, as f64 and as f64 with two trailing -1 rows.  Maps: the reference's nearest and ordered maps, a uniformly random one (rows
with count 0 occur) and one with every position on one row (every atomic lands on one cell)."""
import ctypes as C
import functools

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import delta_ref, measure_ref
from tests.test_gpu_remap import _image, _palette
from tests.util import ROOT

pytestmark = pytest.mark.gpu

REL = 1e-9
SHAPES = {"tile": ((40, 56), 1), "odd64": ((37, 53), 3), "tiles": ((263, 301), 2), "one": ((1, 1), 1), "thin": ((301, 1), 2)}
ROWS = [1, 2, 16, 255, 256, 300, 1029]
KINDS = ["nearest", "ordered", "random", "one_row"]
PREFIX = "patolette_amd_measure:"


@pytest.fixture(autouse=True)
def _defaults_again(gpu):
    yield
    _native.profile(False)


def _dtype(rows):
    return np.uint8 if rows <= 256 else np.uint16


@functools.lru_cache(maxsize=None)
def _clip(size, F):
    frames = delta_ref.clip(size[0], size[1], F)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _maps(size, F, rows, kind):
    """(the byte palette, a map of the clip in the numpy flavour's element type), computed once."""
    from oracle import binding as ob
    pal = _palette(rows, seed=2)
    if kind in ("nearest", "ordered"):
        maps = delta_ref.maps_of(ob, _clip(size, F), pal, kind)
    elif kind == "random":
        maps = np.random.default_rng(rows).integers(0, rows, size=(F,) + size)
    else:
        maps = np.full((F,) + size, rows - 1)
    maps = maps.astype(_dtype(rows))
    pal.setflags(write=False)
    maps.setflags(write=False)
    return pal, maps


@functools.lru_cache(maxsize=None)
def _reference(size, F, rows, kind, skip=None):
    """The reference's (entries, per_frame, ictcp) for _maps(...) on the byte palette, computed once and left unchanged."""
    from oracle import binding as ob
    pal, maps = _maps(size, F, rows, kind)
    out = measure_ref.measure(ob, _clip(size, F), maps, pal, skip_index=skip)
    for a in out:
        a.setflags(write=False)
    return out


def _meaningful(dist_ref):
    """The condition under which the relative bar is applied."""
    print("reference d_sum %s d_max %s" % (dist_ref[:, 0].tolist(), dist_ref[:, 1].tolist()))
    assert np.all(dist_ref[:, 0] >= 1e-3) and np.all(dist_ref[:, 1] >= 1e-6)


def _same(got, ref, integers_only=False):
    """got: (entries, per_frame, ictcp) of the device; ref: the reference's.  Integers bit for bit, the ICtCp figures to REL."""
    ent, per, dist = got
    ent_ref, per_ref, dist_ref = ref
    assert ent.dtype == np.int64 and per.dtype == np.int64 and ent.shape == ent_ref.shape and per.shape == per_ref.shape
    wrong = [int(np.sum(ent != ent_ref)), int(np.sum(per != per_ref))]
    print("entries / per_frame: %s of %s values differ from the reference" % (wrong, [ent_ref.size, per_ref.size]))
    assert wrong == [0, 0]
    if integers_only:
        return
    assert dist.dtype == np.float64 and dist.shape == dist_ref.shape
    rel = np.abs(dist - dist_ref) / dist_ref
    print("d_sum / d_max: largest relative difference %.3g / %.3g" % (rel[:, 0].max(), rel[:, 1].max()))
    assert np.all(rel <= REL)


def _measure(*args, **kw):
    ok, ent, per, dist, msg = patolette_amd.measure(*args, **kw)
    assert ok, msg
    return ent, per, dist


def _kinds(name, rows):
    """The maps of a case.  A single position on its nearest entry of 16 or more random rows has D between 1.4e-5 and 6.7e-4 on the CPU
    oracle, below the d_sum the relative bar is stated for: (1, 1) takes the reference's own maps with 1 and 2 rows only, the random
    map and the one-row map with all.  The reference's ordered map of 158 326 positions on 1029 rows takes the CPU six seconds and
    tells nothing the nearest one does not: left out."""
    if name == "one" and rows >= 16:
        return ["random", "one_row"]
    if name == "tiles" and rows == 1029:
        return ["nearest", "random", "one_row"]
    return KINDS


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_rows_and_maps(gpu, name, rows):
    size, F = SHAPES[name]
    for kind in _kinds(name, rows):
        pal, maps = _maps(size, F, rows, kind)
        ref = _reference(size, F, rows, kind)
        _meaningful(ref[2])
        got = _measure(_clip(size, F), maps, pal)
        _same(got, ref)
        assert got[0][:, 0].sum() == F * size[0] * size[1]
        if kind == "random" and rows == 1029 and name != "tiles":
            assert np.any(got[0][:, 0] == 0)                          # rows that nothing names (fewer positions than three times the rows)
        only = _measure(_clip(size, F), maps, pal, ictcp=False)       # the same integers without the ICtCp part
        assert only[2] is None
        _same(only, ref, integers_only=True)


def test_palette_forms(gpu):
    from oracle import binding as ob
    size, F = SHAPES["odd64"]
    for rows in (16, 1029):
        pal, maps = _maps(size, F, rows, "nearest")
        ref = _reference(size, F, rows, "nearest")
        _meaningful(ref[2])
        palf = pal.astype(np.float64) / 255.0
        for form in (np.ascontiguousarray(palf), np.asfortranarray(palf)):
            _same(_measure(_clip(size, F), maps, form), ref)          # v / 255.0 * 255.0 truncates back to v for every byte v
        filled = np.full((rows + 2, 3), -1.0)                         # two trailing unused rows: dropped, but rows of the result
        filled[:rows] = palf * 0.97 + 0.004                           # (rows whose bytes are not the byte palette's)
        ref2 = measure_ref.measure(ob, _clip(size, F), maps, filled)
        _meaningful(ref2[2])
        assert ref2[0].shape == (rows + 2, 3) and not np.array_equal(ref2[1], ref[1])
        got = _measure(_clip(size, F), maps, filled)
        _same(got, ref2)
        assert not got[0][rows:].any()


def test_width_of_the_accumulators(gpu):
    """79 163 positions at the largest error there is: the frame's and the entry's sse pass 2^32."""
    image = np.zeros((263, 301, 3), dtype=np.uint8)
    pal = np.array([[0, 0, 0], [255, 255, 255]], dtype=np.uint8)
    maps = np.ones((263, 301), dtype=np.uint8)
    ent, per, _ = _measure(image, maps, pal, ictcp=False)
    assert 79163 * 195075 > 2 ** 32
    assert ent.tolist() == [[0, 0, 0], [79163, 79163 * 195075, 195075]]
    assert per.tolist() == [[79163, 79163 * 195075, 195075]]


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c_call(gpu, image, maps, elem, palette=None, palette_u8=None, rows=None, skip=-1, outs=(), channels=None, dims=None):
    """patolette_amd_measure itself.  outs: names of the outputs to pass, the others NULL.  Returns (code, {name: array})."""
    F, h, w = dims if dims is not None else maps.shape
    if rows is None:
        rows = (palette_u8 if palette_u8 is not None else palette).shape[0]
    types = dict(entry_count=np.uint64, entry_sse=np.uint64, entry_max_se=np.uint32, frame_count=np.uint64, frame_sse=np.uint64,
                 frame_max_se=np.uint32, frame_d_sum=np.float64, frame_d_max=np.float64)
    arrays = {k: np.full(rows if k.startswith("entry") else maps.shape[0], 77, dtype=t) for k, t in types.items() if k in outs}
    ptr = {np.uint64: C.POINTER(C.c_uint64), np.uint32: C.POINTER(C.c_uint32), np.float64: _native.dp}
    args = [arrays[k].ctypes.data_as(ptr[t]) if k in arrays else None for k, t in types.items()]
    code = C.c_int(7)
    gpu.patolette_amd_measure(F, w, h, _vp(image), image.shape[-1] if channels is None else channels, _vp(maps), elem,
                              None if palette is None else palette.ctypes.data_as(_native.dp), _vp(palette_u8), rows, skip, *args,
                              C.byref(code))
    return code.value, arrays


ALL_OUTS = ("entry_count", "entry_sse", "entry_max_se", "frame_count", "frame_sse", "frame_max_se", "frame_d_sum", "frame_d_max")


def _c_same(arrays, ref):
    """Whatever outputs were asked for, against the reference."""
    ent, per, dist = ref
    for j, key in enumerate(("count", "sse", "max_se")):
        if "entry_" + key in arrays:
            assert np.array_equal(arrays["entry_" + key].astype(np.int64), ent[:, j]), key
        if "frame_" + key in arrays:
            assert np.array_equal(arrays["frame_" + key].astype(np.int64), per[:, j]), key
    for j, key in enumerate(("frame_d_sum", "frame_d_max")):
        if key in arrays:
            assert np.all(np.abs(arrays[key] - dist[:, j]) <= REL * dist[:, j]), key


def test_elements_channels_and_outputs_through_the_c_entry(gpu):
    size, F = SHAPES["odd64"]
    frames = _clip(size, F)
    rgba = np.concatenate([frames, np.full(frames.shape[:3] + (1,), 7, dtype=np.uint8)], axis=-1)     # a 4th byte is ignored
    for rows in (16, 1029):
        pal, maps = _maps(size, F, rows, "ordered")
        ref = _reference(size, F, rows, "ordered")
        _meaningful(ref[2])
        for eb, dt in ((1, np.uint8), (2, np.uint16), (4, np.uint32), (8, np.uint64)):
            if rows > 256 and eb == 1:
                continue
            for image in (frames, rgba):
                code, arrays = _c_call(gpu, image, maps.astype(dt), eb, palette_u8=pal, outs=ALL_OUTS)
                assert code == 0
                _c_same(arrays, ref)
        # each output alone, the others NULL; and none at all
        first = None
        for name in ALL_OUTS:
            code, arrays = _c_call(gpu, frames, maps, maps.dtype.itemsize, palette_u8=pal, outs=(name,))
            assert code == 0 and list(arrays) == [name]
            _c_same(arrays, ref)
            if name == "frame_d_sum":
                first = arrays[name]
        assert _c_call(gpu, frames, maps, maps.dtype.itemsize, palette_u8=pal)[0] == 0
        code, arrays = _c_call(gpu, frames, maps, maps.dtype.itemsize, palette_u8=pal, outs=ALL_OUTS)
        assert code == 0 and np.array_equal(arrays["frame_d_sum"].view(np.uint64), first.view(np.uint64))
    # 8-byte elements: a skip index beyond 32 bits skips its own positions only; another such value is no row
    pal, maps = _maps(size, F, 16, "ordered")
    T = 2 ** 40 + 3
    wide = maps.astype(np.uint64)
    wide[maps == 5] = T
    code, arrays = _c_call(gpu, frames, wide, 8, palette_u8=pal, skip=T, outs=ALL_OUTS)
    assert code == 0
    _c_same(arrays, _reference(size, F, 16, "ordered", skip=5))
    wide[1, 2, 3] = T + 1
    assert _c_call(gpu, frames, wide, 8, palette_u8=pal, skip=T, outs=ALL_OUTS)[0] == -1
    assert _native.last_error().startswith(PREFIX)
    # a skip index that a byte cannot hold skips nothing
    code, arrays = _c_call(gpu, frames, maps, 1, palette_u8=pal, skip=256 + 5, outs=ALL_OUTS)
    assert code == 0
    _c_same(arrays, _reference(size, F, 16, "ordered"))


def test_skip_index_with_deltas(gpu):
    """What frame_deltas made transparent enters nothing: every frame's count is that frame's `changed`."""
    from oracle import binding as ob
    size, F = (37, 53), 4
    frames = _clip(size, F)
    pal, maps = _maps(size, F, 16, "ordered")
    for tolerance in (0.0, 0.05):
        ok, deltas, rects, changed, _, msg = patolette_amd.frame_deltas(maps, pal, transparent_index=255, frames=frames, tolerance=tolerance)
        assert ok, msg
        assert np.any(deltas == 255)
        got = _measure(frames, deltas, pal, skip_index=255)
        assert np.array_equal(got[1][:, 0], changed) and got[0][:, 0].sum() == changed.sum()
        ref = measure_ref.measure(ob, frames, deltas, pal, skip_index=255)
        _meaningful(ref[2])
        _same(got, ref)
    with pytest.raises(ValueError, match="skip_index"):               # without it, 255 is no row of 16
        patolette_amd.measure(frames, deltas, pal)


def test_skip_index_with_rgba(gpu):
    """Index 0 of a quantize_rgba map is the transparent entry: skipped, the count is the number of opaque pixels."""
    from oracle import binding as ob
    image = _image("scene", (40, 56), 1, 4)
    ok, pal_rgba, pmap, quant, _, tidx, msg = patolette_amd.quantize_rgba(image, 16, alpha_threshold=128, dither=False, tile_size=0,
                                                                          kmeans_niter=2, kmeans_max_samples=4096)
    assert ok and tidx == 0, msg
    opaque = int(np.sum(image[..., 3] >= 128))
    assert 0 < opaque < 40 * 56 and np.array_equal(pmap == 0, image[..., 3] < 128)
    pal = np.ascontiguousarray(pal_rgba[:, :3])
    got = _measure(image, pmap, pal, skip_index=0)
    assert got[1][0, 0] == opaque and got[0][0].tolist() == [0, 0, 0]
    ref = measure_ref.measure(ob, image, pmap, pal, skip_index=0)
    _meaningful(ref[2])
    _same(got, ref)
    # the error of the call's own quantized image on the opaque pixels
    vis = image[..., 3] >= 128
    err = (image[..., :3].astype(np.int64) - quant[..., :3].astype(np.int64)) ** 2
    assert got[1][0, 1] == err[vis].sum()


def test_a_skip_index_that_names_a_used_row(gpu):
    size, F = SHAPES["tiles"]
    pal, maps = _maps(size, F, 16, "nearest")
    skip = int(np.bincount(maps.reshape(-1)).argmax())
    ref = _reference(size, F, 16, "nearest", skip=skip)
    _meaningful(ref[2])
    got = _measure(_clip(size, F), maps, pal, skip_index=skip)
    _same(got, ref)
    assert got[0][skip].tolist() == [0, 0, 0] and got[0][:, 0].sum() == maps.size - int(np.sum(maps == skip))
    nothing = _measure(_clip(size, F)[0], np.full(size, 3, dtype=np.uint8), pal, skip_index=3)       # everything skipped
    assert not nothing[0].any() and nothing[1].tolist() == [[0, 0, 0]] and nothing[2].tolist() == [[0.0, 0.0]]
    assert np.isnan(patolette_amd.psnr(nothing[1])).all()


def test_the_exact_case(gpu):
    """A remap's own quantized image on its palette bytes and its map: no error in code values, and -- pixel and palette taking the same
    conversion of the same value on the device and the host, which agree to the pow bound -- D within the square of the 1e-9 bar."""
    size, F = SHAPES["tiles"]
    for rows in (16, 300):
        pal = _palette(rows, seed=2)
        ok, pmap, quant, msg = patolette_amd.remap(_clip(size, F), pal, dither=False)
        assert ok, msg
        ent, per, dist = _measure(quant, pmap, pal)
        print("exact case, %d rows: d_sum %s d_max %s" % (rows, dist[:, 0].tolist(), dist[:, 1].tolist()))
        assert ent[:, 0].sum() == pmap.size and not ent[:, 1:].any() and not per[:, 1:].any()
        assert np.all(dist[:, 1] <= 1e-18) and np.all(dist >= 0.0)
        assert np.all(np.isinf(patolette_amd.psnr(per)))


def test_cross_check_with_the_lossy_deltas(gpu):
    size, F = (37, 53), 4
    frames = _clip(size, F)
    pal, maps = _maps(size, F, 16, "ordered")
    ok, _, _, _, shown, msg = patolette_amd.frame_deltas(maps, pal, frames=frames, tolerance=0.05, want_shown=True)
    assert ok, msg
    assert np.any(shown != maps)
    of_maps, of_shown = _measure(frames, maps, pal), _measure(frames, shown, pal)
    bound = np.maximum(0.05 * 0.05, of_maps[2][:, 1]) * (1 + 1e-9)
    print("d_max of shown %s, bound %s" % (of_shown[2][:, 1].tolist(), bound.tolist()))
    assert np.all(of_shown[2][:, 1] <= bound)
    assert np.array_equal(of_shown[1][:, 0], of_maps[1][:, 0])
    if of_shown[1][:, 1].sum() < of_maps[1][:, 1].sum():              # (not asserted: the sRGB error need not follow the ICtCp choice)
        print("sse of shown %d is below that of maps %d" % (of_shown[1][:, 1].sum(), of_maps[1][:, 1].sum()))


def _bits(got):
    return [np.ascontiguousarray(a).view(np.uint64).tolist() for a in got]


def test_a_function_of_the_arguments_alone(gpu):
    size, F = SHAPES["tiles"]
    frames = _clip(size, F)
    for rows in (255, 1029):
        pal, maps = _maps(size, F, rows, "nearest")
        first = _bits(_measure(frames, maps, pal))
        assert _bits(_measure(frames, maps, pal)) == first            # the same call twice
        big = _image("noise", (512, 600), 1, 3)                       # after a larger call of its own and one of another entry
        _measure(big, np.zeros((512, 600), dtype=np.uint8), pal[:7])
        ok, *_ = patolette_amd.remap(big, pal[:16], dither=False)
        assert ok
        assert _bits(_measure(frames, maps, pal)) == first
        gpu.patolette_amd_release_workspace()
        assert _bits(_measure(frames, maps, pal)) == first
        assert _bits(_measure(frames, maps.astype(np.uint32), pal)) == first       # the element size changes nothing
    ref = _reference(size, F, 1029, "nearest")
    _meaningful(ref[2])
    _same(_measure(frames, maps, pal), ref)


def test_torch_flavour(gpu):
    """Torch CUDA tensors go through patolette_amd_measure_device: the numpy flavour's results, bit for bit, the f64 ones included.
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
from oracle import binding as ob
from tests import delta_ref
from tests.test_gpu_remap import _palette
for size, F, rows in (((263, 301), 2, 16), ((37, 53), 3, 300), ((40, 56), 1, 255), ((37, 53), 3, 1029)):
    frames, pal = delta_ref.clip(size[0], size[1], F), _palette(rows, seed=2)
    maps = delta_ref.maps_of(ob, frames, pal, "nearest")
    m_np = maps.astype(np.uint8 if rows <= 256 else np.uint16)
    m_t = torch.from_numpy(maps.astype(np.uint8 if rows <= 256 else np.int32)).cuda()
    f_t = torch.from_numpy(frames).cuda()
    for kw in (dict(), dict(skip_index=3), dict(ictcp=False)):
        ok, ent, per, dist, msg = p.measure(frames, m_np, pal, **kw)
        assert ok, msg
        ok, ent_t, per_t, dist_t, msg = p.measure(f_t, m_t, pal, **kw)
        assert ok, msg
        assert all(isinstance(a, np.ndarray) for a in (ent_t, per_t))
        assert np.array_equal(ent_t, ent) and np.array_equal(per_t, per)
        if dist is None:
            assert dist_t is None
        else:
            assert isinstance(dist_t, np.ndarray) and np.array_equal(dist_t.view(np.uint64), dist.view(np.uint64))
    ok, ent1, per1, dist1, msg = p.measure(f_t[0], m_t[0], torch.from_numpy(pal))         # one image; a tensor palette is host data
    assert ok and per1.shape == (1, 3) and dist1.shape == (1, 2), msg
    ok, ent0, per0, dist0, msg = p.measure(frames[0], m_np[0], pal)
    assert ok and np.array_equal(ent1, ent0) and np.array_equal(per1, per0) and np.array_equal(dist1.view(np.uint64), dist0.view(np.uint64))
    for image, m in ((frames, m_t), (f_t, m_np)):
        try:
            p.measure(image, m, pal)
            raise SystemExit("an image and maps in different places were accepted")
        except ValueError:
            pass
    try:
        p.measure(f_t, m_t.to(torch.int64), pal)
        raise SystemExit("int64 tensor maps were accepted")
    except ValueError:
        pass
print("TORCH-MEASURE-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-MEASURE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_failures_and_recovery(gpu):
    size, F = SHAPES["tile"]
    h, w = size
    frames = _clip(size, F)
    pal, maps = _maps(size, F, 16, "ordered")
    palf = np.asfortranarray(pal.astype(np.float64) / 255.0)
    ref = _reference(size, F, 16, "ordered")
    _meaningful(ref[2])

    def call(m=maps, **kw):
        args = dict(palette_u8=pal, outs=ALL_OUTS)
        args.update(kw)
        return _c_call(gpu, args.pop("image", frames), m, args.pop("elem", 1), **args)[0]

    def good():
        code, arrays = _c_call(gpu, frames, maps, 1, palette_u8=pal, outs=ALL_OUTS)
        assert code == 0
        _c_same(arrays, ref)

    def failed(code, *words):
        assert code == -1
        text = _native.last_error()
        assert text.startswith(PREFIX) and all(word in text for word in words), text
        good()

    good()
    # an element that is no row: the kernel's flag
    bad = maps.copy()
    bad[0, 17, 5] = 16
    failed(call(m=bad), "palette_rows")
    failed(call(m=bad, outs=("entry_count",)), "palette_rows")
    failed(call(m=bad, skip=17), "palette_rows")                      # (another index is skipped, not this one)
    assert call(m=bad, skip=16) == 0
    bad = maps.copy()
    bad[0, 39, 55] = 255
    failed(call(m=bad), "palette_rows")
    filled = np.full((20, 3), -1.0, order="F")                        # ... and one that names a dropped trailing row
    filled[:16] = palf
    bad = maps.copy()
    bad[0, 0, 0] = 17
    failed(call(m=bad, palette_u8=None, palette=filled), "dropped")
    assert call(palette_u8=None, palette=filled) == 0
    with pytest.raises(ValueError, match="palette_rows"):
        patolette_amd.measure(frames, bad, pal)
    good()
    # -1: the arguments
    failed(call(elem=3), "map_elem_bytes")
    failed(call(elem=0), "map_elem_bytes")
    failed(call(channels=2), "channels")
    failed(call(channels=5), "channels")
    failed(call(palette=palf), "exactly one")
    failed(call(palette_u8=None, rows=16), "exactly one")
    failed(call(rows=0), "palette_rows")
    failed(call(skip=-2), "skip_index")
    nan = palf.copy(order="F")
    nan[3, 1] = np.nan
    failed(call(palette_u8=None, palette=nan), "finite")
    failed(call(palette_u8=None, palette=np.full((16, 3), -1.0, order="F")), "unused-row")
    none = [None] * 8
    code = C.c_int(7)
    gpu.patolette_amd_measure(F, w, h, None, 3, _vp(maps), 1, None, _vp(pal), 16, -1, *none, C.byref(code))
    failed(code.value, "no pixels")
    gpu.patolette_amd_measure(F, w, h, _vp(frames), 3, None, 1, None, _vp(pal), 16, -1, *none, C.byref(code))
    failed(code.value, "no maps")
    # -2 and -4
    assert call(dims=(0, h, w)) == -2
    assert call(dims=(F, 0, w)) == -2
    assert call(dims=(F, h, 0)) == -2
    good()
    assert call(dims=(1 << 31, h, w)) == -4 and _native.last_error().startswith(PREFIX) and "too big" in _native.last_error()
    assert call(dims=(1, 50000, 50000)) == -4
    good()
    ok, *rest, msg = patolette_amd.measure(np.zeros((0, 5, 3), dtype=np.uint8), np.zeros((0, 5), dtype=np.uint8), pal)
    assert not ok and rest == [None] * 3 and msg == "Image dimensions should be greater than 0."


def test_last_stats_and_the_kernels(gpu):
    size, F = SHAPES["tiles"]
    pal, maps = _maps(size, F, 255, "nearest")
    for ictcp in (True, False):
        _native.profile(True)
        _measure(_clip(size, F), maps, pal, ictcp=ictcp)
        prof = _native.profile_results()
        _native.profile(False)
        assert prof["k_measure"]["launches"] == 1 and prof["k_measure_fold"]["launches"] == 1      # one launch for all frames
        assert not set(prof) & {"k_convert_u8", "k_convert", "k_nn_map", "k_nn_map_u8", "k_ordered_map", "k_frame_deltas"}
        st = patolette_amd.last_stats()
        assert st["ms_total"] > 0 and st["ms_map"] > 0 and st["ms_upload"] > 0 and st["ms_total"] >= st["ms_map"]
        assert all(st[key] == 0 for key in st if not key.startswith("ms_"))
        assert st["ms_convert"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0 and st["ms_kmeans"] == 0 and st["ms_saliency"] == 0
