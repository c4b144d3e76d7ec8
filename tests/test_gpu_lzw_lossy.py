"""gif_lzw_lossy / patolette_amd_gif_lzw_lossy and write_gif(near=...) on the device against tests/lzw_lossy_ref.py.

`data`, `offsets` and `coded` are compared bit for bit with the reference, and the device's streams are also decoded by the
independent decoder of tests/lzw_ref.py back to `coded`.  The shapes are those of tests/test_gpu_lzw.py, the smallest at which each
part can go wrong, under an empty table, a pairing table (s ^ 1) and a dense one (15 candidates a row)."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import delta_ref, lzw_lossy_ref, lzw_ref
from tests.test_gpu_lzw import SHAPES, _cases, _maps
from tests.test_lzw_lossy_reference import HAND, hand_table
from tests.util import ROOT

pytestmark = pytest.mark.gpu

PREFIX = "patolette_amd_gif_lzw_lossy:"
TABLES = ("empty", "pairing", "dense")


@pytest.fixture(autouse=True)
def _defaults_again(gpu):
    yield
    _native.profile(False)


@functools.lru_cache(maxsize=None)
def _table(name, m):
    near = {"empty": lambda m: lzw_lossy_ref.empty_table(), "pairing": lzw_lossy_ref.pairing_table, "dense": lzw_lossy_ref.dense_table,
            "counts": lzw_lossy_ref.counts_table}[name](m)
    near.setflags(write=False)
    return near


@functools.lru_cache(maxsize=None)
def _reference(kind, size, F, m, segment, table):
    ref = lzw_lossy_ref.encode_frames_lossy(_maps(kind, size, F, m), _table(table, m), None, m, segment or lzw_ref.DEFAULT_SEGMENT)
    for a in ref:
        a.setflags(write=False)
    return ref


def _lossy(maps, near, rects=None, m=8, segment=None):
    ok, data, offsets, coded, msg = patolette_amd.gif_lzw_lossy(maps, near, rects, m, segment, want_coded=True)
    assert ok, msg
    assert isinstance(data, np.ndarray) and data.dtype == np.uint8 and offsets.dtype == np.int64
    assert isinstance(coded, np.ndarray) and coded.dtype == np.uint8 and coded.shape == np.asarray(maps).shape
    return data, offsets, coded


def _same(got, ref):
    data, offsets, coded = got
    assert np.array_equal(offsets, ref[1]), (offsets.tolist()[-3:], ref[1].tolist()[-3:])
    wrong = int(np.sum(data != ref[0]))
    print("%d of %d bytes and %d of %d coded entries differ from the reference" % (wrong, ref[0].size, int(np.sum(coded != ref[2])), coded.size))
    assert wrong == 0
    assert np.array_equal(coded, ref[2].reshape(coded.shape))


def _decoded(got, rects, m):
    """(a): the device's streams through the independent decoder are the device's coded maps inside every rectangle."""
    data, offsets, coded = got
    coded = coded if coded.ndim == 3 else coded[None]
    for f in range(coded.shape[0]):
        x0, y0, w, h = (0, 0, coded.shape[2], coded.shape[1]) if rects is None else (int(v) for v in rects[f])
        sym = lzw_ref.decode(data[offsets[f]:offsets[f + 1]].tobytes(), m, w * h)
        assert sym == coded[f, y0:y0 + h, x0:x0 + w].reshape(-1).tolist(), f


def _exact_of_coded(got, rects, m, segment):
    """(b): the exact coder on the device, given the coded maps, returns the lossy call's bytes."""
    ok, data, offsets, msg = patolette_amd.gif_lzw(got[2], rects, m, segment)
    assert ok, msg
    assert np.array_equal(offsets, got[1]) and np.array_equal(data, got[0])


@pytest.mark.parametrize("table", ["pairing", "dense"])
@pytest.mark.parametrize("segment", [50, 350, None])
@pytest.mark.parametrize("m", [2, 8])
def test_every_ending_position(gpu, m, segment, table):
    """ONE call: 700 frames of one row, frame f compressing its first f + 1 symbols."""
    maps = lzw_ref.contents("noise", 700 * 700, m).reshape(700, 1, 700)
    rects = np.array([(0, 0, f + 1, 1) for f in range(700)], dtype=np.int32)
    near = _table(table, m)
    got = _lossy(maps, near, rects, m, segment)
    _same(got, lzw_lossy_ref.encode_frames_lossy(maps, near, rects, m, segment or 8192))
    _decoded(got, rects, m)
    assert np.any(got[2] != maps)


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_contents_segments_and_tables(gpu, name):
    """The full cross with the three tables for the small shapes; for the one of 10^5 symbols and more, test_gpu_lzw.py's subset with
    the tables taken in turn (every table meets every m and every segment at least once over the two rotations)."""
    size, F = SHAPES[name]
    substituted = 0
    for n, (kind, m, segment) in enumerate(_cases(name)):
        maps = _maps(kind, size, F, m)
        for table in (TABLES[n % 3], TABLES[(n // 3 + 1) % 3]) if name == "tiles" else TABLES:
            got = _lossy(maps, _table(table, m), None, m, segment)
            ref = _reference(kind, size, F, m, segment, table)
            _same(got, ref)
            assert got[0].size <= patolette_amd.gif_lzw_bound([[0, 0, size[1], size[0]]] * F, segment)
            substituted += int(np.sum(got[2] != maps))
            if table == "empty":
                assert np.array_equal(got[2], maps)
            if maps.size <= 8000:
                _decoded(got, None, m)
                _exact_of_coded(got, None, m, segment)
    assert substituted > 0 or name == "one"
    one = _lossy(_maps("noise", size, F, 8)[0], _table("pairing", 8))              # an (H, W) map is one frame; the defaults
    _same(one, lzw_lossy_ref.encode_frames_lossy(_maps("noise", size, F, 8)[:1], _table("pairing", 8)))


@pytest.mark.parametrize("name", list(HAND))
def test_hand_written_priorities(gpu, name):
    m, x, _, codes, want_coded = HAND[name]
    maps = np.array(x, dtype=np.uint8).reshape(1, 1, len(x))
    acc, at = 0, 0
    for code, width in codes:
        acc |= code << at
        at += width
    data, offsets, coded = _lossy(maps, hand_table(name), None, m)
    assert data.tobytes() == acc.to_bytes((at + 7) // 8, "little") and offsets.tolist() == [0, (at + 7) // 8]
    assert coded.reshape(-1).tolist() == want_coded


def test_every_count(gpu):
    """Rows with every count 0 .. 15: lanes beyond the count take no part, whatever the rest of the row holds."""
    for m in (4, 5, 8):
        near = _table("counts", m).copy()
        assert set(near[:1 << m, 0].tolist()) == set(range(16))
        for s in range(1 << m):
            near[s, 1 + near[s, 0]:] = (s + 1) % (1 << m)                            # bytes behind the count: never read
        for kind in ("noise", "ramp"):
            maps = _maps(kind, (37, 53), 3, m)
            for segment in (64, None):
                got = _lossy(maps, near, None, m, segment)
                _same(got, lzw_lossy_ref.encode_frames_lossy(maps, _table("counts", m), None, m, segment or 8192))
                _decoded(got, None, m)


def test_the_full_dictionary_with_the_pairing_table(gpu):
    maps = _maps("noise", (96, 96), 1, 8)
    near = _table("pairing", 8)
    codes = []
    lzw_lossy_ref.encode_lossy(maps.reshape(-1), 8, near, 65536, codes)
    inner = [i for i, (c, w) in enumerate(codes) if c == 256 and i > 0]
    assert inner and all(codes[i][1] == 12 for i in inner)                           # a Clear that is no segment boundary
    got = _lossy(maps, near, None, 8, 65536)
    _same(got, _reference("noise", (96, 96), 1, 8, 65536, "pairing"))
    _decoded(got, None, 8)
    _exact_of_coded(got, None, 8, 65536)


def test_an_empty_table_is_the_exact_coder_and_coded_maps_recode_exactly(gpu):
    """(e) device against device, and (b) through gif_lzw(coded), on rectangles."""
    size, F = SHAPES["tiles"]
    rects = np.array([(3, 2, 290, 250), (0, 0, 301, 263)], dtype=np.int32)
    for m, segment in ((5, 300), (8, None)):
        maps = _maps("noise", size, F, m)
        ok, data, offsets, msg = patolette_amd.gif_lzw(maps, rects, m, segment)
        assert ok, msg
        got = _lossy(maps, _table("empty", m), rects, m, segment)
        assert np.array_equal(got[0], data) and np.array_equal(got[1], offsets) and np.array_equal(got[2], maps)
        for table in ("pairing", "dense"):
            got = _lossy(maps, _table(table, m), rects, m, segment)
            assert got[0].size < data.size and np.any(got[2] != maps)
            _exact_of_coded(got, rects, m, segment)


RECTS = np.array([(10, 7, 20, 11), (0, 5, 9, 20), (44, 5, 9, 20), (5, 0, 30, 4), (5, 33, 30, 4), (0, 0, 53, 37), (17, 19, 1, 1), (0, 36, 53, 1),
                  (52, 0, 1, 37), (0, 0, 1, 1), (52, 36, 1, 1), (3, 2, 47, 33)], dtype=np.int32)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c_call(gpu, maps, near, rects=None, m=8, segment=0, capacity=None, dims=None, out=True, offsets=True, coded=True, sentinel=0x5A):
    """patolette_amd_gif_lzw_lossy itself.  Returns (code, out array, offsets array, coded array filled with the sentinel first)."""
    F, h, w = dims if dims is not None else maps.shape
    r = None if rects is None else np.ascontiguousarray(rects, dtype=np.int32)
    if capacity is None:
        capacity = patolette_amd.gif_lzw_bound([[0, 0, maps.shape[2], maps.shape[1]]] * maps.shape[0], segment if 1 <= segment <= 1 << 24 else None)
    buf = np.full(capacity, 0xAA, dtype=np.uint8)
    off = np.full(maps.shape[0] + 1, 77, dtype=np.uint64)
    cod = np.full(maps.shape, sentinel, dtype=np.uint8) if coded is True else coded
    code = C.c_int(7)
    gpu.patolette_amd_gif_lzw_lossy(F, w, h, _vp(maps), None if r is None else r.ctypes.data_as(C.POINTER(C.c_int32)), m, segment, _vp(near), _vp(cod),
                                    _vp(buf) if out and capacity else None, capacity, off.ctypes.data_as(C.POINTER(C.c_uint64)) if offsets else None,
                                    C.byref(code))
    return code.value, buf, off, cod


def test_rectangles_and_what_lies_outside_them(gpu):
    h, w, F = 37, 53, len(RECTS)
    for m in (3, 8):
        maps = lzw_ref.contents("noise", F * h * w, m, seed=9).reshape(F, h, w)
        for table in ("pairing", "dense"):
            near = _table(table, m)
            for segment in (7, 64, None):
                got = _lossy(maps, near, RECTS, m, segment)
                ref = lzw_lossy_ref.encode_frames_lossy(maps, near, RECTS, m, segment or 8192)
                _same(got, ref)
                _decoded(got, RECTS, m)
                _exact_of_coded(got, RECTS, m, segment)
            # at the C level a sentinel-filled `coded` stays untouched outside the rectangles
            code, buf, off, cod = _c_call(gpu, maps, near, RECTS, m, 64)
            assert code == 0
            inside = np.zeros(maps.shape, dtype=bool)
            for f, (x0, y0, rw, rh) in enumerate(RECTS):
                inside[f, y0:y0 + rh, x0:x0 + rw] = True
            ref = lzw_lossy_ref.encode_frames_lossy(maps, near, RECTS, m, 64)
            assert np.all(cod[~inside] == 0x5A) and np.array_equal(cod[inside], ref[2][inside])
            assert np.array_equal(buf[:int(off[-1])], ref[0])
            code, buf2, off2, _ = _c_call(gpu, maps, near, RECTS, m, 64, coded=None)       # coded is optional
            assert code == 0 and np.array_equal(off2, off) and np.array_equal(buf2, buf)
    empty, as_one = RECTS.copy(), RECTS.copy()                                      # an empty rectangle stands for (0, 0, 1, 1)
    empty[3], as_one[3] = (0, 0, 0, 0), (0, 0, 1, 1)
    _same(_lossy(maps, near, empty, 8), lzw_lossy_ref.encode_frames_lossy(maps, near, as_one, 8))


@functools.lru_cache(maxsize=None)
def _clip(size, F, t1):
    """delta_ref's clip on 255 rows, ordered maps, its deltas (T = 255) and shown maps: made on the device by entries their own suites check."""
    frames = delta_ref.clip(size[0], size[1], F)
    ok, pal8, maps, _, _, msg = patolette_amd.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2, want_quantized=False)
    assert ok and maps.dtype == np.uint8 and pal8.shape == (255, 3), msg
    ok, deltas, rects, changed, shown, msg = patolette_amd.frame_deltas(maps, pal8, transparent_index=255, frames=frames, tolerance=t1, want_shown=True)
    assert ok, msg
    for a in (frames, pal8, deltas, rects, shown):
        a.setflags(write=False)
    return frames, pal8, deltas, rects, shown


def test_transparency_is_never_lossy(gpu):
    """(d): the transparent index of a delta map has an empty row and is in no row: it survives exactly, and nothing else becomes it."""
    _, pal8, deltas, rects, _ = _clip((37, 53), 8, 0.0)
    ok, near, msg = patolette_amd.gif_neighbours(pal8, 0.1, transparent_index=255)
    assert ok and near[255, 0] == 0 and np.any(near[:255, 0] > 0), msg
    assert not any(255 in near[s, 1:1 + near[s, 0]].tolist() for s in range(256))
    assert np.mean(deltas[1:] == 255) > 0.3
    for use_rects in (None, rects):
        for segment in (300, None):
            got = _lossy(deltas, near, use_rects, 8, segment)
            _same(got, lzw_lossy_ref.encode_frames_lossy(deltas, near, use_rects, 8, segment or 8192))
            assert np.array_equal(got[2] == 255, deltas == 255)
            assert np.any(got[2] != deltas)
            _decoded(got, use_rects if use_rects is None else np.where(rects[:, 2:3] == 0, np.array([[0, 0, 1, 1]]), rects), 8)


def test_elements_outside_the_rectangles_and_the_flag(gpu):
    h, w, m = 37, 53, 3
    near = _table("dense", m)
    maps = lzw_ref.contents("noise", 2 * h * w, m).reshape(2, h, w).copy()
    rects = np.array([(10, 7, 20, 11), (1, 1, 51, 35)], dtype=np.int32)
    ref = lzw_lossy_ref.encode_frames_lossy(maps, near, rects, m, 64)
    outside = maps.copy()
    outside[0, :7] = 255
    outside[0, 7:18, :10] = 8
    outside[0, 7:18, 30:] = 200
    outside[0, 18:] = 9
    outside[1, 0], outside[1, 36], outside[1, :, 0], outside[1, :, 52] = 8, 255, 77, 8
    got = _lossy(outside, near, rects, m, 64)                                      # not read: no flag, the same streams
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    inside = np.zeros(maps.shape, dtype=bool)
    inside[0, 7:18, 10:30], inside[1, 1:36, 1:52] = True, True
    assert np.array_equal(got[2][inside], ref[2][inside]) and np.array_equal(got[2][~inside], outside[~inside])
    for f, y, x, v in ((0, 7, 10, 8), (0, 17, 29, 255), (1, 35, 51, 8), (1, 20, 20, 9)):
        bad = maps.copy()
        bad[f, y, x] = v
        code, *_ = _c_call(gpu, bad, near, rects, m, 64)
        assert code == -1
        text = _native.last_error()
        assert text.startswith(PREFIX) and "min_code_size" in text, text
        with pytest.raises(ValueError, match="min_code_size"):
            patolette_amd.gif_lzw_lossy(bad, near, rects, m, 64)
        _same(_lossy(maps, near, rects, m, 64), ref)                               # the next call works


def test_capacity(gpu):
    maps, near = _maps("noise", (37, 53), 3, 5), _table("pairing", 5)
    ref = _reference("noise", (37, 53), 3, 5, 300, "pairing")
    need = int(ref[1][-1])
    code, buf, off, cod = _c_call(gpu, maps, near, None, 5, 300, capacity=need)
    assert code == 0 and np.array_equal(buf, ref[0]) and np.array_equal(off.astype(np.int64), ref[1]) and np.array_equal(cod, ref[2])
    code, buf, off, _ = _c_call(gpu, maps, near, None, 5, 300, capacity=need - 1)
    assert code == -1 and _native.last_error().startswith(PREFIX) and "capacity" in _native.last_error()
    assert int(off[3]) == need and np.array_equal(off.astype(np.int64), ref[1]) and np.all(buf == 0xAA)     # nothing copied
    code, buf, off, _ = _c_call(gpu, maps, near, None, 5, 300, capacity=0)
    assert code == -1 and int(off[3]) == need
    code, buf, off, _ = _c_call(gpu, maps, near, None, 5, 300, capacity=need + 5)
    assert code == 0 and np.array_equal(buf[:need], ref[0]) and np.all(buf[need:] == 0xAA)


def test_failures_and_recovery(gpu):
    size, F, m = (40, 56), 2, 5
    h, w = size
    maps, near = _maps("ramp", size, F, m), _table("dense", m)
    ref = _reference("ramp", size, F, m, None, "dense")

    def good():
        code, buf, off, cod = _c_call(gpu, maps, near, None, m)
        assert code == 0 and np.array_equal(off.astype(np.int64), ref[1]) and np.array_equal(buf[:int(off[-1])], ref[0]) and np.array_equal(cod, ref[2])

    def failed(result, *words):
        assert result[0] == -1
        text = _native.last_error()
        assert text.startswith(PREFIX) and all(word in text for word in words), text
        good()

    good()
    failed(_c_call(gpu, maps, near, None, 1), "min_code_size")
    failed(_c_call(gpu, maps, near, None, 9), "min_code_size")
    failed(_c_call(gpu, maps, near, None, m, (1 << 24) + 1), "segment")
    failed(_c_call(gpu, maps, near, None, m, offsets=False), "offsets")
    failed(_c_call(gpu, maps, near, None, m, out=False), "no out")
    failed(_c_call(gpu, maps, None, None, m), "no near")
    count16, cand32 = near.copy(), near.copy()
    count16[31, 0], cand32[0, 15] = 16, 32
    failed(_c_call(gpu, maps, count16, None, m), "count")
    failed(_c_call(gpu, maps, cand32, None, m), "candidate")
    beyond = near.copy()                                                            # rows at and above 2^m, and bytes behind a count: not read
    beyond[32:], beyond[7, 0], beyond[7, 4:] = 255, 3, 255
    code, buf, off, _ = _c_call(gpu, maps, beyond, None, m)
    want = lzw_lossy_ref.encode_frames_lossy(maps, beyond, None, m)
    assert code == 0 and np.array_equal(buf[:int(off[-1])], want[0])
    failed(_c_call(gpu, maps, near, None, m, coded=maps), "overlap")
    two = np.concatenate([maps, maps])
    failed(_c_call(gpu, two[:F], near, None, m, coded=two.reshape(-1)[h * w // 2:h * w // 2 + maps.size].reshape(maps.shape)), "overlap")
    full = [0, 0, w, h]
    for rect in ([0, 0, 0, 0], [0, 0, w + 1, h], [0, 0, w, h + 1], [-1, 0, 3, 3], [0, -1, 3, 3], [w - 2, 0, 3, 3], [0, h - 2, 3, 3], [5, 5, 0, 3],
                 [5, 5, 3, 0], [5, 5, -2, 3]):
        failed(_c_call(gpu, maps, near, [full, rect], m), "rectangle")
        failed(_c_call(gpu, maps, near, [rect, full], m), "rectangle")
    code = C.c_int(7)
    off = np.zeros(F + 1, dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint8)
    gpu.patolette_amd_gif_lzw_lossy(F, w, h, None, None, m, 0, _vp(near), None, _vp(buf), 64, off.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(code))
    failed((code.value,), "no maps")
    bad = maps.copy()
    bad[1, 39, 55] = 32
    failed(_c_call(gpu, bad, near, None, m), "min_code_size")
    # -2 and -4
    assert _c_call(gpu, maps, near, None, m, dims=(0, h, w))[0] == -2
    assert _c_call(gpu, maps, near, None, m, dims=(F, 0, w))[0] == -2
    assert _c_call(gpu, maps, near, None, m, dims=(F, h, 0))[0] == -2
    good()
    assert _c_call(gpu, maps, near, None, m, dims=(1 << 31, h, w))[0] == -4 and _native.last_error().startswith(PREFIX) and "too big" in _native.last_error()
    assert _c_call(gpu, maps, near, None, m, dims=(1, 50000, 50000))[0] == -4
    good()
    ok, data, offsets, coded, msg = patolette_amd.gif_lzw_lossy(np.zeros((0, 5, 7), dtype=np.uint8), near, want_coded=True)
    assert not ok and data is None and offsets is None and coded is None and msg == "Image dimensions should be greater than 0."
    ok, data, offsets, coded, msg = patolette_amd.gif_lzw_lossy(maps, near, None, m)
    assert ok and coded is None and np.array_equal(data, ref[0])


def test_torch_flavour(gpu):
    """Torch CUDA tensors go through patolette_amd_gif_lzw_lossy_device: the numpy flavour's bytes, and `coded` a CUDA tensor that is no
    view of the maps.  Own process: torch loads its HIP runtime before libpatolette_amd.so does."""
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
from tests import lzw_ref, lzw_lossy_ref
for (F, h, w), m, segment in (((3, 37, 53), 8, None), ((2, 263, 301), 5, 300), ((1, 1, 1), 2, None), ((2, 301, 1), 3, 7)):
    maps = lzw_ref.contents("noise", F * h * w, m).reshape(F, h, w)
    near = lzw_lossy_ref.dense_table(m)
    rects = np.array([(0, 0, w, h)] * (F - 1) + [(w // 3, h // 3, w - w // 3, h - h // 3)], dtype=np.int32)
    t = torch.from_numpy(maps).cuda()
    for r in (None, rects):
        ok, data, off, coded, msg = p.gif_lzw_lossy(maps, near, r, m, segment, want_coded=True)
        assert ok, msg
        ok, data_t, off_t, coded_t, msg = p.gif_lzw_lossy(t, near, r, m, segment, want_coded=True)
        assert ok, msg
        assert isinstance(data_t, np.ndarray) and isinstance(off_t, np.ndarray)
        assert np.array_equal(off_t, off) and np.array_equal(data_t, data)
        assert torch.is_tensor(coded_t) and coded_t.is_cuda and coded_t.dtype == torch.uint8 and coded_t.data_ptr() != t.data_ptr()
        assert np.array_equal(coded_t.cpu().numpy(), coded) and np.array_equal(t.cpu().numpy(), maps)
        ref = lzw_lossy_ref.encode_frames_lossy(maps, near, r, m, segment or 8192)
        assert np.array_equal(off_t, ref[1]) and np.array_equal(data_t, ref[0]) and np.array_equal(coded, ref[2])
        ok, data_e, off_e, msg = p.gif_lzw(coded_t, r, m, segment)              # (b), on the device from end to end
        assert ok and np.array_equal(data_e, data) and np.array_equal(off_e, off)
        ok, data_n, off_n, none, msg = p.gif_lzw_lossy(t, near, r, m, segment)
        assert ok and none is None and np.array_equal(data_n, data)
    blob_t = p.write_gif(None, t, np.zeros((1 << m, 3), dtype=np.uint8), rects, near=near)
    assert blob_t == p.write_gif(None, maps, np.zeros((1 << m, 3), dtype=np.uint8), rects, near=near)
    assert blob_t != p.write_gif(None, maps, np.zeros((1 << m, 3), dtype=np.uint8), rects) or maps.size == 1
print("TORCH-LZW-LOSSY-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-LZW-LOSSY-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_last_stats_and_the_kernels(gpu):
    size, F = SHAPES["tiles"]
    maps = _maps("noise", size, F, 8)
    names = {"k_lzw_lossy_segments", "k_lzw_offsets", "k_lzw_pack"}
    for segment in (300, None):
        _native.profile(True)
        _lossy(maps, _table("pairing", 8), None, 8, segment)
        prof = _native.profile_results()
        _native.profile(False)
        assert all(prof[k]["launches"] == 1 for k in names)                          # one launch each, all frames
        assert {k for k in prof if prof[k]["launches"]} == names
        st = patolette_amd.last_stats()
        assert st["ms_total"] > 0 and st["ms_map"] > 0 and st["ms_upload"] > 0 and st["ms_total"] >= st["ms_map"]
        assert all(st[key] == 0 for key in st if not key.startswith("ms_"))
        assert st["ms_convert"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0 and st["ms_kmeans"] == 0 and st["ms_saliency"] == 0


@pytest.mark.parametrize("size,F", [((37, 53), 8), ((120, 64), 6)])
def test_end_to_end(gpu, ob, size, F, tmp_path):
    """quantize_frames(.., 255, dither="ordered") -> frame_deltas(tolerance=t1, want_shown=True) -> gif_neighbours(pal8, t2, transparent_index=255)
    -> write_gif(.., near=near): the file, parsed, decoded by the independent decoder and composited, is the composite of `coded`; PIL,
    where it is installed, sees the same frames; every composited entry lies within t2 of `shown`'s entry at its position."""
    for t1, t2 in ((0.0, 0.05), (0.05, 0.02)):
        frames, pal8, deltas, rects, shown = _clip(size, F, t1)
        ok, near, msg = patolette_amd.gif_neighbours(pal8, t2, transparent_index=255)
        assert ok, msg
        path = tmp_path / ("clip_%g_%g.gif" % (t1, t2))
        blob = patolette_amd.write_gif(path, deltas, pal8, rects, transparent_index=255, loop=2, near=near)
        assert path.read_bytes() == blob
        exact = patolette_amd.write_gif(None, deltas, pal8, rects, transparent_index=255, loop=2)
        print("%s t1 %g t2 %g: %d bytes, %d by the exact coder" % (size, t1, t2, len(blob), len(exact)))
        head, parsed = lzw_ref.parse_gif(blob)
        assert (head["width"], head["height"], head["loop"]) == (size[1], size[0], 2)
        assert len(parsed) == F and all(fr["m"] == 8 and fr["transparent"] == 255 and fr["disposal"] == 1 for fr in parsed)
        want_rects = [tuple(int(v) for v in r) if r[2] else (0, 0, 1, 1) for r in rects]
        assert [fr["rect"] for fr in parsed] == want_rects
        data, offsets, coded = _lossy(deltas, near, rects)
        assert [fr["stream"] for fr in parsed] == [data[offsets[f]:offsets[f + 1]].tobytes() for f in range(F)]
        # the composite of `coded`: inside its rectangle every coded entry but the transparent one overwrites the canvas
        canvas, drawn = np.full(size, -1, dtype=np.int64), []
        for f, (x0, y0, w, h) in enumerate(want_rects):
            part = coded[f, y0:y0 + h, x0:x0 + w].astype(np.int64)
            canvas[y0:y0 + h, x0:x0 + w] = np.where(part == 255, canvas[y0:y0 + h, x0:x0 + w], part)
            drawn.append(canvas.copy())
        drawn = np.stack(drawn)
        composite = lzw_ref.composite(head, parsed)
        assert np.array_equal(composite, drawn) and composite.min() >= 0 and composite.max() < 255
        D = lzw_lossy_ref.distances(pal8)
        worst = float(np.sqrt(D[composite, shown.astype(np.int64)].max()))
        print("  the largest ICtCp distance of a composited entry to shown's: %.6f" % worst)
        assert worst <= t2 + 1e-9
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(io.BytesIO(blob))
        assert im.n_frames == F
        for f in range(F):
            im.seek(f)
            assert np.array_equal(np.array(im.convert("RGB")), pal8[composite[f]]), f
