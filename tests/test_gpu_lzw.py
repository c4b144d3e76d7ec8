"""gif_lzw / patolette_amd_gif_lzw and write_gif on the device against tests/lzw_ref.py.

`data` and `offsets` are compared bit for bit with the reference encoder, and the device's streams are also decoded by the
independent decoder (which shares no code with the encoder) back to the pixels.  The cases are the smallest at which each part can go
wrong: every ending position relative to the width increments; shapes that are no multiple of 64 symbols, of a segment, of the
kernels' blocks; the contents that make the longest and the shortest matches; the full dictionary; rectangles at every edge."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import delta_ref, lzw_ref
from tests.test_gpu_remap import _palette
from tests.util import ROOT

pytestmark = pytest.mark.gpu

PREFIX = "patolette_amd_gif_lzw:"
SHAPES = {"one": ((1, 1), 1), "tiny": ((5, 3), 1), "odd64": ((37, 53), 3), "thin": ((301, 1), 2), "row": ((1, 301), 1), "square": ((64, 64), 1),
          "tiles": ((263, 301), 2)}
MS = [2, 3, 5, 8]
SEGMENTS = [7, 64, 300, None, 1 << 20]          # None: the default 8192; the last lies beyond every frame here


@pytest.fixture(autouse=True)
def _defaults_again(gpu):
    yield
    _native.profile(False)


@functools.lru_cache(maxsize=None)
def _maps(kind, size, F, m):
    maps = lzw_ref.contents(kind, F * size[0] * size[1], m, seed=F).reshape((F,) + size)
    maps.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def _reference(kind, size, F, m, segment):
    data, offsets = lzw_ref.encode_frames(_maps(kind, size, F, m), None, m, segment or lzw_ref.DEFAULT_SEGMENT)
    data.setflags(write=False)
    offsets.setflags(write=False)
    return data, offsets


def _lzw(*args, **kw):
    ok, data, offsets, msg = patolette_amd.gif_lzw(*args, **kw)
    assert ok, msg
    assert isinstance(data, np.ndarray) and data.dtype == np.uint8 and offsets.dtype == np.int64
    return data, offsets


def _same(got, ref):
    data, offsets = got
    assert np.array_equal(offsets, ref[1]), (offsets.tolist()[-3:], ref[1].tolist()[-3:])
    wrong = int(np.sum(data != ref[0]))
    print("%d of %d bytes differ from the reference" % (wrong, ref[0].size))
    assert wrong == 0


def _decoded(got, maps, rects, m):
    """The device's streams through the independent decoder: the pixels of every rectangle."""
    data, offsets = got
    for f in range(maps.shape[0]):
        x0, y0, w, h = (0, 0, maps.shape[2], maps.shape[1]) if rects is None else (int(v) for v in rects[f])
        sym = lzw_ref.decode(data[offsets[f]:offsets[f + 1]].tobytes(), m, w * h)
        assert sym == maps[f, y0:y0 + h, x0:x0 + w].reshape(-1).tolist(), f


@pytest.mark.parametrize("segment", [50, 350, 8192])
@pytest.mark.parametrize("m", [2, 8])
def test_every_ending_position(gpu, m, segment):
    """ONE call: 700 frames of one row, frame f compressing its first f + 1 symbols -- every place a stream can end at relative to the
    width increments (the entry the decoder makes on the pending prefix)."""
    maps = lzw_ref.contents("noise", 700 * 700, m).reshape(700, 1, 700)
    rects = np.array([(0, 0, f + 1, 1) for f in range(700)], dtype=np.int32)
    got = _lzw(maps, rects, m, segment)
    _same(got, lzw_ref.encode_frames(maps, rects, m, segment))
    _decoded(got, maps, rects, m)


def _cases(name):
    """(kind, m, segment) of a shape: the full cross for the small ones; for the two of 10^5 symbols and more, whose reference takes
    the CPU a tenth of a second and more per stream, every m, every segment and every content at least once."""
    kinds = ["noise", "one", "ramp"]
    if name in ("tiles", "odd64"):
        return [(kinds[(i + j) % 3], m, seg) for i, m in enumerate(MS) for j, seg in enumerate(SEGMENTS) if name == "odd64" or (i + j) % 2 == 0]
    return [(kind, m, seg) for kind in kinds for m in MS for seg in SEGMENTS]


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_contents_and_segments(gpu, name):
    size, F = SHAPES[name]
    for kind, m, segment in _cases(name):
        maps = _maps(kind, size, F, m)
        got = _lzw(maps, None, m, segment)
        _same(got, _reference(kind, size, F, m, segment))
        assert got[0].size <= patolette_amd.gif_lzw_bound([[0, 0, size[1], size[0]]] * F, segment)
        if maps.size <= 8000:
            _decoded(got, maps, None, m)
    one = _lzw(_maps("noise", size, F, 8)[0])                                     # an (H, W) map is one frame; the defaults
    _same(one, lzw_ref.encode_frames(_maps("noise", size, F, 8)[:1]))


@functools.lru_cache(maxsize=None)
def _clip_deltas(size, F, tolerance):
    """(frames, byte palette, deltas, rects, shown) of delta_ref's clip on 16 random rows, ordered maps, T = 255: made on the device by
    the entries test_gpu_ordered.py and test_gpu_delta.py check."""
    frames = delta_ref.clip(size[0], size[1], F)
    pal = _palette(16, seed=2)
    ok, maps, _, msg = patolette_amd.remap(frames, pal, dither="ordered", want_quantized=False)
    assert ok, msg
    ok, deltas, rects, changed, shown, msg = patolette_amd.frame_deltas(maps, pal, transparent_index=255, frames=frames, tolerance=tolerance,
                                                                        want_shown=True)
    assert ok, msg
    for a in (frames, pal, deltas, rects, shown):
        a.setflags(write=False)
    return frames, pal, deltas, rects, shown


def test_the_clips_deltas(gpu):
    """Mostly the transparent index: long matches, with the changed positions scattered in them."""
    for size, F in (((37, 53), 4), ((120, 64), 5)):
        for tolerance in (0.0, 0.05):
            _, _, deltas, rects, _ = _clip_deltas(size, F, tolerance)
            assert np.mean(deltas[1:] == 255) > 0.3
            for use_rects in (None, rects):
                for segment in (300, None):
                    got = _lzw(deltas, use_rects, 8, segment)
                    _same(got, lzw_ref.encode_frames(deltas, use_rects, 8, segment or 8192))
                    _decoded(got, deltas, use_rects, 8)


def test_the_full_dictionary(gpu):
    maps = _maps("noise", (96, 96), 1, 8)
    codes = []
    lzw_ref.encode(maps.reshape(-1), 8, 65536, codes)
    inner = [i for i, (c, w) in enumerate(codes) if c == 256 and i > 0]
    assert inner and all(codes[i][1] == 12 for i in inner)                       # a Clear that is no segment boundary
    got = _lzw(maps, None, 8, 65536)
    _same(got, _reference("noise", (96, 96), 1, 8, 65536))
    _decoded(got, maps, None, 8)
    long2 = np.tile(lzw_ref.contents("noise", 9000, 2), 40).reshape(1, 600, 600)  # m = 2 fills it with ever longer strings
    codes = []
    lzw_ref.encode(long2.reshape(-1), 2, 1 << 24, codes)
    assert sum(1 for c, w in codes if c == 4) >= 2
    _same(_lzw(long2, None, 2, 1 << 24), lzw_ref.encode_frames(long2, None, 2, 1 << 24))


def test_rectangles(gpu):
    h, w = 37, 53
    rects = np.array([(10, 7, 20, 11), (0, 5, 9, 20), (44, 5, 9, 20), (5, 0, 30, 4), (5, 33, 30, 4), (0, 0, w, h), (17, 19, 1, 1), (0, 36, w, 1),
                      (52, 0, 1, h), (0, 0, 1, 1), (52, 36, 1, 1), (3, 2, 47, 33)], dtype=np.int32)
    F = len(rects)
    for m in (3, 8):
        maps = lzw_ref.contents("noise", F * h * w, m, seed=9).reshape(F, h, w)
        for segment in (7, 64, None):
            got = _lzw(maps, rects, m, segment)
            _same(got, lzw_ref.encode_frames(maps, rects, m, segment or 8192))
            _decoded(got, maps, rects, m)
    # an empty rectangle stands for (0, 0, 1, 1)
    empty = rects.copy()
    empty[3] = (0, 0, 0, 0)
    as_one = rects.copy()
    as_one[3] = (0, 0, 1, 1)
    _same(_lzw(maps, empty, 8), lzw_ref.encode_frames(maps, as_one, 8))


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c_call(gpu, maps, rects=None, m=8, segment=0, capacity=None, dims=None, out=True, offsets=True):
    """patolette_amd_gif_lzw itself.  Returns (code, out array, offsets array)."""
    F, h, w = dims if dims is not None else maps.shape
    r = None if rects is None else np.ascontiguousarray(rects, dtype=np.int32)
    if capacity is None:                                                          # (the full frames' bound holds any rectangles')
        capacity = patolette_amd.gif_lzw_bound([[0, 0, maps.shape[2], maps.shape[1]]] * maps.shape[0], segment if 1 <= segment <= 1 << 24 else None)
    buf = np.full(capacity, 0xAA, dtype=np.uint8)
    off = np.full(maps.shape[0] + 1, 77, dtype=np.uint64)
    code = C.c_int(7)
    gpu.patolette_amd_gif_lzw(F, w, h, _vp(maps), None if r is None else r.ctypes.data_as(C.POINTER(C.c_int32)), m, segment,
                              _vp(buf) if out and capacity else None, capacity, off.ctypes.data_as(C.POINTER(C.c_uint64)) if offsets else None,
                              C.byref(code))
    return code.value, buf, off


def test_elements_outside_the_rectangles_and_the_flag(gpu):
    h, w, m = 37, 53, 3
    maps = lzw_ref.contents("noise", 2 * h * w, m).reshape(2, h, w).copy()
    rects = np.array([(10, 7, 20, 11), (1, 1, 51, 35)], dtype=np.int32)
    ref = lzw_ref.encode_frames(maps, rects, m, 64)
    outside = maps.copy()
    outside[0, :7] = 255
    outside[0, 7:18, :10] = 8
    outside[0, 7:18, 30:] = 200
    outside[0, 18:] = 9
    outside[1, 0], outside[1, 36], outside[1, :, 0], outside[1, :, 52] = 8, 255, 77, 8
    _same(_lzw(outside, rects, m, 64), ref)                                       # not read: no flag, the same streams
    for f, y, x, v in ((0, 7, 10, 8), (0, 17, 29, 255), (1, 35, 51, 8), (1, 20, 20, 9)):
        bad = maps.copy()
        bad[f, y, x] = v
        code, _, _ = _c_call(gpu, bad, rects, m, 64)
        assert code == -1
        text = _native.last_error()
        assert text.startswith(PREFIX) and "min_code_size" in text, text
        with pytest.raises(ValueError, match="min_code_size"):
            patolette_amd.gif_lzw(bad, rects, m, 64)
        _same(_lzw(maps, rects, m, 64), ref)                                      # the next call works


def test_capacity(gpu):
    maps = _maps("noise", (37, 53), 3, 5)
    ref = _reference("noise", (37, 53), 3, 5, 300)
    need = int(ref[1][-1])
    code, buf, off = _c_call(gpu, maps, None, 5, 300, capacity=need)
    assert code == 0 and np.array_equal(buf, ref[0]) and np.array_equal(off.astype(np.int64), ref[1])
    code, buf, off = _c_call(gpu, maps, None, 5, 300, capacity=need - 1)
    assert code == -1 and _native.last_error().startswith(PREFIX) and "capacity" in _native.last_error()
    assert int(off[3]) == need and np.array_equal(off.astype(np.int64), ref[1]) and np.all(buf == 0xAA)     # nothing copied
    code, buf, off = _c_call(gpu, maps, None, 5, 300, capacity=0)
    assert code == -1 and int(off[3]) == need
    code, buf, off = _c_call(gpu, maps, None, 5, 300, capacity=need + 5)
    assert code == 0 and np.array_equal(buf[:need], ref[0]) and np.all(buf[need:] == 0xAA)


def test_failures_and_recovery(gpu):
    size, F, m = (40, 56), 2, 5
    h, w = size
    maps = _maps("ramp", size, F, m)
    ref = _reference("ramp", size, F, m, None)

    def good():
        code, buf, off = _c_call(gpu, maps, None, m)
        assert code == 0 and np.array_equal(off.astype(np.int64), ref[1]) and np.array_equal(buf[:int(off[-1])], ref[0])

    def failed(result, *words):
        assert result[0] == -1
        text = _native.last_error()
        assert text.startswith(PREFIX) and all(word in text for word in words), text
        good()

    good()
    failed(_c_call(gpu, maps, None, 1), "min_code_size")
    failed(_c_call(gpu, maps, None, 9), "min_code_size")
    failed(_c_call(gpu, maps, None, m, (1 << 24) + 1), "segment")
    failed(_c_call(gpu, maps, None, m, offsets=False), "offsets")
    failed(_c_call(gpu, maps, None, m, out=False), "no out")
    full = [0, 0, w, h]
    for rect in ([0, 0, 0, 0], [0, 0, w + 1, h], [0, 0, w, h + 1], [-1, 0, 3, 3], [0, -1, 3, 3], [w - 2, 0, 3, 3], [0, h - 2, 3, 3], [5, 5, 0, 3],
                 [5, 5, 3, 0], [5, 5, -2, 3]):
        failed(_c_call(gpu, maps, [full, rect], m), "rectangle")
        failed(_c_call(gpu, maps, [rect, full], m), "rectangle")
    code = C.c_int(7)
    off = np.zeros(F + 1, dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint8)
    gpu.patolette_amd_gif_lzw(F, w, h, None, None, m, 0, _vp(buf), 64, off.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(code))
    failed((code.value,), "no maps")
    bad = maps.copy()
    bad[1, 39, 55] = 32
    failed(_c_call(gpu, bad, None, m), "min_code_size")
    # -2 and -4
    assert _c_call(gpu, maps, None, m, dims=(0, h, w))[0] == -2
    assert _c_call(gpu, maps, None, m, dims=(F, 0, w))[0] == -2
    assert _c_call(gpu, maps, None, m, dims=(F, h, 0))[0] == -2
    good()
    assert _c_call(gpu, maps, None, m, dims=(1 << 31, h, w))[0] == -4 and _native.last_error().startswith(PREFIX) and "too big" in _native.last_error()
    assert _c_call(gpu, maps, None, m, dims=(1, 50000, 50000))[0] == -4
    good()
    ok, data, offsets, msg = patolette_amd.gif_lzw(np.zeros((0, 5, 7), dtype=np.uint8))
    assert not ok and data is None and offsets is None and msg == "Image dimensions should be greater than 0."


def _bits(got):
    return got[0].tobytes(), got[1].tolist()


def test_a_function_of_the_arguments_alone(gpu):
    """The workspace rules: the same bits on a second call, after a larger call, after another entry's call, after the workspace is released."""
    size, F = SHAPES["tiles"]
    maps = _maps("noise", size, F, 5)
    rects = np.array([(3, 2, 290, 250), (0, 0, 301, 263)], dtype=np.int32)
    for segment in (300, None):
        first = _bits(_lzw(maps, rects, 5, segment))
        assert _bits(_lzw(maps, rects, 5, segment)) == first
        big = lzw_ref.contents("noise", 512 * 600, 8).reshape(512, 600)
        _lzw(big, None, 8, 100)                                                   # more segments, a longer staging area, more output
        ok, *_ = patolette_amd.remap(np.zeros((64, 64, 3), dtype=np.uint8), _palette(16), dither=False)
        assert ok
        assert _bits(_lzw(maps, rects, 5, segment)) == first
        gpu.patolette_amd_release_workspace()
        assert _bits(_lzw(maps, rects, 5, segment)) == first
    _same(_lzw(maps, rects, 5, None), lzw_ref.encode_frames(maps, rects, 5))


def test_torch_flavour(gpu):
    """Torch CUDA tensors go through patolette_amd_gif_lzw_device: the numpy flavour's bytes.  Own process: torch loads its HIP runtime
    before libpatolette_amd.so does."""
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
from tests import lzw_ref
for (F, h, w), m, segment in (((3, 37, 53), 8, None), ((2, 263, 301), 5, 300), ((1, 1, 1), 2, None), ((2, 301, 1), 3, 7)):
    maps = lzw_ref.contents("noise", F * h * w, m).reshape(F, h, w)
    rects = np.array([(0, 0, w, h)] * (F - 1) + [(w // 3, h // 3, w - w // 3, h - h // 3)], dtype=np.int32)
    t = torch.from_numpy(maps).cuda()
    for r in (None, rects):
        ok, data, off, msg = p.gif_lzw(maps, r, m, segment)
        assert ok, msg
        ok, data_t, off_t, msg = p.gif_lzw(t, r, m, segment)
        assert ok, msg
        assert isinstance(data_t, np.ndarray) and isinstance(off_t, np.ndarray)
        assert np.array_equal(off_t, off) and np.array_equal(data_t, data)
        ref = lzw_ref.encode_frames(maps, r, m, segment or 8192)
        assert np.array_equal(off_t, ref[1]) and np.array_equal(data_t, ref[0])
    ok, d1, o1, msg = p.gif_lzw(t[0], None, m, segment)                    # one map
    ok0, d0, o0, _ = p.gif_lzw(maps[0], None, m, segment)
    assert ok and ok0 and np.array_equal(d1, d0) and np.array_equal(o1, o0)
    view = t.transpose(1, 2).contiguous().transpose(1, 2)                  # the same values, not contiguous: made so
    ok, dv, ov, msg = p.gif_lzw(view, None, m, segment)
    ok2, dn, on, _ = p.gif_lzw(maps, None, m, segment)
    assert ok and ok2 and np.array_equal(dv, dn) and np.array_equal(ov, on)
    blob_t = p.write_gif(None, t, np.zeros((1 << m, 3), dtype=np.uint8), rects)
    assert blob_t == p.write_gif(None, maps, np.zeros((1 << m, 3), dtype=np.uint8), rects)
try:
    p.gif_lzw(t.to(torch.int32))
    raise SystemExit("int32 tensor maps were accepted")
except ValueError:
    pass
print("TORCH-LZW-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-LZW-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_last_stats_and_the_kernels(gpu):
    size, F = SHAPES["tiles"]
    maps = _maps("noise", size, F, 8)
    for segment in (300, None):
        _native.profile(True)
        _lzw(maps, None, 8, segment)
        prof = _native.profile_results()
        _native.profile(False)
        assert all(prof[k]["launches"] == 1 for k in ("k_lzw_segments", "k_lzw_offsets", "k_lzw_pack"))      # one launch each, all frames
        assert {k for k in prof if prof[k]["launches"]} == {"k_lzw_segments", "k_lzw_offsets", "k_lzw_pack"}
        st = patolette_amd.last_stats()
        assert st["ms_total"] > 0 and st["ms_map"] > 0 and st["ms_upload"] > 0 and st["ms_total"] >= st["ms_map"]
        assert all(st[key] == 0 for key in st if not key.startswith("ms_"))
        assert st["ms_convert"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0 and st["ms_kmeans"] == 0 and st["ms_saliency"] == 0


@pytest.mark.parametrize("size,F", [((37, 53), 8), ((120, 64), 6)])
def test_end_to_end(gpu, size, F, tmp_path):
    """quantize_frames(.., 255, dither="ordered") -> frame_deltas -> write_gif: the file, parsed, decoded by the independent decoder and
    composited frame by frame, is `shown`; PIL, where it is installed, sees the same frames as RGB."""
    frames = delta_ref.clip(size[0], size[1], F)
    ok, pal8, maps, _, _, msg = patolette_amd.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2, want_quantized=False)
    assert ok and maps.dtype == np.uint8 and pal8.shape == (255, 3), msg
    for tolerance in (0.0, 0.05):
        ok, deltas, rects, changed, shown, msg = patolette_amd.frame_deltas(maps, pal8, transparent_index=255, frames=frames, tolerance=tolerance,
                                                                            want_shown=True)
        assert ok, msg
        if tolerance == 0.0:
            assert np.array_equal(shown, maps)
        path = tmp_path / ("clip_%g.gif" % tolerance)
        blob = patolette_amd.write_gif(path, deltas, pal8, rects, transparent_index=255, delay=[0.03 + 0.01 * f for f in range(F)], loop=2)
        assert path.read_bytes() == blob
        sink = io.BytesIO()
        assert patolette_amd.write_gif(sink, deltas, pal8, rects, transparent_index=255, delay=[0.03 + 0.01 * f for f in range(F)], loop=2) == blob
        assert sink.getvalue() == blob
        head, parsed = lzw_ref.parse_gif(blob)
        assert (head["width"], head["height"], head["loop"]) == (size[1], size[0], 2)
        assert head["table"].shape == (256, 3) and np.array_equal(head["table"][:255], pal8) and not head["table"][255].any()
        assert len(parsed) == F and all(fr["m"] == 8 and fr["transparent"] == 255 and fr["disposal"] == 1 for fr in parsed)
        assert [fr["delay_cs"] for fr in parsed] == [3 + f for f in range(F)]
        want = [tuple(int(v) for v in r) if r[2] else (0, 0, 1, 1) for r in rects]
        assert [fr["rect"] for fr in parsed] == want
        data, offsets = _lzw(deltas, rects)
        assert [fr["stream"] for fr in parsed] == [data[offsets[f]:offsets[f + 1]].tobytes() for f in range(F)]
        assert np.array_equal(lzw_ref.composite(head, parsed), shown.astype(np.int64))
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(io.BytesIO(blob))
        assert im.n_frames == F
        for f in range(F):
            im.seek(f)
            assert np.array_equal(np.array(im.convert("RGB")), pal8[shown[f]]), f
    # a palette of 16 rows and no transparency: 4 bits; of 3 rows with index 5 transparent: 3 bits
    small = (maps % 16).astype(np.uint8)
    head, parsed = lzw_ref.parse_gif(patolette_amd.write_gif(None, small, pal8[:16], loop=None, disposal=0, segment=64))
    assert head["table"].shape == (16, 3) and head["loop"] is None and parsed[0]["m"] == 4 and parsed[0]["transparent"] is None
    assert np.array_equal(lzw_ref.composite(head, parsed), small.astype(np.int64))
    head, parsed = lzw_ref.parse_gif(patolette_amd.write_gif(None, (maps % 3).astype(np.uint8)[0], pal8[:3], transparent_index=5))
    assert head["table"].shape == (8, 3) and parsed[0]["m"] == 3 and parsed[0]["transparent"] == 5 and len(parsed) == 1
    head, parsed = lzw_ref.parse_gif(patolette_amd.write_gif(None, (maps % 2).astype(np.uint8), pal8[:2]))
    assert head["table"].shape == (2, 3) and parsed[0]["m"] == 2
    assert np.array_equal(lzw_ref.composite(head, parsed), (maps % 2).astype(np.int64))
