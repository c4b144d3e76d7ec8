"""png_deflate / patolette_amd_png_deflate, write_png and write_apng on the device.

The oracle is an independent decoder, not a model of the coder: zlib inflates every stream back to the filtered stream byte for byte
(tests/png_ref.py: check_streams), tests/png_ref.py reads the files, PIL opens them.  The cases are the smallest at which each part can
go wrong: streams that end at every bit position, shapes that are no multiple of 64 positions, of a segment, of a row; one byte; the
contents with the longest and with no matches; rectangles at every edge; segments shorter than a row and the largest."""
import ctypes as C
import functools
import io
import zlib

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import delta_ref, lzw_ref, png_ref
from tests.test_gpu_remap import _palette
from tests.util import ROOT

pytestmark = pytest.mark.gpu

PREFIX = "patolette_amd_png_deflate:"
SHAPES = {"one": ((1, 1), 1), "tiny": ((5, 3), 1), "odd64": ((37, 53), 3), "thin": ((301, 1), 2), "row": ((1, 301), 1), "square": ((64, 64), 1),
          "tiles": ((263, 301), 2)}
SEGMENTS = [7, 64, 300, None, 32768]            # None: the default 16384; the last is the largest


@pytest.fixture(autouse=True)
def _defaults_again(gpu):
    yield
    _native.profile(False)


@functools.lru_cache(maxsize=None)
def _maps(kind, size, F, m):
    maps = lzw_ref.contents(kind, F * size[0] * size[1], m, seed=F).reshape((F,) + size)
    maps.setflags(write=False)
    return maps


def _full(maps):
    return [[0, 0, maps.shape[-1], maps.shape[-2]]] * (maps.shape[0] if maps.ndim == 3 else 1)


def _deflate(maps, rects=None, segment=None):
    ok, data, offsets, adler, msg = patolette_amd.png_deflate(maps, rects, segment)
    assert ok, msg
    assert isinstance(data, np.ndarray) and data.dtype == np.uint8 and offsets.dtype == np.int64 and adler.dtype == np.uint32
    png_ref.check_streams(maps, rects, data, offsets, adler)
    return data, offsets, adler


def _bits(got):
    return got[0].tobytes(), got[1].tolist(), got[2].tolist()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_contents_and_segments(gpu, name):
    size, F = SHAPES[name]
    for kind in ("noise", "one", "ramp"):
        for m in (2, 8):
            maps = _maps(kind, size, F, m)
            for segment in SEGMENTS:
                data, offsets, adler = _deflate(maps, None, segment)
                assert data.size <= patolette_amd.png_deflate_bound(_full(maps), segment), (kind, m, segment)
    one = _deflate(_maps("noise", size, F, 8)[0])                                 # an (H, W) map is one frame; the defaults
    assert _bits(one) == _bits(_deflate(_maps("noise", size, F, 8)[:1]))


def test_every_ending_position(gpu):
    """ONE call: 300 frames of one row, frame f coding its first f + 1 elements: streams of every length, ending at every bit."""
    maps = lzw_ref.contents("noise", 300 * 300, 3).reshape(300, 1, 300)
    rects = np.array([(0, 0, f + 1, 1) for f in range(300)], dtype=np.int32)
    for segment in (50, None):
        data, offsets, adler = _deflate(maps, rects, segment)
        assert data.size <= patolette_amd.png_deflate_bound(rects, segment)


def test_rectangles(gpu):
    h, w = 37, 53
    rects = np.array([(10, 7, 20, 11), (0, 5, 9, 20), (44, 5, 9, 20), (5, 0, 30, 4), (5, 33, 30, 4), (0, 0, w, h), (17, 19, 1, 1), (0, 36, w, 1),
                      (52, 0, 1, h), (0, 0, 1, 1), (52, 36, 1, 1), (3, 2, 47, 33)], dtype=np.int32)
    F = len(rects)
    for m in (3, 8):
        maps = lzw_ref.contents("noise", F * h * w, m, seed=9).reshape(F, h, w)
        for segment in (7, 64, None):
            data, offsets, adler = _deflate(maps, rects, segment)
            assert data.size <= patolette_amd.png_deflate_bound(rects, segment)
    # an empty rectangle stands for (0, 0, 1, 1)
    empty = rects.copy()
    empty[3] = (0, 0, 0, 0)
    as_one = rects.copy()
    as_one[3] = (0, 0, 1, 1)
    assert _bits(_deflate(maps, empty)) == _bits(_deflate(maps, as_one))


def test_elements_outside_the_rectangles_are_not_read(gpu):
    h, w = 37, 53
    maps = lzw_ref.contents("noise", 2 * h * w, 3).reshape(2, h, w).copy()
    rects = np.array([(10, 7, 20, 11), (1, 1, 51, 35)], dtype=np.int32)
    ref = _bits(_deflate(maps, rects, 64))
    outside = maps.copy()
    outside[0, :7] = 255
    outside[0, 7:18, :10] = 8
    outside[0, 7:18, 30:] = 200
    outside[0, 18:] = 9
    outside[1, 0], outside[1, 36], outside[1, :, 0], outside[1, :, 52] = 8, 255, 77, 8
    got = patolette_amd.png_deflate(outside, rects, 64)
    assert got[0] and (got[1].tobytes(), got[2].tolist(), got[3].tolist()) == ref
    inside = maps.copy()
    inside[0, 17, 29] ^= 1                                                        # the rectangle's last element is read
    assert _bits(_deflate(inside, rects, 64)) != ref


# ---------------------------------------------------------------- sizes
H, W = 360, 640


@functools.lru_cache(maxsize=None)
def _size_maps():
    y, x = np.mgrid[0:H, 0:W]
    g = 0.7 * x / W + 0.3 * y / H
    b2 = np.array([[0, 2], [3, 1]])
    b4 = np.block([[4 * b2, 4 * b2 + 2], [4 * b2 + 3, 4 * b2 + 1]])
    b8 = np.block([[4 * b4, 4 * b4 + 2], [4 * b4 + 3, 4 * b4 + 1]])
    t = (np.tile(b8, (H // 8, W // 8)) + 0.5) / 64.0 - 0.5                        # the 8 x 8 Bayer threshold in (-0.5, 0.5)
    rng = np.random.default_rng(0)
    delta = np.full((H, W), 255, dtype=np.uint8)
    mask = rng.random((H, W)) < 0.03
    delta[mask] = rng.integers(0, 200, size=int(mask.sum()))
    return {
        "ordered16": np.floor(15 * g + t + 0.5).astype(np.uint8),
        "ordered200": np.floor(199 * g + t + 0.5).astype(np.uint8),
        "poster": ((x // 40 + y // 30) % 7).astype(np.uint8),
        "delta": delta,
        "noise256": np.random.default_rng(1).integers(0, 256, size=(H, W)).astype(np.uint8),
        "flat": np.full((H, W), 5, dtype=np.uint8),
    }


# bytes / zlib level 6's bytes of the same filtered stream at the default segment, as measured; the test allows 2 % more,
# for another zlib build: the coder itself is deterministic
MEASURED = {"ordered16": 1.0207, "ordered200": 1.1115, "poster": 1.0293, "delta": 1.0834, "noise256": 1.0021}


@pytest.mark.parametrize("name", list(MEASURED))
def test_sizes_against_zlib(gpu, name):
    m = _size_maps()[name]
    data, offsets, adler = _deflate(m)
    level6 = zlib.compressobj(6, zlib.DEFLATED, -15)
    ref = len(level6.compress(png_ref.filtered(m)) + level6.flush())
    print("%s: %d bytes, zlib level 6 %d bytes, ratio %.4f (measured %.4f)" % (name, data.size, ref, data.size / ref, MEASURED[name]))
    assert data.size <= patolette_amd.png_deflate_bound(_full(m))
    assert data.size / ref <= MEASURED[name] * 1.02


def test_sizes_that_hold_whatever_the_measurement(gpu):
    maps = _size_maps()
    filtered = H * (W + 1)
    data, _, _ = _deflate(maps["noise256"])
    assert data.size <= patolette_amd.png_deflate_bound(_full(maps["noise256"]))
    data, _, _ = _deflate(maps["flat"])
    print("flat: %d bytes of %d" % (data.size, filtered))
    assert data.size < 0.02 * filtered                                            # 258 bytes cost at most 26 bits even under the fixed code
    rows = np.tile(np.random.default_rng(2).integers(0, 256, size=(1, 300)).astype(np.uint8), (64, 1))
    data, _, _ = _deflate(rows, None, 300)
    print("equal rows, segment 300: %d bytes of %d" % (data.size, 64 * 301))
    assert data.size < 0.25 * 64 * 301                                            # only matches that start before the segment can do that


# ---------------------------------------------------------------- determinism and flavours
def test_a_function_of_the_arguments_alone(gpu):
    """The workspace rules: the same bits on a second call, after a larger call, after another entry's call, after the workspace is released."""
    size, F = SHAPES["tiles"]
    maps = _maps("noise", size, F, 5)
    rects = np.array([(3, 2, 290, 250), (0, 0, 301, 263)], dtype=np.int32)
    for segment in (300, None):
        first = _bits(_deflate(maps, rects, segment))
        assert _bits(_deflate(maps, rects, segment)) == first
        big = lzw_ref.contents("ramp", 512 * 600, 8).reshape(512, 600)
        _deflate(big, None, 100)                                                  # more segments, a longer staging area, more output
        ok, *_ = patolette_amd.remap(np.zeros((64, 64, 3), dtype=np.uint8), _palette(16), dither=False)
        assert ok
        ok, *_ = patolette_amd.gif_lzw(maps, rects, 5, segment)                   # the entry that shares the staging areas
        assert ok
        assert _bits(_deflate(maps, rects, segment)) == first
        gpu.patolette_amd_release_workspace()
        assert _bits(_deflate(maps, rects, segment)) == first


def test_a_frame_alone_has_its_bytes_of_the_batch(gpu):
    size, F = SHAPES["odd64"]
    ordered = _size_maps()["ordered16"][:size[0] * 2, :size[1] * 2]
    for maps in (_maps("noise", size, F, 3), _maps("ramp", size, F, 8), np.stack([ordered[:37, :53], ordered[37:, 53:], ordered[20:57, 30:83]])):
        rects = np.array([(0, 0, 53, 37), (5, 4, 40, 30), (52, 36, 1, 1)], dtype=np.int32)
        for use in (None, rects):
            for segment in (64, None):
                data, offsets, adler = _deflate(maps, use, segment)
                for f in range(F):
                    d1, o1, a1 = _deflate(maps[f:f + 1], None if use is None else use[f:f + 1], segment)
                    assert d1.tobytes() == data[offsets[f]:offsets[f + 1]].tobytes() and a1[0] == adler[f], (f, segment)


def test_torch_flavour(gpu):
    """Torch CUDA tensors go through patolette_amd_png_deflate_device: the numpy flavour's bytes.  Own process: torch loads its HIP
    runtime before libpatolette_amd.so does."""
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
from tests import lzw_ref, png_ref
for (F, h, w), m, segment in (((3, 37, 53), 8, None), ((2, 263, 301), 5, 300), ((1, 1, 1), 2, None), ((2, 301, 1), 3, 7)):
    maps = lzw_ref.contents("noise", F * h * w, m).reshape(F, h, w)
    rects = np.array([(0, 0, w, h)] * (F - 1) + [(w // 3, h // 3, w - w // 3, h - h // 3)], dtype=np.int32)
    t = torch.from_numpy(maps).cuda()
    for r in (None, rects):
        ok, data, off, adler, msg = p.png_deflate(maps, r, segment)
        assert ok, msg
        ok, data_t, off_t, adler_t, msg = p.png_deflate(t, r, segment)
        assert ok, msg
        assert isinstance(data_t, np.ndarray) and isinstance(off_t, np.ndarray) and isinstance(adler_t, np.ndarray)
        assert np.array_equal(off_t, off) and np.array_equal(data_t, data) and np.array_equal(adler_t, adler)
        png_ref.check_streams(maps, r, data_t, off_t, adler_t)
    ok, d1, o1, a1, msg = p.png_deflate(t[0], None, segment)                 # one map
    ok0, d0, o0, a0, _ = p.png_deflate(maps[0], None, segment)
    assert ok and ok0 and np.array_equal(d1, d0) and np.array_equal(o1, o0) and np.array_equal(a1, a0)
    view = t.transpose(1, 2).contiguous().transpose(1, 2)                  # the same values, not contiguous: made so
    ok, dv, ov, av, msg = p.png_deflate(view, None, segment)
    ok2, dn, on, an, _ = p.png_deflate(maps, None, segment)
    assert ok and ok2 and np.array_equal(dv, dn) and np.array_equal(ov, on) and np.array_equal(av, an)
    pal = np.arange(3 << m, dtype=np.uint8).reshape(1 << m, 3)
    assert p.write_apng(None, t, pal, rects) == p.write_apng(None, maps, pal, rects)
    assert p.write_png(None, t[0], pal) == p.write_png(None, maps[0], pal)
try:
    p.png_deflate(t.to(torch.int32))
    raise SystemExit("int32 tensor maps were accepted")
except ValueError:
    pass
print("TORCH-PNG-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-PNG-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c_call(gpu, maps, rects=None, segment=0, capacity=None, dims=None, out=True, offsets=True, adler=True):
    """patolette_amd_png_deflate itself.  Returns (code, out array, offsets array, adler array)."""
    F, h, w = dims if dims is not None else maps.shape
    r = None if rects is None else np.ascontiguousarray(rects, dtype=np.int32)
    if capacity is None:                                                          # (the full frames' bound holds any rectangles')
        capacity = patolette_amd.png_deflate_bound(_full(maps), segment if 1 <= segment <= 32768 else None)
    buf = np.full(capacity, 0xAA, dtype=np.uint8)
    off = np.full(maps.shape[0] + 1, 77, dtype=np.uint64)
    adl = np.full(maps.shape[0], 77, dtype=np.uint32)
    code = C.c_int(7)
    gpu.patolette_amd_png_deflate(F, w, h, _vp(maps), None if r is None else r.ctypes.data_as(C.POINTER(C.c_int32)), segment,
                                  _vp(buf) if out and capacity else None, capacity, off.ctypes.data_as(C.POINTER(C.c_uint64)) if offsets else None,
                                  adl.ctypes.data_as(C.POINTER(C.c_uint32)) if adler else None, C.byref(code))
    return code.value, buf, off, adl


def test_capacity(gpu):
    maps = _maps("noise", (37, 53), 3, 5)
    data, offsets, adler = _deflate(maps, None, 300)
    need = int(offsets[-1])
    code, buf, off, adl = _c_call(gpu, maps, None, 300, capacity=need)
    assert code == 0 and np.array_equal(buf, data) and np.array_equal(off.astype(np.int64), offsets) and np.array_equal(adl, adler)
    code, buf, off, adl = _c_call(gpu, maps, None, 300, capacity=need - 1)
    assert code == -1 and _native.last_error().startswith(PREFIX) and "capacity" in _native.last_error()
    assert int(off[3]) == need and np.array_equal(off.astype(np.int64), offsets) and np.all(buf == 0xAA)     # nothing copied
    code, buf, off, adl = _c_call(gpu, maps, None, 300, capacity=0)
    assert code == -1 and int(off[3]) == need
    code, buf, off, adl = _c_call(gpu, maps, None, 300, capacity=need + 5)
    assert code == 0 and np.array_equal(buf[:need], data) and np.all(buf[need:] == 0xAA)


def test_failures_and_recovery(gpu):
    size, F = (40, 56), 2
    h, w = size
    maps = _maps("ramp", size, F, 5)
    ref = _deflate(maps)

    def good():
        code, buf, off, adl = _c_call(gpu, maps)
        assert code == 0 and np.array_equal(off.astype(np.int64), ref[1]) and np.array_equal(buf[:int(off[-1])], ref[0]) and np.array_equal(adl, ref[2])

    def failed(result, *words):
        assert result[0] == -1
        text = _native.last_error()
        assert text.startswith(PREFIX) and all(word in text for word in words), text
        good()

    good()
    failed(_c_call(gpu, maps, None, 32769), "segment")
    failed(_c_call(gpu, maps, None, 1 << 24), "segment")
    failed(_c_call(gpu, maps, offsets=False), "offsets")
    failed(_c_call(gpu, maps, adler=False), "adler")
    failed(_c_call(gpu, maps, out=False), "no out")
    full = [0, 0, w, h]
    for rect in ([0, 0, 0, 0], [0, 0, w + 1, h], [0, 0, w, h + 1], [-1, 0, 3, 3], [0, -1, 3, 3], [w - 2, 0, 3, 3], [0, h - 2, 3, 3], [5, 5, 0, 3],
                 [5, 5, 3, 0], [5, 5, -2, 3]):
        failed(_c_call(gpu, maps, [full, rect]), "rectangle")
        failed(_c_call(gpu, maps, [rect, full]), "rectangle")
    code = C.c_int(7)
    off = np.zeros(F + 1, dtype=np.uint64)
    adl = np.zeros(F, dtype=np.uint32)
    buf = np.zeros(64, dtype=np.uint8)
    gpu.patolette_amd_png_deflate(F, w, h, None, None, 0, _vp(buf), 64, off.ctypes.data_as(C.POINTER(C.c_uint64)), adl.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  C.byref(code))
    failed((code.value,), "no maps")
    # -2 and -4
    assert _c_call(gpu, maps, dims=(0, h, w))[0] == -2
    assert _c_call(gpu, maps, dims=(F, 0, w))[0] == -2
    assert _c_call(gpu, maps, dims=(F, h, 0))[0] == -2
    good()
    assert _c_call(gpu, maps, dims=(1 << 31, h, w))[0] == -4 and _native.last_error().startswith(PREFIX) and "too big" in _native.last_error()
    assert _c_call(gpu, maps, dims=(1, 50000, 50000))[0] == -4
    good()
    ok, data, offsets, adler, msg = patolette_amd.png_deflate(np.zeros((0, 5, 7), dtype=np.uint8))
    assert not ok and data is None and offsets is None and adler is None and msg == "Image dimensions should be greater than 0."


def test_last_stats_and_the_kernels(gpu):
    size, F = SHAPES["tiles"]
    maps = _maps("noise", size, F, 8)
    kernels = {"k_png_filter", "k_deflate_segments", "k_lzw_offsets", "k_lzw_pack"}
    for segment in (300, None):
        _native.profile(True)
        _deflate(maps, None, segment)
        prof = _native.profile_results()
        _native.profile(False)
        assert all(prof[k]["launches"] == 1 for k in kernels)                                                 # one launch each, all frames
        assert {k for k in prof if prof[k]["launches"]} == kernels
        st = patolette_amd.last_stats()
        assert st["ms_total"] > 0 and st["ms_map"] > 0 and st["ms_upload"] > 0 and st["ms_total"] >= st["ms_map"]
        assert all(st[key] == 0 for key in st if not key.startswith("ms_"))
        assert st["ms_convert"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0 and st["ms_kmeans"] == 0 and st["ms_saliency"] == 0


# ---------------------------------------------------------------- end to end
def _same_rgba(got, want):
    """Equal alpha everywhere and equal colour wherever something shows."""
    return np.array_equal(got[..., 3], want[..., 3]) and np.array_equal(got[..., :3][want[..., 3] > 0], want[..., :3][want[..., 3] > 0])


def test_quantize_u8_to_write_png(gpu, tmp_path):
    frames = delta_ref.clip(120, 64, 1)
    ok, pal8, pmap, _, _, msg = patolette_amd.quantize_u8(frames[0], 64, dither=True, tile_size=0, kmeans_niter=2, want_quantized=False)
    assert ok and pmap.dtype == np.uint8, msg
    path = tmp_path / "image.png"
    blob = patolette_amd.write_png(path, pmap, pal8)
    assert path.read_bytes() == blob
    head, parsed = png_ref.parse(blob)
    assert np.array_equal(head["palette"], pal8) and np.array_equal(parsed[0]["indices"], pmap)
    data, offsets, adler = _deflate(pmap)
    assert parsed[0]["stream"] == b"\x78\x9c" + data.tobytes() + int(adler[0]).to_bytes(4, "big")
    try:
        from PIL import Image
    except ImportError:
        return
    im = Image.open(io.BytesIO(blob))
    assert im.mode == "P" and np.array_equal(np.array(im), pmap) and np.array_equal(np.array(im.convert("RGB")), pal8[pmap])


@pytest.mark.parametrize("size,F", [((37, 53), 8), ((120, 64), 6)])
def test_rgba_frames_to_write_apng(gpu, size, F, tmp_path):
    """quantize_rgba_frames(.., dither="ordered") -> frame_deltas_rgba -> write_apng with its disposals: the reader's compositor and PIL
    show palette_rgba[shown] for every frame."""
    frames = delta_ref.clip(size[0], size[1], F)
    yy, xx = np.mgrid[0:size[0], 0:size[1]]
    alpha = np.stack([np.where((yy - size[0] / 2 - 2 * f) ** 2 + (xx - size[1] / 2 + f) ** 2 < (min(size) / 2.5) ** 2, 255, 0) for f in range(F)])
    rgba = np.concatenate([frames, alpha[..., None].astype(np.uint8)], axis=3)
    ok, pal_rgba, maps, _, _, tindex, msg = patolette_amd.quantize_rgba_frames(rgba, 64, dither="ordered", tile_size=0, kmeans_niter=2, want_quantized=False)
    assert ok and tindex == 0 and maps.dtype == np.uint8, msg
    for tolerance in (0.0, 0.05):
        ok, deltas, rects, disposals, changed, shown, msg = patolette_amd.frame_deltas_rgba(maps, pal_rgba, frames=rgba, tolerance=tolerance, want_shown=True)
        assert ok, msg
        path = tmp_path / ("clip_%g.png" % tolerance)
        blob = patolette_amd.write_apng(path, deltas, pal_rgba, rects, transparent_index=0, disposal=disposals, delay=0.05, loop=2)
        assert path.read_bytes() == blob
        head, parsed = png_ref.parse(blob)
        assert (head["width"], head["height"], head["num_frames"], head["num_plays"]) == (size[1], size[0], F, 2)
        assert [fr["dispose_op"] for fr in parsed] == [(0, 0, 1, 2)[int(d)] for d in disposals]
        assert all(fr["blend_op"] == png_ref.BLEND_OVER for fr in parsed)
        want = pal_rgba[shown]
        assert _same_rgba(png_ref.composite(head, parsed), want)
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(io.BytesIO(blob))
        assert im.n_frames == F
        for f in range(F):
            im.seek(f)
            assert _same_rgba(np.array(im.convert("RGBA")), want[f]), f


@pytest.mark.parametrize("size,F", [((37, 53), 8), ((120, 64), 6)])
def test_frames_to_write_apng(gpu, size, F):
    """quantize_frames(.., 255, dither="ordered") -> frame_deltas -> write_apng(transparent_index=255): likewise."""
    frames = delta_ref.clip(size[0], size[1], F)
    ok, pal8, maps, _, _, msg = patolette_amd.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2, want_quantized=False)
    assert ok and maps.dtype == np.uint8 and pal8.shape == (255, 3), msg
    for tolerance in (0.0, 0.05):
        ok, deltas, rects, changed, shown, msg = patolette_amd.frame_deltas(maps, pal8, transparent_index=255, frames=frames, tolerance=tolerance,
                                                                            want_shown=True)
        assert ok, msg
        blob = patolette_amd.write_apng(None, deltas, pal8, rects, transparent_index=255, delay=[0.03 + 0.01 * f for f in range(F)])
        head, parsed = png_ref.parse(blob)
        assert head["palette"].shape == (256, 3) and np.array_equal(head["palette"][:255], pal8) and head["alpha"].tolist() == [255] * 255 + [0]
        assert [fr["rect"] for fr in parsed] == [(0, 0, size[1], size[0])] + [tuple(int(v) for v in r) if r[2] else (0, 0, 1, 1) for r in rects[1:]]
        assert np.array_equal(png_ref.composite_indices(head, parsed), shown.astype(np.int64))
        rgba = png_ref.composite(head, parsed)
        assert np.all(rgba[..., 3] == 255) and np.array_equal(rgba[..., :3], pal8[shown])
        data, offsets, adler = _deflate(deltas, np.concatenate([[[0, 0, size[1], size[0]]], rects[1:]]).astype(np.int32))
        assert [fr["stream"] for fr in parsed] == [b"\x78\x9c" + data[offsets[f]:offsets[f + 1]].tobytes() + int(adler[f]).to_bytes(4, "big") for f in range(F)]
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(io.BytesIO(blob))
        assert im.n_frames == F
        for f in range(F):
            im.seek(f)
            assert np.array_equal(np.array(im.convert("RGB")), pal8[shown[f]]), f
