"""write_png / write_apng, png_deflate's arguments and csrc/deflate_codes.h without a GPU.

The containers are written with `png_deflate` replaced by the zlib stand-in of tests/png_ref.py and read back by that file's parser
(every CRC, every sequence number) and compositor, and by PIL where it is installed.  The code tables are checked by a stand-alone
program under the sanitizers, whose blocks zlib then inflates."""
import ctypes as C
import io
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import lzw_ref, png_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def standin(monkeypatch):
    calls = []

    def fake(maps, rects=None, segment=None):
        calls.append((np.asarray(maps).shape, None if rects is None else np.asarray(rects).copy(), segment))
        return png_ref.zlib_png_deflate(maps, rects, segment)

    monkeypatch.setattr(patolette_amd, "png_deflate", fake)
    return calls


def _map(h=37, w=53, k=16, seed=0):
    return np.random.default_rng(seed).integers(0, k, size=(h, w)).astype(np.uint8)


def _pal(k, seed=1, channels=3):
    return np.random.default_rng(seed).integers(0, 256, size=(k, channels)).astype(np.uint8)


def _same_rgba(got, want):
    """Equal alpha everywhere and equal colour wherever something shows (a viewer's colour under alpha 0 is its own business)."""
    return np.array_equal(got[..., 3], want[..., 3]) and np.array_equal(got[..., :3][want[..., 3] > 0], want[..., :3][want[..., 3] > 0])


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


# ---------------------------------------------------------------- write_png
def test_write_png_fields_and_pixels(standin, tmp_path):
    m, pal = _map(), _pal(16)
    path = tmp_path / "a.png"
    blob = patolette_amd.write_png(path, m, pal, segment=300)
    assert path.read_bytes() == blob and standin[-1][2] == 300 and standin[-1][1] is None
    sink = io.BytesIO()
    assert patolette_amd.write_png(sink, m, pal, segment=300) == blob and sink.getvalue() == blob
    assert [k for k, _ in png_ref.chunks(blob)] == [b"IHDR", b"PLTE", b"IDAT", b"IEND"]
    head, frames = png_ref.parse(blob)
    assert (head["width"], head["height"], head["num_plays"]) == (53, 37, None) and len(frames) == 1
    assert np.array_equal(head["palette"], pal) and np.all(head["alpha"] == 255)
    assert frames[0]["stream"][:2] == b"\x78\x9c" and np.array_equal(frames[0]["indices"], m)
    Image = _pil()
    if Image is not None:
        im = Image.open(io.BytesIO(blob))
        assert im.mode == "P" and im.size == (53, 37) and np.array_equal(np.array(im), m)
        assert np.array_equal(np.array(im.convert("RGB")), pal[m])


def test_write_png_palettes_and_transparency(standin):
    m = _map(k=5)
    # (K, 4): tRNS from the alpha column, cut behind the last entry that is not opaque
    pal4 = _pal(5, channels=4)
    pal4[:, 3] = (255, 0, 255, 128, 255)
    blob = patolette_amd.write_png(None, m, pal4)
    cs = dict(png_ref.chunks(blob))
    assert cs[b"tRNS"] == bytes([255, 0, 255, 128]) and cs[b"PLTE"] == pal4[:, :3].tobytes()
    head, frames = png_ref.parse(blob)
    assert np.array_equal(head["alpha"], pal4[:, 3]) and np.array_equal(frames[0]["indices"], m)
    Image = _pil()
    if Image is not None:
        assert np.array_equal(np.array(Image.open(io.BytesIO(blob)).convert("RGBA")), pal4[m])
    # every entry opaque: no tRNS
    pal4[:, 3] = 255
    assert b"tRNS" not in dict(png_ref.chunks(patolette_amd.write_png(None, m, pal4)))
    # (K, 3) with a transparent index inside the palette
    pal3 = _pal(5)
    head, _ = png_ref.parse(patolette_amd.write_png(None, m, pal3, transparent_index=2))
    assert head["alpha"].tolist() == [255, 255, 0, 255, 255] and np.array_equal(head["palette"], pal3)
    # ... and at or beyond K: PLTE is padded with zero rows up to it
    for t in (5, 9, 255):
        blob = patolette_amd.write_png(None, m, pal3, transparent_index=t)
        head, frames = png_ref.parse(blob)
        assert head["palette"].shape == (t + 1, 3) and np.array_equal(head["palette"][:5], pal3) and not head["palette"][5:].any()
        assert head["alpha"].tolist() == [255] * t + [0] and dict(png_ref.chunks(blob))[b"tRNS"] == bytes([255] * t + [0])
    # (K, 4) and a transparent index on top of its alpha column
    pal4[:, 3] = (255, 255, 7, 255, 255)
    head, _ = png_ref.parse(patolette_amd.write_png(None, m, pal4, transparent_index=0))
    assert head["alpha"].tolist() == [0, 255, 7, 255, 255]
    # a 256-row palette and a 1 x 1 map
    one = np.array([[255]], dtype=np.uint8)
    head, frames = png_ref.parse(patolette_amd.write_png(None, one, _pal(256)))
    assert head["palette"].shape == (256, 3) and frames[0]["indices"].tolist() == [[255]]


# ---------------------------------------------------------------- write_apng
def _deltas(F=6, h=37, w=53, t=255, seed=3):
    """Maps, and deltas against the frame before with `t` where nothing changes, their dirty rectangles (frame 3 unchanged: empty)."""
    rng = np.random.default_rng(seed)
    maps = np.empty((F, h, w), dtype=np.uint8)
    maps[0] = rng.integers(0, 16, size=(h, w))
    for f in range(1, F):
        maps[f] = maps[f - 1]
        if f != 3:
            y0, x0 = int(rng.integers(0, h - 9)), int(rng.integers(0, w - 11))
            maps[f, y0:y0 + 9, x0:x0 + 11] = rng.integers(0, 16, size=(9, 11))
    deltas, rects = maps.copy(), np.zeros((F, 4), dtype=np.int32)
    rects[0] = (0, 0, w, h)
    for f in range(1, F):
        changed = maps[f] != maps[f - 1]
        deltas[f] = np.where(changed, maps[f], t)
        if changed.any():
            ys, xs = np.nonzero(changed)
            rects[f] = (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
    return maps, deltas, rects


def test_write_apng_fields_and_composite(standin, tmp_path):
    maps, deltas, rects = _deltas()
    F, h, w = maps.shape
    pal = _pal(16)
    delays = [0.03 + 0.01 * f for f in range(F)]
    path = tmp_path / "a.png"
    blob = patolette_amd.write_apng(path, deltas, pal, rects, transparent_index=255, delay=delays, loop=3, segment=64)
    assert path.read_bytes() == blob and standin[-1][2] == 64
    kinds = [k for k, _ in png_ref.chunks(blob)]
    assert kinds == [b"IHDR", b"acTL", b"PLTE", b"tRNS", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (F - 1) + [b"IEND"]
    head, frames = png_ref.parse(blob)                                            # (checks the sequence numbers 0 .. 2F - 2)
    assert (head["width"], head["height"], head["num_frames"], head["num_plays"]) == (w, h, F, 3)
    assert head["palette"].shape == (256, 3) and head["alpha"][255] == 0 and np.all(head["alpha"][:255] == 255)
    assert [fr["sequence"] for fr in frames] == [0] + [2 * f - 1 for f in range(1, F)]
    assert [fr["data_sequences"] for fr in frames] == [[]] + [[2 * f] for f in range(1, F)]
    assert [(fr["delay_num"], fr["delay_den"]) for fr in frames] == [(3 + f, 100) for f in range(F)]
    assert all(fr["dispose_op"] == png_ref.DISPOSE_NONE and fr["blend_op"] == png_ref.BLEND_OVER for fr in frames)
    want = [tuple(int(v) for v in r) if r[2] else (0, 0, 1, 1) for r in rects]
    assert [fr["rect"] for fr in frames] == want and want[3] == (0, 0, 1, 1)
    for f, fr in enumerate(frames):
        x0, y0, rw, rh = fr["rect"]
        assert np.array_equal(fr["indices"], deltas[f, y0:y0 + rh, x0:x0 + rw])
    # the canvas a GIF of the same deltas shows
    data, offsets = lzw_ref.encode_frames(deltas, np.array(want, dtype=np.int32), 8, 8192)
    table = np.zeros((256, 3), dtype=np.uint8)
    table[:16] = pal
    gif = lzw_ref.wrap_gif([data[offsets[f]:offsets[f + 1]].tobytes() for f in range(F)], want, (h, w), table, 8, transparent_index=255)
    shown = lzw_ref.composite(*lzw_ref.parse_gif(gif))
    assert np.array_equal(shown, maps.astype(np.int64))
    assert np.array_equal(png_ref.composite_indices(head, frames), shown)
    rgba = png_ref.composite(head, frames)
    assert np.all(rgba[..., 3] == 255) and np.array_equal(rgba[..., :3], pal[maps])
    Image = _pil()
    if Image is not None:
        im = Image.open(io.BytesIO(blob))
        assert im.n_frames == F and im.info.get("loop") == 3
        for f in range(F):
            im.seek(f)
            assert np.array_equal(np.array(im.convert("RGBA")), rgba[f]), f


def test_write_apng_frame_0_is_the_full_frame(standin):
    maps, deltas, rects = _deltas()
    F, h, w = maps.shape
    small = rects.copy()
    small[0] = (5, 4, 20, 10)
    blob = patolette_amd.write_apng(None, deltas, _pal(16), small, transparent_index=255)
    passed = small.copy()
    passed[0], passed[3] = (0, 0, w, h), (0, 0, 1, 1)                              # frame 0 full; the empty rectangle as (0, 0, 1, 1)
    assert np.array_equal(standin[-1][1], passed)
    head, frames = png_ref.parse(blob)
    assert frames[0]["rect"] == (0, 0, w, h) and np.array_equal(frames[0]["indices"], deltas[0])
    assert blob == patolette_amd.write_apng(None, deltas, _pal(16), rects, transparent_index=255)
    # no rectangles: every frame full; one (H, W) map: one frame
    head, frames = png_ref.parse(patolette_amd.write_apng(None, maps, _pal(16)))
    assert all(fr["rect"] == (0, 0, w, h) for fr in frames) and all(fr["blend_op"] == png_ref.BLEND_SOURCE for fr in frames)
    assert np.array_equal(png_ref.composite(head, frames)[..., :3], _pal(16)[maps])
    head, frames = png_ref.parse(patolette_amd.write_apng(None, maps[0], _pal(16), loop=0))
    assert head["num_frames"] == 1 and head["num_plays"] == 0 and len(frames) == 1 and frames[0]["data_sequences"] == []


def test_write_apng_disposal_and_blend(standin):
    """GIF's disposal numbers: 0 and 1 NONE, 2 BACKGROUND, 3 PREVIOUS; blend OVER with a transparent index, else SOURCE.  Sprites that
    move over a transparent background, every frame disposed to background: the composite is each frame's own sprite."""
    F, h, w = 5, 20, 24
    pal = _pal(4, channels=4)
    pal[:, 3] = (0, 255, 255, 255)
    maps = np.zeros((F, h, w), dtype=np.uint8)
    rects = np.zeros((F, 4), dtype=np.int32)
    rects[0] = (0, 0, w, h)
    for f in range(F):
        maps[f, 2 + f:8 + f, 3 * f:3 * f + 6] = 1 + f % 3
        if f:
            rects[f] = (3 * f, 2 + f, 6, 6)
    disposal = [2, 2, 3, 1, 0]
    blob = patolette_amd.write_apng(None, maps, pal, rects, transparent_index=0, disposal=disposal, delay=0.5)
    head, frames = png_ref.parse(blob)
    assert [fr["dispose_op"] for fr in frames] == [1, 1, 2, 0, 0] and all(fr["blend_op"] == png_ref.BLEND_OVER for fr in frames)
    assert all((fr["delay_num"], fr["delay_den"]) == (50, 100) for fr in frames)
    idx = png_ref.composite_indices(head, frames)
    want = np.where(maps == 0, -1, maps.astype(np.int64))
    assert np.array_equal(idx[:4], want[:4])                                       # background, background, previous: each sprite alone
    assert np.array_equal(idx[4], np.where(want[4] >= 0, want[4], want[3]))        # frame 3 was left in place
    rgba = png_ref.composite(head, frames)
    Image = _pil()
    if Image is not None:
        im = Image.open(io.BytesIO(blob))
        for f in range(F):
            im.seek(f)
            assert _same_rgba(np.array(im.convert("RGBA")), rgba[f]), f
    for d in (0, 1, 2, 3):
        _, frames = png_ref.parse(patolette_amd.write_apng(None, maps, pal, rects, disposal=d))
        assert all(fr["dispose_op"] == (0, 0, 1, 2)[d] for fr in frames)
        assert all(fr["blend_op"] == png_ref.BLEND_SOURCE for fr in frames)       # no transparent index


# ---------------------------------------------------------------- arguments, before any library call
def test_every_value_error_comes_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_native, "lib", no_library)
    m, pal = _map(), _pal(16)
    bad_maps = (np.zeros((4, 4), dtype=np.uint16), np.zeros((4, 4), dtype=np.float32), np.zeros(7, dtype=np.uint8), np.zeros((1, 2, 3, 4), dtype=np.uint8), [[1, 2]])
    for maps in bad_maps:
        with pytest.raises(ValueError):
            patolette_amd.png_deflate(maps)
        with pytest.raises(ValueError):
            patolette_amd.write_png(None, maps, pal)
        with pytest.raises(ValueError):
            patolette_amd.write_apng(None, maps, pal)
    for segment in (0, -1, 32769, 1.5, True, "8192"):
        with pytest.raises(ValueError, match="segment"):
            patolette_amd.png_deflate(m, None, segment)
        with pytest.raises(ValueError, match="segment"):
            patolette_amd.write_png(None, m, pal, segment=segment)
        with pytest.raises(ValueError, match="segment"):
            patolette_amd.write_apng(None, m, pal, segment=segment)
        with pytest.raises(ValueError, match="segment"):
            patolette_amd.png_deflate_bound([[0, 0, 5, 5]], segment)
    for rects in ([[0, 0, 54, 37]], [[0, 0, 53, 38]], [[-1, 0, 3, 3]], [[0, 0, 0, 3]], [[0, 0, 3, 3], [0, 0, 3, 3]], [[0.0, 0.0, 3.0, 3.0]], [0, 0, 3, 3]):
        with pytest.raises(ValueError, match="rect"):
            patolette_amd.png_deflate(m, rects)
    with pytest.raises(ValueError, match="rect"):
        patolette_amd.write_apng(None, np.stack([m, m]), pal, [[0, 0, 53, 37], [50, 0, 4, 4]])
    with pytest.raises(ValueError, match="map"):
        patolette_amd.write_png(None, np.stack([m, m]), pal)                       # one map only
    for palette in (np.zeros((4, 2), dtype=np.uint8), np.zeros((4, 5), dtype=np.uint8), np.zeros((4, 3), dtype=np.float64), np.zeros((0, 3), dtype=np.uint8),
                    np.zeros((257, 3), dtype=np.uint8), np.zeros(12, dtype=np.uint8)):
        with pytest.raises(ValueError, match="palette"):
            patolette_amd.write_png(None, m, palette)
        with pytest.raises(ValueError, match="palette"):
            patolette_amd.write_apng(None, m, palette)
    for t in (-1, 256, 1.0, True):
        with pytest.raises(ValueError, match="transparent_index"):
            patolette_amd.write_png(None, m, pal, transparent_index=t)
        with pytest.raises(ValueError, match="transparent_index"):
            patolette_amd.write_apng(None, m, pal, transparent_index=t)
    for delay in (-0.1, float("nan"), 700.0, [0.1, 0.2]):
        with pytest.raises(ValueError, match="delay"):
            patolette_amd.write_apng(None, m, pal, delay=delay)
    for loop in (-1, 1.5, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="loop"):
            patolette_amd.write_apng(None, m, pal, loop=loop)
    for disposal in (4, -1, 1.0, True, [1, 1], [5]):
        with pytest.raises(ValueError, match="disposal"):
            patolette_amd.write_apng(None, m, pal, disposal=disposal)


def test_the_bound():
    """9 bits a filtered byte and 10 a segment, per frame rounded up to bytes: at most 9/8 of the filtered bytes, a constant per segment
    and a constant per frame."""
    rects = np.array([(0, 0, 53, 37), (3, 2, 1, 1), (0, 0, 640, 360)], dtype=np.int32)
    for segment, seg in ((None, 16384), (7, 7), (300, 300), (32768, 32768)):
        total = 0
        for x0, y0, w, h in rects.tolist():
            flen = h * (w + 1)
            nseg = -(-flen // seg)
            total += -(-(9 * flen + 10 * nseg) // 8)
            assert -(-(9 * flen + 10 * nseg) // 8) <= 9 * flen / 8 + 2 * nseg + 1
        assert patolette_amd.png_deflate_bound(rects, segment) == total


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(HERE, "..", "include", "patolette_amd.h")).read()
    for name in ("patolette_amd_png_deflate", "patolette_amd_png_deflate_device"):
        assert "void %s(" % name in header and name in _native.SYMBOLS
        restype, argtypes = _native.SYMBOLS[name]
        assert restype is None and len(argtypes) == 11 and argtypes[-1] == C.POINTER(C.c_int) and argtypes[-2] == C.POINTER(C.c_uint32)
    assert "int patolette_amd_debug_deflate_block(" in header                      # host code only: tests/test_deflate_model.py calls it
    restype, argtypes = _native.SYMBOLS["patolette_amd_debug_deflate_block"]
    assert restype is C.c_int and len(argtypes) == 6 and argtypes[-1] == C.POINTER(C.c_uint64)
    assert hasattr(_native.lib(), "patolette_amd_debug_deflate_block")
    for name in ("png_deflate", "png_deflate_bound", "write_png", "write_apng"):
        assert name in patolette_amd.__all__ and callable(getattr(patolette_amd, name))
    assert "deflate.hip" in open(os.path.join(HERE, "..", "patolette_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------- the stand-in and the reader themselves
def test_the_reader_rejects_what_is_wrong(standin):
    blob = patolette_amd.write_apng(None, np.stack([_map(), _map(seed=5)]), _pal(16))
    png_ref.parse(blob)
    broken = bytearray(blob)
    broken[40] ^= 1                                                               # inside acTL: its CRC no longer holds
    with pytest.raises(AssertionError, match="CRC"):
        png_ref.chunks(bytes(broken))
    at = blob.index(b"fdAT") + 4                                                  # a wrong sequence number, CRC mended
    n = int.from_bytes(blob[at - 8:at - 4], "big")
    body = b"\x00\x00\x00\x07" + blob[at + 4:at + n]
    mended = blob[:at] + body + zlib.crc32(b"fdAT" + body).to_bytes(4, "big") + blob[at + n + 4:]
    with pytest.raises(AssertionError, match="sequence"):
        png_ref.parse(mended)
    ok, data, offsets, adler, _ = png_ref.zlib_png_deflate(_map(), None)
    png_ref.check_streams(_map(), None, data, offsets, adler)
    with pytest.raises(AssertionError):
        png_ref.check_streams(_map(seed=9), None, data, offsets, adler)


# ---------------------------------------------------------------- csrc/deflate_codes.h
def test_the_code_tables_hold_under_sanitizers(tmp_path):
    """tests/deflate_codes_check.cpp: code lengths within the limits, Kraft sums of exactly 1, Huffman's cost wherever its tree fits;
    then the blocks the host function wrote for those histograms, inflated by zlib behind the program's preset dictionary."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "deflate_codes_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(HERE, "..", "patolette_amd", "csrc"), os.path.join(HERE, "deflate_codes_check.cpp"), "-o", exe], check=True)
    out = tmp_path / "blocks"
    out.mkdir()
    run = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "histograms and run-length cases checked" in run.stdout
    preset = bytes((i * 7 + i // 251) & 255 for i in range(32768))
    names = sorted(p[:-8] for p in os.listdir(out) if p.endswith(".deflate"))
    assert len(names) >= 25 and {"one_literal", "two_literals", "all_equal", "no_distance", "one_distance_0", "fibonacci", "flat_lengths"} <= set(names)
    for name in names:
        d = zlib.decompressobj(-15, zdict=preset)
        got = d.decompress((out / (name + ".deflate")).read_bytes()) + d.flush()
        assert d.eof and not d.unused_data, name
        assert got == (out / (name + ".expect")).read_bytes(), name
