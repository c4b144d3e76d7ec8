"""tests/lzw_ref.py against itself, against independent statements and against PIL (no GPU): the reference encoder of gif_lzw, the
decoder written from the GIF specification, the container parser; and the argument checks of gif_lzw / write_gif that must come
before any library call."""
import io

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import lzw_ref

# every length at which the first width increments fall (m = 2: free reaches 8 after 2 codes, 16, 32, ...), then sparser
LENGTHS = list(range(1, 140)) + [255, 256, 257, 300, 511, 699, 700, 1023, 1500]
SEGMENTS = [7, 50, 64, 350, 8192]
KINDS = ["noise", "one", "ramp"]


def test_decode_inverts_encode():
    for m in (2, 3, 5, 8):
        for kind in KINDS:
            for n in LENGTHS:
                x = lzw_ref.contents(kind, n, m)
                for segment in SEGMENTS:
                    if segment != 8192 and n > 3 * segment and n not in (300, 700):
                        continue
                    stream = lzw_ref.encode(x, m, segment)
                    assert lzw_ref.decode(stream, m, n) == x.tolist(), (m, kind, n, segment)
                    assert len(stream) <= lzw_ref.bound(n, segment)


def test_the_full_dictionary():
    """9216 symbols of noise at m = 8: the dictionary fills (3838 entries) and the encoder emits a Clear that is no segment boundary."""
    x = lzw_ref.contents("noise", 96 * 96, 8)
    codes = []
    stream = lzw_ref.encode(x, 8, 65536, codes)
    clears = [i for i, (c, w) in enumerate(codes) if c == 256]
    assert clears[0] == 0 and len(clears) >= 2 and all(codes[i][1] == 12 for i in clears[1:])
    assert lzw_ref.decode(stream, 8, x.size) == x.tolist()
    assert len(stream) <= lzw_ref.bound(x.size, 65536)
    x2 = lzw_ref.contents("noise", 9000, 2)                     # m = 2 fills it too: 4090 entries of ever longer strings
    codes = []
    stream = lzw_ref.encode(np.tile(x2, 40), 2, 1 << 24, codes)
    assert sum(1 for c, w in codes if c == 4) >= 2
    assert lzw_ref.decode(stream, 2, 40 * 9000) == np.tile(x2, 40).tolist()


def _bits_of(data, nbits):
    v = int.from_bytes(data, "little")
    return v & ((1 << nbits) - 1)


def test_a_segmented_stream_is_its_segments_end_to_end():
    for m, n, segment in ((2, 700, 50), (8, 700, 350), (5, 301, 7), (8, 9000, 4096), (3, 64, 64), (3, 65, 64)):
        x = lzw_ref.contents("noise", n, m)
        whole = lzw_ref.encode(x, m, segment)
        acc, at = 1 << m, m + 1                                  # the opening Clear
        nseg = -(-n // segment)
        for k in range(nseg):
            bw = lzw_ref.BitWriter()
            lzw_ref.encode_segment(bw, x[k * segment:(k + 1) * segment], m, "eoi" if k == nseg - 1 else "clear")
            nb = bw.bits()
            acc |= _bits_of(bw.done(), nb) << at
            at += nb
        assert whole == acc.to_bytes((at + 7) // 8, "little"), (m, n, segment)


def _plain_lzw(x, m):
    """An unsegmented GIF encoder stated the textbook way, on strings: the longest string in the table is emitted, string + next symbol
    is entered; when code 4095 has been used up, a Clear.  The code width is that of the largest code the decoder could see next."""
    clear, eoi = 1 << m, (1 << m) + 1
    bw = lzw_ref.BitWriter()
    table = {(s,): s for s in range(clear)}
    nxt, width = eoi + 1, m + 1
    bw.put(clear, width)
    cur = ()
    for s in [int(v) for v in x]:
        if cur + (s,) in table:
            cur = cur + (s,)
            continue
        bw.put(table[cur], width)
        if nxt <= 4095:
            table[cur + (s,)] = nxt
            nxt += 1
            if nxt - 1 == (1 << width) and width < 12:
                width += 1
        else:
            bw.put(clear, width)
            table = {(v,): v for v in range(clear)}
            nxt, width = eoi + 1, m + 1
        cur = (s,)
    bw.put(table[cur], width)
    if nxt <= 4095 and nxt == (1 << width) and width < 12:     # the decoder enters a string on this code as well
        width += 1
    bw.put(eoi, width)
    return bw.done()


def test_one_segment_beyond_the_frame_is_the_unsegmented_coder():
    for m in (2, 8):
        for kind in KINDS:
            for n in [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 250, 254, 255, 256, 257, 258, 700, 9216]:
                x = lzw_ref.contents(kind, n, m)
                assert lzw_ref.encode(x, m, n + 1) == _plain_lzw(x, m), (m, kind, n)
                assert lzw_ref.encode(x, m, 1 << 24) == lzw_ref.encode(x, m, n)


def test_two_by_two_byte_for_byte():
    """m = 2, the symbols 0 1 0 1: Clear (4) at 3 bits; 0 and 1 are misses, entered as 6 and 7; the third and fourth symbol match entry
    6, the pending prefix, still at 3 bits; the decoder's entry on it is code 8 = 2^3, so the end code (5) takes 4 bits.
    Bits, first code lowest: 100 | 000 << 3 | 001 << 6 | 110 << 9 | 0101 << 12 = 0x5c44."""
    codes = []
    stream = lzw_ref.encode(np.array([[0, 1], [0, 1]]).reshape(-1), 2, codes=codes)
    assert codes == [(4, 3), (0, 3), (1, 3), (6, 3), (5, 4)]
    assert stream == bytes([0x44, 0x5C])
    assert lzw_ref.decode(stream, 2, 4) == [0, 1, 0, 1]
    # a segment per symbol: every symbol between two Clears at 3 bits, the last before the end code
    codes = []
    stream = lzw_ref.encode([3, 2], 2, segment=1, codes=codes)
    assert codes == [(4, 3), (3, 3), (4, 3), (2, 3), (5, 3)]
    assert stream == (4 | 3 << 3 | 4 << 6 | 2 << 9 | 5 << 12).to_bytes(2, "little")


def _grey(rows):
    pal = np.zeros((rows, 3), dtype=np.uint8)
    pal[:, 0] = np.arange(rows)
    pal[:, 1] = 255 - np.arange(rows)
    pal[:, 2] = (np.arange(rows) * 7) % 256
    return pal


def test_pil_decodes_the_segmented_streams():
    Image = pytest.importorskip("PIL.Image")
    cases = [(m, kind, (1, n), segment) for m in (2, 8) for kind in ("noise", "ramp") for n in list(range(1, 70)) + [255, 256, 257, 699]
             for segment in (7, 50, 8192)]
    cases += [(8, "noise", (96, 96), 65536), (8, "noise", (96, 96), 2048), (5, "one", (37, 53), 300), (3, "noise", (263, 301), 8192)]
    for m, kind, (h, w), segment in cases:
        x = lzw_ref.contents(kind, h * w, m).reshape(h, w)
        pal = _grey(1 << m)
        blob = lzw_ref.wrap_gif([lzw_ref.encode(x.reshape(-1), m, segment)], [(0, 0, w, h)], (h, w), pal, m, loop=None)
        im = Image.open(io.BytesIO(blob))
        got = np.array(im.convert("RGB"))
        assert np.array_equal(got, pal[x]), (m, kind, h, w, segment)


def test_parser_and_compositor_on_an_animation():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    h, w, T = 9, 13, 15
    maps = rng.integers(0, 15, size=(4, h, w)).astype(np.uint8)
    rects = [(0, 0, w, h), (2, 3, 5, 4), (0, 0, 1, 1), (12, 8, 1, 1)]
    canvas, shown = maps[0].astype(np.int64), [maps[0].astype(np.int64)]
    deltas = np.full_like(maps, T)
    deltas[0] = maps[0]
    for f in range(1, 4):
        x0, y0, rw, rh = rects[f]
        if f != 2:
            deltas[f, y0:y0 + rh, x0:x0 + rw] = maps[f, y0:y0 + rh, x0:x0 + rw]
            canvas = canvas.copy()
            canvas[y0:y0 + rh, x0:x0 + rw] = maps[f, y0:y0 + rh, x0:x0 + rw]
        shown.append(canvas)
    streams = [lzw_ref.encode(deltas[f, y0:y0 + rh, x0:x0 + rw].reshape(-1), 4, 7) for f, (x0, y0, rw, rh) in enumerate(rects)]
    pal = _grey(16)
    blob = lzw_ref.wrap_gif(streams, rects, (h, w), pal, 4, transparent_index=T, delay_cs=7, loop=3)
    head, frames = lzw_ref.parse_gif(blob)
    assert (head["width"], head["height"], head["loop"]) == (w, h, 3) and np.array_equal(head["table"], pal)
    assert [fr["rect"] for fr in frames] == rects and all(fr["transparent"] == T and fr["delay_cs"] == 7 and fr["disposal"] == 1 for fr in frames)
    assert np.array_equal(lzw_ref.composite(head, frames), np.stack(shown))
    im = Image.open(io.BytesIO(blob))
    assert im.n_frames == 4
    for f in range(4):
        im.seek(f)
        assert np.array_equal(np.array(im.convert("RGB")), pal[shown[f]]), f


def test_value_errors_come_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "lib", no_library)
    maps = np.zeros((2, 5, 7), dtype=np.uint8)
    pal = np.zeros((16, 3), dtype=np.uint8)
    bad_lzw = [
        dict(maps=maps.astype(np.uint16)), dict(maps=maps.astype(np.int64)), dict(maps=np.zeros(5, dtype=np.uint8)),
        dict(maps=np.zeros((1, 2, 5, 7), dtype=np.uint8)), dict(maps=[[1, 2]]),
        dict(rects=np.zeros((3, 4), dtype=np.int32)), dict(rects=np.zeros((2, 3), dtype=np.int32)), dict(rects=np.zeros((2, 4))),
        dict(rects=[[0, 0, 8, 5], [0, 0, 7, 5]]), dict(rects=[[0, 0, 7, 6], [0, 0, 7, 5]]), dict(rects=[[-1, 0, 2, 2], [0, 0, 7, 5]]),
        dict(rects=[[0, 0, 7, 5], [6, 4, 2, 1]]), dict(rects=[[0, 0, 7, 5], [6, 4, 1, 2]]), dict(rects=[[0, 0, 0, 3], [0, 0, 7, 5]]),
        dict(min_code_size=1), dict(min_code_size=9), dict(min_code_size=2.0), dict(min_code_size=True),
        dict(segment=0), dict(segment=-3), dict(segment=2 ** 24 + 1), dict(segment=64.0),
    ]
    for kw in bad_lzw:
        args = dict(maps=maps)
        args.update(kw)
        with pytest.raises(ValueError):
            patolette_amd.gif_lzw(**args)
    bad_gif = [
        dict(palette_u8=np.zeros((257, 3), dtype=np.uint8)), dict(palette_u8=np.zeros((16, 4), dtype=np.uint8)),
        dict(palette_u8=np.zeros((16, 3))), dict(transparent_index=256), dict(transparent_index=-1), dict(transparent_index=1.5),
        dict(maps=maps.astype(np.uint16)), dict(rects=[[0, 0, 8, 5], [0, 0, 7, 5]]), dict(delay=-1.0), dict(delay=[0.1, 0.1, 0.1]),
        dict(delay=float("nan")), dict(delay=700.0), dict(loop=-1), dict(loop=65536), dict(loop=1.5), dict(disposal=4), dict(disposal=-1),
        dict(segment=0), dict(segment=2 ** 24 + 1), dict(maps=np.zeros((0, 5, 7), dtype=np.uint8)),
        dict(maps=np.zeros((1, 0, 7), dtype=np.uint8)),
    ]
    for kw in bad_gif:
        args = dict(file=None, maps=maps, palette_u8=pal)
        args.update(kw)
        with pytest.raises(ValueError):
            patolette_amd.write_gif(**args)
    with pytest.raises(AssertionError, match="the library was called"):        # (and good arguments do reach it)
        patolette_amd.gif_lzw(maps, [[0, 0, 0, 0], [1, 1, 6, 4]], 4, 64)
    assert patolette_amd.gif_lzw_bound([[0, 0, 7, 5], [0, 0, 1, 1]], 8) == lzw_ref.bound(35, 8) + lzw_ref.bound(1, 8)
