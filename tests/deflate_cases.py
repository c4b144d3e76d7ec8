"""The inputs of tests/test_gpu_png_tokens.py, and the model's results for them (tests/deflate_model.py), computed once per process.

A case is (maps (F, H, W) uint8, rects (F, 4) or None, the segments to run it at; None: the default).  tests/test_deflate_model.py
asserts, without a GPU, that the MODEL reaches every edge the cases were built for and that every single-rule mutation of the model
changes the tokens of at least one of them; the GPU test then holds the device to the model on exactly these inputs."""
import functools

import numpy as np

from tests import deflate_model, png_ref

DEFAULT_SEGMENT = 16384


def _noise(seed, shape, top=256):
    return np.random.default_rng(seed).integers(0, top, size=shape).astype(np.uint8)


def _rows_with_period(seed, w, period_rows, h):
    """h rows of w noise elements that repeat after period_rows rows"""
    return np.tile(_noise(seed, (period_rows, w)), (-(-h // period_rows), 1))[:h]


def _candidates_map():
    """Width 40 (R = 41), noise at 8 bits; from row 8 on, five elements at a time repeat what lies R - 1, R + 1, 2R, 4R, 8R back, in
    turn, with a different element on either side: matches too short for an exploration to keep, at one candidate distance alone."""
    w, R = 40, 41
    a = _noise(21, (30, w))
    flat = png_ref.filtered(a)
    s = np.frombuffer(flat, dtype=np.uint8).copy()
    turn = 0
    for y in range(8, 30):
        for x in (4, 17, 30):
            d = (R - 1, R + 1, 2 * R, 4 * R, 8 * R)[turn % 5]
            turn += 1
            p = y * R + 1 + x
            s[p:p + 5] = s[p - d:p - d + 5]
            for q in (p - 1, p + 5):
                if s[q] == s[q - d]:
                    s[q] ^= 1
    return s.reshape(30, R)[:, 1:].copy()[None]


def _far_three_map(w):
    """Noise at 8 bits; every 29th element from row 8 on starts three elements that repeat the ones 8 rows up: three-byte matches at
    8R and nothing longer."""
    a = _noise(31 + w, (12, w))
    for y in range(8, 12):
        for x in range(5 + y, w - 4, 29):
            a[y, x:x + 3] = a[y - 8, x:x + 3]
            if a[y, x + 3] == a[y - 8, x + 3]:
                a[y, x + 3] ^= 1
            if a[y, x - 1] == a[y - 8, x - 1]:
                a[y, x - 1] ^= 1
    return a[None]


def _mix(seed, size, distances, copy=(70, 400), fresh=(70, 900), top=256):
    """Fresh noise and copies of what lies one of `distances` back, in turns: what an exploration finds, loses and finds again."""
    rng = np.random.default_rng(seed)
    out = list(_noise(seed + 1, (max(distances),), top))
    while len(out) < size:
        out += list(rng.integers(0, top, size=int(rng.integers(*fresh))).astype(np.uint8))
        d = int(distances[int(rng.integers(0, len(distances)))])
        for _ in range(int(rng.integers(*copy))):
            out.append(out[-d])
    return np.array(out[:size], dtype=np.uint8)


def _words(seed, size, nwords, top=256):
    """Words of 4 .. 11 noise elements in random order: repeats at distances only a hash table finds."""
    rng = np.random.default_rng(seed)
    words = [rng.integers(0, top, size=int(rng.integers(4, 12))).astype(np.uint8) for _ in range(nwords)]
    out = []
    while len(out) < size:
        out += list(words[int(rng.integers(0, nwords))])
    return np.array(out[:size], dtype=np.uint8)


def _bayer(h, w, levels):
    y, x = np.mgrid[0:h, 0:w]
    g = 0.7 * x / w + 0.3 * y / h
    b2 = np.array([[0, 2], [3, 1]])
    b4 = np.block([[4 * b2, 4 * b2 + 2], [4 * b2 + 3, 4 * b2 + 1]])
    b8 = np.block([[4 * b4, 4 * b4 + 2], [4 * b4 + 3, 4 * b4 + 1]])
    t = (np.tile(b8, (-(-h // 8), -(-w // 8)))[:h, :w] + 0.5) / 64.0 - 0.5
    return np.floor((levels - 1) * g + t + 0.5).astype(np.uint8)


def _fibonacci_map():
    """Two rows.  The first is noise in 17 .. 255.  The second repeats it but for every fifth element, which takes the values 1 .. 14
    in counts 2, 3, 5, 8, ... 987, shuffled: at a segment of one row the second row's tokens are these literals, each followed by a
    match of four bytes a row up, the row's zero byte and the end of block -- a literal/length histogram 1, 1, 2, 3, 5, ... 987, 2581
    whose Huffman tree is a chain 16 deep whichever way its ties go.  (Three bytes of a record that repeat an earlier one give a
    match at the literal, and the lazy step takes it back: the four-byte match behind it is longer.)"""
    rng = np.random.default_rng(81)
    counts = [2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987]
    literals = np.repeat(np.arange(1, len(counts) + 1), counts).astype(np.uint8)
    rng.shuffle(literals)
    pool = rng.integers(17, 256, size=5 * literals.size).astype(np.uint8)
    records = pool.copy().reshape(-1, 5)
    records[:, 0] = literals
    return np.stack([pool, records.reshape(-1)])[None]


def _widths():
    """One call, seven frames: rectangles 1, 2, 3, 6, 7, 8 and 9 wide of two-valued noise, where R - 1, R and R + 1 meet 1, 2, 4, 8."""
    maps = _noise(41, (7, 90, 9), 2)
    rects = np.array([(0, 0, w, 90) for w in (1, 2, 3, 6, 7, 8, 9)], dtype=np.int32)
    return maps, rects


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (maps, rects, segments)"""
    equal_rows = np.tile(_noise(5, (1, 300)), (8, 1))[None]
    equal_rows[0, 3, 192] ^= 1                                          # filtered byte 1096: at segment 100 a three-byte match ends segment 10
    equal_rows[0, 4, 92] ^= 1                                           # 1297: the last two bytes of segment 12 repeat a row up, as literals
    widths, width_rects = _widths()
    flat = np.zeros((1, 20, 99), dtype=np.uint8)
    explore = _mix(61, 40 * 600, (1500, 2311, 3007, 4500, 5003)).reshape(1, 40, 600)
    words = np.concatenate([_words(71, 6000, 60), np.tile(_noise(72, (150,)), 3), _words(71, 3000, 60), _words(73, 2431, 400)])
    out = {
        "noise8": (_noise(1, (2, 37, 53)), None, (7, 64, None)),
        "lengths": (_noise(2, (1, 5, 12), 2), None, (1, 2, 3, 63, 64, 65)),
        "flat": (flat, None, (1, 700, None)),
        "window32768": (_rows_with_period(3, 255, 128, 148)[None], None, (32768, None)),
        "window32769": (_rows_with_period(4, 330, 99, 114)[None], None, (32768, None)),
        "equal_rows": (equal_rows, None, (100,)),
        "three_frames": (np.concatenate([equal_rows] * 3), None, (100, None)),
        "widths": (widths, width_rects, (50, None)),
        "candidates": (_candidates_map(), None, (32, None)),
        "far3_at_4096": (_far_three_map(511), None, (None,)),
        "far3_beyond": (_far_three_map(599), None, (None,)),
        "explore": (explore, None, (2048, None)),
        "words": (words.reshape(1, 109, 109), None, (None, 3000)),
        "two_valued": (_noise(6, (1, 60, 200), 2), None, (None,)),
        "bayer": (_bayer(24, 96, 16)[None], None, (None,)),
        "fibonacci": (_fibonacci_map(), None, (12906,)),
        "endings": (_noise(7, (40, 1, 40), 256), np.array([(0, 0, f + 1, 1) for f in range(40)], dtype=np.int32), (13,)),
    }
    for maps, _, _ in out.values():
        maps.setflags(write=False)
    return out


def frames_of(name):
    """[(filtered stream, row bytes)] of a case's frames"""
    maps, rects, _ = cases()[name]
    out = []
    for f in range(maps.shape[0]):
        rows = png_ref.rect_rows(maps, rects, f)
        out.append((png_ref.filtered(rows), rows.shape[1] + 1))
    return out


@functools.lru_cache(maxsize=None)
def model(name, segment, mutation=None):
    """[(tokens per segment, traces per segment)] of a case's frames at a segment (None: the default)"""
    seg = DEFAULT_SEGMENT if segment is None else segment
    return [deflate_model.model_tokens(stream, R, seg, mutation) for stream, R in frames_of(name)]


def runs():
    """every (case, segment) the GPU test runs"""
    return [(name, segment) for name, (_, _, segments) in cases().items() for segment in segments]
