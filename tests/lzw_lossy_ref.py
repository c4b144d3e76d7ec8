"""Reference of gif_lzw_lossy / patolette_amd_gif_lzw_lossy and of gif_neighbours, in plain Python / numpy (test infrastructure).

`encode_lossy` is the normative statement of the lossy coder of include/patolette_amd.h: everything of tests/lzw_ref.py's `encode`
(segments, the opening Clear, the width rule, the closing code, the Clear of a full dictionary) with ONE change, the step: when the
pair (prefix, symbol) is not in the dictionary, the symbol's candidates near[s][1 .. near[s][0]] are tried in their order, and the first
one whose pair IS in the dictionary continues the match in the symbol's place.  Only when none is does the old miss run, and it enters
the TRUE symbol.  The first symbol of a segment is taken as it is.  Besides the bytes it returns `coded`, the symbols the stream
decodes to.

`neighbours` builds the table from a palette: per used row the other used rows within `tolerance` in ICtCp (tests/color_ref.py), the D
of the frame_deltas contract, by (D, index), cut to `max_neighbours`."""
import numpy as np

from tests import color_ref, lzw_ref

DEFAULT_SEGMENT = lzw_ref.DEFAULT_SEGMENT


def empty_table():
    return np.zeros((256, 16), dtype=np.uint8)


def pairing_table(m=8):
    """Row s lists s ^ 1."""
    near = empty_table()
    for s in range(1 << m):
        near[s, 0], near[s, 1] = 1, s ^ 1
    return near


def dense_table(m=8, seed=5):
    """15 candidates per row, drawn below 2^m: duplicates and the symbol itself occur (both are allowed)."""
    near = empty_table()
    rng = np.random.default_rng(seed + m)
    near[:1 << m, 0] = 15
    near[:1 << m, 1:] = rng.integers(0, 1 << m, size=(1 << m, 15))
    return near


def counts_table(m=8, seed=7):
    """Row s has s % 16 candidates: every count 0 .. 15 (from m = 4 on)."""
    near = empty_table()
    rng = np.random.default_rng(seed + m)
    for s in range(1 << m):
        near[s, 0] = s % 16
        near[s, 1:1 + s % 16] = rng.integers(0, 1 << m, size=s % 16)
    return near


def encode_segment_lossy(bw, symbols, m, closing, near, coded, codes=None):
    """One segment into `bw` (lzw_ref.encode_segment with the lossy step); `coded`: a list that receives the symbol coded at each step."""
    clear, eoi = 1 << m, (1 << m) + 1

    def put(code, width):
        bw.put(code, width)
        if codes is not None:
            codes.append((code, width))

    table, free, width = {}, eoi + 1, m + 1
    prefix = int(symbols[0])
    assert 0 <= prefix < clear
    coded.append(prefix)
    for s in symbols[1:]:
        s = int(s)
        assert 0 <= s < clear
        count = int(near[s][0])
        assert count <= 15
        for c in [s] + [int(v) for v in near[s][1:1 + count]]:
            assert 0 <= c < clear
            hit = table.get((prefix, c))
            if hit is not None:
                prefix = hit
                coded.append(c)
                break
        else:
            put(prefix, width)
            if free < 4096:
                table[(prefix, s)] = free
                if free == (1 << width) and width < 12:
                    width += 1
                free += 1
            else:
                put(clear, width)
                table, free, width = {}, eoi + 1, m + 1
            prefix = s
            coded.append(s)
    put(prefix, width)
    if free < 4096 and free == (1 << width) and width < 12:
        width += 1
    put(clear if closing == "clear" else eoi, width)


def encode_lossy(symbols, m, near, segment=DEFAULT_SEGMENT, codes=None):
    """The stream of one frame and what it decodes to: (bytes, coded uint8 array of symbols' length)."""
    symbols = np.asarray(symbols).reshape(-1)
    near = np.asarray(near)
    assert symbols.size >= 1 and 2 <= m <= 8 and segment >= 1 and near.shape == (256, 16)
    bw = lzw_ref.BitWriter()
    bw.put(1 << m, m + 1)
    if codes is not None:
        codes.append((1 << m, m + 1))
    rows = [[int(v) for v in row] for row in near]                 # (plain lists: the loop above indexes them a lot)
    coded = []
    nseg = -(-symbols.size // segment)
    for k in range(nseg):
        encode_segment_lossy(bw, symbols[k * segment:(k + 1) * segment].tolist(), m, "eoi" if k == nseg - 1 else "clear", rows, coded, codes)
    return bw.done(), np.array(coded, dtype=np.uint8)


def encode_frames_lossy(maps, near, rects=None, m=8, segment=DEFAULT_SEGMENT):
    """What gif_lzw_lossy returns for (F, H, W) maps: (data uint8, offsets (F + 1,) int64, coded: a copy of maps overwritten inside
    the rectangles).  rects as lzw_ref.encode_frames takes them."""
    maps = np.asarray(maps)
    if maps.ndim == 2:
        maps = maps[None]
    streams, coded = [], maps.copy()
    for f in range(maps.shape[0]):
        x0, y0, w, h = (0, 0, maps.shape[2], maps.shape[1]) if rects is None else (int(v) for v in rects[f])
        if w == 0 and h == 0:
            x0, y0, w, h = 0, 0, 1, 1
        stream, c = encode_lossy(maps[f, y0:y0 + h, x0:x0 + w].reshape(-1), m, near, segment)
        streams.append(stream)
        coded[f, y0:y0 + h, x0:x0 + w] = c.reshape(h, w)
    offsets = np.zeros(len(streams) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in streams])
    return np.frombuffer(b"".join(streams), dtype=np.uint8), offsets, coded


def used_rows(palette):
    """The used rows of a (K, 3) palette as float64 sRGB: bytes / 255, or the float rows without the trailing (-1, -1, -1) ones."""
    pal = np.asarray(palette)
    if pal.dtype == np.uint8:
        return pal.astype(np.float64) / 255.0
    k = pal.shape[0]
    while k > 0 and np.all(pal[k - 1] == -1.0):
        k -= 1
    return np.ascontiguousarray(pal[:k], dtype=np.float64)


def distances(palette):
    """(k, k) float64: D = (d0 * d0 + d1 * d1) + d2 * d2 between the used rows in ICtCp, the D of the frame_deltas contract."""
    rows = used_rows(palette)
    lab = color_ref.convert_f64("srgb_to_ictcp", np.ascontiguousarray(rows.T).reshape(-1)).reshape(3, rows.shape[0]).T
    d = lab[:, None, :] - lab[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbours(palette, tolerance, transparent_index=None, max_neighbours=15, undecided=None):
    """The table of gif_neighbours: (256, 16) uint8.  undecided: a list that receives (s, e) or (s, e1, e2) of every pair whose D lies
    within a relative 1e-9 of tolerance^2, and of every two D's of a row closer than that which are not both exactly 0: where the
    library's pow and numpy's may decide differently."""
    D = distances(palette)
    k = D.shape[0]
    t2 = float(tolerance) * float(tolerance)
    near = empty_table()
    for s in range(k):
        if s == transparent_index:
            continue
        cand = [(float(D[s, e]), e) for e in range(k) if e != s and e != transparent_index]
        if undecided is not None:
            undecided.extend((s, e) for d, e in cand if abs(d - t2) <= 1e-9 * max(d, t2) and not (d == 0.0 and t2 == 0.0))
        inside = sorted((d, e) for d, e in cand if d <= t2)
        if undecided is not None:
            undecided.extend((s, a[1], b[1]) for a, b in zip(inside, inside[1:]) if b[0] - a[0] <= 1e-9 * b[0] and not (a[0] == 0.0 and b[0] == 0.0))
        inside = inside[:max_neighbours]
        near[s, 0] = len(inside)
        near[s, 1:1 + len(inside)] = [e for _, e in inside]
    return near
