"""Reference of the frame deltas with a colour table per frame (frame_deltas_local / patolette_amd_frame_deltas_local), stated in numpy
on the pieces of tests/delta_ref.py (test infrastructure).  The definition is the one in include/patolette_amd.h:

  * P tables of K rows of bytes; frame f is drawn with table g(f) = palette_of[f] (None: g(f) = f); col(f, a) = row a of table g(f);
  * frame 0: delta = m[0], the canvas colour C = col(0, m[0]); rect (0, 0, W, H), changed = H * W;
  * frame f >= 1, every position on its own, a = m[f][p]:
      keep = (col(f, a) == C over the three bytes) or (tolerance > 0 and D <= tolerance * tolerance), D evaluated only where the bytes
      differ, between the SOURCE pixel (bytes / 255.0) and the canvas colour (bytes / 255.0), both through `convert("srgb_to_ictcp")`,
      D = (d0*d0 + d1*d1) + d2*d2 (numpy fuses nothing);
      keep: delta = T; otherwise delta = a and C = col(f, a); shown_rgb = C;
  * rect = the tight box (x0, y0, w, h) of delta != T, (0, 0, 0, 0) when there is none; changed = their number.

Every call also reports the smallest relative gap |D - tol^2| / tol^2 over every D it evaluated, how many it evaluated and how many
kept, as delta_ref.frame_deltas does and for the same reason.

Also here: a GIF reader that accepts local colour tables (`parse_gif`; lzw_ref.parse_gif refuses them and stays as it is), and an RGB
compositor for disposal 0 / 1 (`composite_rgb`)."""
import numpy as np

from tests import lzw_ref
from tests.delta_ref import rect_of


def tables_of(palette_of, P, F):
    of = np.arange(F) if palette_of is None else np.asarray(palette_of).astype(np.int64)
    assert of.shape == (F,) and np.all(of >= 0) and np.all(of < P) and (palette_of is not None or P == F)
    return of


def frame_deltas(ob, maps, palettes, palette_of=None, T=None, frames=None, tolerance=0.0):
    """maps: (F, H, W) integers below K; palettes: (P, K, 3) uint8; frames: (F, H, W, 3|4) uint8 (tolerance > 0).
    Returns (deltas int64, shown_rgb (F, H, W, 3) uint8, rects (F, 4) int32, changed (F,) int64, smallest relative gap, D evaluated,
    of them kept)."""
    maps = np.asarray(maps).astype(np.int64)
    palettes = np.asarray(palettes)
    assert palettes.dtype == np.uint8 and palettes.ndim == 3 and palettes.shape[2] == 3
    P, K, _ = palettes.shape
    F, h, w = maps.shape
    of = tables_of(palette_of, P, F)
    T = K if T is None else int(T)
    assert 1 <= K <= T <= 255 and np.all(maps >= 0) and np.all(maps < K)
    tol2 = np.float64(tolerance) * np.float64(tolerance)
    deltas = np.empty_like(maps)
    shown = np.empty((F, h, w, 3), dtype=np.uint8)
    rects, changed = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.int64)
    canvas = palettes[of[0]][maps[0]]                                   # (h, w, 3) bytes
    deltas[0], shown[0] = maps[0], canvas
    rects[0], changed[0] = (0, 0, w, h), h * w
    gap, tested, kept = np.inf, 0, 0

    def ictcp(rgb8):
        v = rgb8.astype(np.float64) / 255.0
        return ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(v)), v.shape[0])

    for f in range(1, F):
        a = maps[f]
        col = palettes[of[f]][a]
        differs = np.any(col != canvas, axis=-1)
        keep = ~differs
        if tolerance > 0.0 and np.any(differs):
            d = ictcp(np.asarray(frames)[f][..., :3][differs]) - ictcp(canvas[differs])
            D = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            near = D <= tol2
            gap = min(gap, float(np.min(np.abs(D - tol2) / tol2)))
            tested += int(D.size)
            kept += int(np.sum(near))
            keep[differs] = near
        move = ~keep
        deltas[f] = np.where(move, a, T)
        canvas = np.where(move[..., None], col, canvas)
        shown[f] = canvas
        rects[f] = rect_of(move)
        changed[f] = int(np.sum(move))
    return deltas, shown, rects, changed, gap, tested, kept


def replay_rgb(deltas, palettes, palette_of, T):
    """Consequence (a): draw deltas[f] with table g(f) over the canvas, skipping T.  Returns every frame's canvas, (F, H, W, 3) uint8."""
    deltas = np.asarray(deltas).astype(np.int64)
    palettes = np.asarray(palettes)
    of = tables_of(palette_of, palettes.shape[0], deltas.shape[0])
    out = np.empty(deltas.shape + (3,), dtype=np.uint8)
    canvas = np.zeros(deltas.shape[1:] + (3,), dtype=np.uint8)
    for f in range(deltas.shape[0]):
        draw = deltas[f] != T if f > 0 else np.ones(deltas.shape[1:], dtype=bool)
        canvas = np.where(draw[..., None], palettes[of[f]][np.where(draw, deltas[f], 0)], canvas)
        out[f] = canvas
    return out


def parse_gif(blob):
    """lzw_ref.parse_gif with local colour tables: every frame dict also has `table`, its local table ((2^k, 3) uint8) or None for a
    frame drawn with the global one, and `packed`, the image descriptor's packed byte.  Interlace is refused."""
    assert blob[:6] == b"GIF89a"
    u16 = lambda p: blob[p] | blob[p + 1] << 8
    head = dict(width=u16(6), height=u16(8), loop=None, table=None)
    packed = blob[10]
    p = 13
    if packed & 0x80:
        n = 2 << (packed & 7)
        head["table"] = np.frombuffer(blob[p:p + 3 * n], dtype=np.uint8).reshape(n, 3).copy()
        p += 3 * n
    frames, gce = [], None

    def blocks(p):
        data = bytearray()
        while blob[p]:
            data += blob[p + 1:p + 1 + blob[p]]
            p += 1 + blob[p]
        return bytes(data), p + 1

    while True:
        kind = blob[p]
        if kind == 0x3B:
            assert p == len(blob) - 1, "bytes after the trailer"
            break
        if kind == 0x21:
            label = blob[p + 1]
            data, p = blocks(p + 2)
            if label == 0xF9:
                assert len(data) == 4
                gce = dict(disposal=(data[0] >> 2) & 7, transparent=data[3] if data[0] & 1 else None, delay_cs=data[1] | data[2] << 8)
            elif label == 0xFF and data[:11] == b"NETSCAPE2.0":
                assert data[11] == 1
                head["loop"] = data[12] | data[13] << 8
            continue
        assert kind == 0x2C, "neither an extension, an image nor the trailer"
        rect = (u16(p + 1), u16(p + 3), u16(p + 5), u16(p + 7))
        flags = blob[p + 9]
        assert flags & 0x78 == 0, "interlace, the sort flag and the reserved bits are out of scope"
        p += 10
        table = None
        if flags & 0x80:
            n = 2 << (flags & 7)
            table = np.frombuffer(blob[p:p + 3 * n], dtype=np.uint8).reshape(n, 3).copy()
            p += 3 * n
        else:
            assert flags == 0
        m = blob[p]
        stream, p = blocks(p + 1)
        frame = dict(rect=rect, m=m, stream=stream, table=table, packed=flags)
        frame.update(gce or dict(disposal=0, transparent=None, delay_cs=0))
        frames.append(frame)
        gce = None
    return head, frames


def composite_rgb(head, frames):
    """Every frame's canvas of colours, (F, H, W, 3) uint8, as a viewer builds it with disposal 0 / 1: inside the rectangle every
    decoded index but the transparent one is drawn with the frame's local table, or the global one.  The canvas starts black."""
    canvas = np.zeros((head["height"], head["width"], 3), dtype=np.uint8)
    out = []
    for fr in frames:
        assert fr["disposal"] in (0, 1)
        table = fr["table"] if fr["table"] is not None else head["table"]
        x0, y0, w, h = fr["rect"]
        idx = np.array(lzw_ref.decode(fr["stream"], fr["m"], w * h), dtype=np.int64).reshape(h, w)
        assert np.all(idx < table.shape[0])
        keep = idx == fr["transparent"] if fr["transparent"] is not None else np.zeros_like(idx, dtype=bool)
        part = canvas[y0:y0 + h, x0:x0 + w]
        canvas[y0:y0 + h, x0:x0 + w] = np.where(keep[..., None], part, table[idx])
        out.append(canvas.copy())
    return np.stack(out)
