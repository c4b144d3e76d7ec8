"""Reference of the frame deltas of RGBA maps (frame_deltas_rgba / patolette_amd_frame_deltas_rgba), stated in numpy on top of what the
CPU oracle exports (test infrastructure).  The definition is the one in include/patolette_amd.h: index 0 is the transparent entry, 0 in
a delta means "leave the canvas", the canvas c starts as all 0, and frame after frame

  * next(f) = f + 1, for the last frame 0 with `loop`, none without;
  * V[f] = the tight box of m[f] != 0 & m[next(f)] == 0 (empty without a next frame); disposals[f] = 2 if V[f] is not empty, else 1;
  * a = m[f][p] == 0: delta = 0;  a != 0: keep = c != 0 and (a == c or (tolerance > 0 and D <= tolerance * tolerance)), D as in
    tests/delta_ref.py (the SOURCE pixel against palette row c through `convert("srgb_to_ictcp")`, (d0*d0 + d1*d1) + d2*d2), evaluated
    only where c != 0 and a != c;  keep: delta = 0, otherwise delta = a and c = a;  shown = c;
  * C[f] = the tight box of delta != 0, changed[f] their number; rects[f] = the smallest box holding C[f] and V[f], (0, 0, 0, 0) when
    both are empty;  then, with disposal 2, c = 0 inside rects[f].

Like delta_ref.frame_deltas, every call reports the smallest relative gap |D - tol^2| / tol^2 over every D it evaluated, how many it
evaluated and how many of them kept.

Also here: `replay`, a viewer that honours rectangles and disposal 1 / 2 over several passes of the loop; `wrap_gif`, the tests' own
container with one disposal per frame; `clip`, the RGBA clip the tests use; `maps_of`, the reference's own maps of it."""
import numpy as np

from tests import delta_ref, lzw_ref, remap_ref, rgba_remap_ref
from tests.delta_ref import rect_of


def union(a, b):
    """The smallest (x0, y0, w, h) holding both boxes; an empty one is (0, 0, 0, 0)."""
    if a[2] == 0:
        return tuple(int(v) for v in b)
    if b[2] == 0:
        return tuple(int(v) for v in a)
    x0, y0 = min(a[0], b[0]), min(a[1], b[1])
    x1, y1 = max(a[0] + a[2], b[0] + b[2]), max(a[1] + a[3], b[1] + b[3])
    return (int(x0), int(y0), int(x1 - x0), int(y1 - y0))


def used_rows(palette):
    """The palette's used rows as (k, 3) float64 sRGB, row 0 (the transparent entry) included: a (K, 4) uint8 RGBA palette without its
    trailing (0, 0, 0, 0) rows, or what remap_ref.palette_rows takes."""
    pal = np.asarray(palette)
    if pal.ndim == 2 and pal.shape[1] == 4:
        assert pal.dtype == np.uint8
        k = pal.shape[0]
        while k > 0 and not pal[k - 1].any():
            k -= 1
        assert k >= 1 and pal[0, 3] == 0
        return pal[:k, :3].astype(np.float64) / 255.0
    if pal.dtype != np.uint8:                                      # (row 0's colour is never read: whatever it holds)
        pal = np.array(pal, dtype=np.float64)
        pal[0] = 0.0
    return remap_ref.palette_rows(pal)


def frame_deltas(ob, maps, palette, frames=None, tolerance=0.0, loop=True, near=None):
    """maps: (F, H, W) integers, 0 = transparent; palette: (K, 4) RGBA, (K, 3) with row 0 the transparent entry, or an int row count
    (tolerance 0 only); frames: (F, H, W, 3|4) uint8.  near: instead of a tolerance, an (F, H, W) boolean array that says where
    "D <= tolerance^2" holds (no oracle needed: the consequences must hold for any such predicate).
    Returns (deltas int64, shown int64, rects (F,4) int32, disposals (F,) int32, changed (F,) int64, smallest relative gap, D evaluated,
    of them kept)."""
    maps = np.asarray(maps).astype(np.int64)
    F, h, w = maps.shape
    pmap = None
    if isinstance(palette, (int, np.integer)):
        rows = int(palette)
        assert tolerance == 0.0
    else:
        used = used_rows(palette)
        rows = used.shape[0]
        if tolerance > 0.0:
            pmap = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(used)), rows)
    assert np.all(maps >= 0) and np.all(maps < rows)
    tol2 = np.float64(tolerance) * np.float64(tolerance)
    deltas, shown = np.zeros_like(maps), np.zeros_like(maps)
    rects, disposals, changed = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int64)
    canvas = np.zeros((h, w), dtype=np.int64)
    gap, tested, kept = np.inf, 0, 0
    for f in range(F):
        nxt = f + 1 if f + 1 < F else (0 if loop else None)
        V = rect_of((maps[f] != 0) & (maps[nxt] == 0)) if nxt is not None else (0, 0, 0, 0)
        a = maps[f]
        assert np.all((a != 0) | (canvas == 0))                    # "the canvas entry is provably 0 there already"
        differs = (a != 0) & (canvas != 0) & (a != canvas)
        keep = (canvas != 0) & (a == canvas)
        if near is not None:
            keep |= differs & np.asarray(near)[f]
        elif tolerance > 0.0 and np.any(differs):
            px = np.asarray(frames)[f][..., :3][differs].astype(np.float64) / 255.0
            v = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(px)), px.shape[0])
            d = v - pmap[canvas[differs]]
            D = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            close = D <= tol2
            gap = min(gap, float(np.min(np.abs(D - tol2) / tol2)))
            tested += int(D.size)
            kept += int(np.sum(close))
            keep[differs] = close
        move = (a != 0) & ~keep
        deltas[f] = np.where(move, a, 0)
        canvas = np.where(move, a, canvas)
        shown[f] = canvas
        changed[f] = int(np.sum(move))
        rects[f] = union(rect_of(move), V)
        disposals[f] = 2 if V[2] else 1
        if disposals[f] == 2:
            x0, y0, rw, rh = (int(v) for v in rects[f])
            canvas = canvas.copy()
            canvas[y0:y0 + rh, x0:x0 + rw] = 0
    return deltas, shown, rects, disposals, changed, gap, tested, kept


def replay(deltas, rects, disposals, passes=2, reset=False):
    """A viewer: in frame f the deltas inside rects[f] that are not 0 overwrite the canvas; what it then shows is recorded; then
    rects[f] is cleared to 0 where disposals[f] == 2 (1: left in place).  `passes` times through the frames; reset: whether the canvas
    starts empty again at every restart.  Asserts that no delta lies outside its rectangle.  Returns (passes * F, H, W) int64."""
    deltas = np.asarray(deltas).astype(np.int64)
    F, h, w = deltas.shape
    canvas = np.zeros((h, w), dtype=np.int64)
    out = []
    for _ in range(passes):
        if reset:
            canvas[:] = 0
        for f in range(F):
            assert int(disposals[f]) in (1, 2)
            x0, y0, rw, rh = (int(v) for v in rects[f])
            inside = np.zeros((h, w), dtype=bool)
            inside[y0:y0 + rh, x0:x0 + rw] = True
            assert not np.any((deltas[f] != 0) & ~inside), "a delta outside its rectangle"
            canvas = np.where(inside & (deltas[f] != 0), deltas[f], canvas)
            out.append(canvas.copy())
            if int(disposals[f]) == 2:
                canvas = np.where(inside, 0, canvas)
    return np.stack(out)


def replay_parsed(head, parsed, passes=2):
    """`replay` for what lzw_ref.parse_gif returns: the streams decoded with lzw_ref.decode, the transparent index standing for
    "leave the canvas", indices shifted by nothing.  Returns (passes * F, H, W) int64 with the transparent index wherever nothing shows."""
    h, w = head["height"], head["width"]
    F = len(parsed)
    deltas = np.zeros((F, h, w), dtype=np.int64)
    rects, disposals = np.zeros((F, 4), dtype=np.int64), np.zeros(F, dtype=np.int64)
    for f, fr in enumerate(parsed):
        assert fr["transparent"] == 0
        x0, y0, rw, rh = fr["rect"]
        deltas[f, y0:y0 + rh, x0:x0 + rw] = np.array(lzw_ref.decode(fr["stream"], fr["m"], rw * rh), dtype=np.int64).reshape(rh, rw)
        rects[f], disposals[f] = fr["rect"], fr["disposal"]
    return replay(deltas, rects, disposals, passes)


def wrap_gif(streams, rects, disposals, size, palette, m, delay_cs=4, loop=0):
    """The tests' own container (lzw_ref.wrap_gif frame by frame) with transparent index 0 and one disposal per frame."""
    blob = bytearray()
    for f, stream in enumerate(streams):
        one = lzw_ref.wrap_gif([stream], [rects[f]], size, palette, m, transparent_index=0, delay_cs=delay_cs, loop=loop,
                               disposal=int(disposals[f]))
        start = 0 if f == 0 else one.index(b"\x21\xf9\x04")        # (the header, the table and the loop block once)
        blob += one[start:-1]
    return bytes(blob + b"\x3b")


def pil_frames(blob):
    """Every frame of a GIF as PIL composes it, (F, H, W, 4) uint8 RGBA."""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    out = []
    for f in range(im.n_frames):
        im.seek(f)
        out.append(np.array(im.convert("RGBA")))
    return np.stack(out)


def rgba_of(palette_rgb, shown):
    """What a viewer shows for `shown`: (.., 4) uint8, palette_rgb[shown] with alpha 255, (0, 0, 0, 0) where shown is 0."""
    shown = np.asarray(shown).astype(np.int64)
    out = np.concatenate([np.asarray(palette_rgb)[shown], np.full(shown.shape + (1,), 255, dtype=np.uint8)], axis=-1)
    out[shown == 0] = 0
    return out


def same_picture(got, want):
    """Two (.., 4) RGBA arrays show the same: equal alpha, equal colour wherever alpha is not 0."""
    return np.array_equal(got[..., 3], want[..., 3]) and np.array_equal(got[want[..., 3] > 0], want[want[..., 3] > 0])


def clip(h, w, F, seed=5, jitter=2, rest=1):
    """(F, h, w, 4) uint8: delta_ref.clip with alpha 255 inside a disc that moves by (2, 3) per frame and 0 outside it, and alpha 0 in a
    static hole of (h // 5, w // 5) that the disc passes over.
    rest: the disc moves only every `rest`-th frame.  With rest == 1 some pixel vanishes in EVERY frame, so every frame is disposed to
    background over a rectangle that holds all it drew, every frame meets an empty canvas and draws its whole disc again: the contract
    then never compares two opaque entries, and the lossy mode evaluates no distance at all.  With rest == 2 every second frame
    finds its predecessor's canvas in place."""
    rgb = delta_ref.clip(h, w, F, seed, jitter)
    yy, xx = np.mgrid[0:h, 0:w]
    radius = 0.35 * min(h, w) + 0.5
    hh, hw = h // 5, w // 5
    out = np.empty((F, h, w, 4), dtype=np.uint8)
    out[..., :3] = rgb
    for i in range(F):
        cy, cx = (h // 3 + 2 * (i // rest)) % h, (w // 3 + 3 * (i // rest)) % w
        opaque = (yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius
        opaque[h // 3:h // 3 + hh, w // 3:w // 3 + hw] = False
        out[i, ..., 3] = np.where(opaque, 255, 0)
    return out


def maps_of(ob, frames, palette, kind="nearest"):
    """The reference's own maps of RGBA `frames` on `palette` (row 0 the transparent entry): int64, 0 where alpha < 128."""
    mode = rgba_remap_ref.NEAREST if kind == "nearest" else rgba_remap_ref.ORDERED
    assert kind in ("nearest", "ordered")
    pal = np.asarray(palette)
    return rgba_remap_ref.remap_rgba(ob, frames, pal, None if pal.shape[1] == 4 else 0, 128, mode)[0]
