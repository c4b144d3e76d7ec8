"""Reference of the frame deltas (frame_deltas / patolette_amd_frame_deltas), stated in numpy on top of what the CPU oracle exports
(test infrastructure).  The definition is the one in include/patolette_amd.h:

  * frame 0: delta = shown = canvas = m[0]; rect (0, 0, W, H), changed = H * W;
  * frame f >= 1, every position on its own, a = m[f][p], c = the canvas entry:
      keep = (a == c) or (tolerance > 0 and D <= tolerance * tolerance), D evaluated only where a != c, between the SOURCE pixel
      (bytes / 255.0) and palette row c, both through `convert("srgb_to_ictcp")`, D = (d0*d0 + d1*d1) + d2*d2 (numpy fuses nothing);
      keep: delta = T; otherwise delta = a and the canvas takes a; shown = the canvas;
  * rect = the tight box (x0, y0, w, h) of delta != T, (0, 0, 0, 0) when there is none; changed = their number.

Besides the outputs, every call reports the smallest relative gap |D - tol^2| / tol^2 over every D it evaluated, how many it evaluated
and how many of them kept: a bit-for-bit comparison with another implementation of pow means something only away from the threshold.

Also here: the clip the tests use (`clip`) and the reference's own maps of it (`maps_of`)."""
import numpy as np

from tests import ordered_ref, remap_ref
from tests.util import scene


def clip(h, w, F, seed=5, jitter=2):
    """(F, h, w, 3) uint8: one scene, every frame with its own +-jitter noise (drawn frame after frame from one generator) and an
    inverted block of (h // 4, w // 3) that moves by (2, 3) per frame."""
    base = np.round(scene(h, w, seed) * 255).astype(np.int64)
    rng = np.random.default_rng(seed)
    bh, bw = h // 4, w // 3
    out = np.empty((F, h, w, 3), dtype=np.uint8)
    for i in range(F):
        fr = base + rng.integers(-jitter, jitter + 1, size=base.shape)
        if bh > 0 and bw > 0:
            y0, x0 = (2 + 2 * i) % (h - bh), (1 + 3 * i) % (w - bw)
            fr[y0:y0 + bh, x0:x0 + bw] = 255 - base[y0:y0 + bh, x0:x0 + bw]
        out[i] = np.clip(fr, 0, 255).astype(np.uint8)
    return out


def maps_of(ob, frames, palette, kind):
    """The reference's own maps of `frames` on `palette`: kind "nearest", or "ordered" at the palette's default spread.  int64."""
    if kind == "nearest":
        return remap_ref.remap(ob, frames, palette, dither=False)[0]
    assert kind == "ordered"
    return ordered_ref.remap(ob, frames, palette, ordered_ref.ordered_spread(palette))[0]


def rect_of(mask):
    """(x0, y0, w, h) of the True cells of an (h, w) mask; (0, 0, 0, 0) for none."""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return (0, 0, 0, 0)
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


def frame_deltas(ob, maps, palette, T=None, frames=None, tolerance=0.0):
    """maps: (F, H, W) integers; palette: what remap takes, or an int row count (tolerance 0 only); frames: (F, H, W, 3|4) uint8.
    Returns (deltas int64, shown int64, rects (F,4) int32, changed (F,) int64, smallest relative gap, D evaluated, of them kept)."""
    maps = np.asarray(maps).astype(np.int64)
    F, h, w = maps.shape
    pmap = None
    if isinstance(palette, (int, np.integer)):
        rows = int(palette)
        assert tolerance == 0.0
    else:
        rows = np.asarray(palette).shape[0]
        used = remap_ref.palette_rows(palette)
        if tolerance > 0.0:
            pmap = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(used)), used.shape[0])
        assert np.all(maps < used.shape[0])
    T = rows if T is None else int(T)
    assert T >= rows and np.all(maps >= 0) and np.all(maps < rows)
    tol2 = np.float64(tolerance) * np.float64(tolerance)
    deltas, shown = np.empty_like(maps), np.empty_like(maps)
    rects, changed = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.int64)
    canvas = maps[0].copy()
    deltas[0], shown[0] = maps[0], maps[0]
    rects[0], changed[0] = (0, 0, w, h), h * w
    gap, tested, kept = np.inf, 0, 0
    for f in range(1, F):
        a = maps[f]
        differs = a != canvas
        keep = ~differs
        if tolerance > 0.0 and np.any(differs):
            px = np.asarray(frames)[f][..., :3][differs].astype(np.float64) / 255.0          # the differing positions, row-scan order
            v = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(px)), px.shape[0])
            d = v - pmap[canvas[differs]]
            D = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            near = D <= tol2
            gap = min(gap, float(np.min(np.abs(D - tol2) / tol2)))
            tested += int(D.size)
            kept += int(np.sum(near))
            keep[differs] = near
        move = ~keep
        deltas[f] = np.where(move, a, T)
        canvas = np.where(move, a, canvas)
        shown[f] = canvas
        rects[f] = rect_of(move)
        changed[f] = int(np.sum(move))
    return deltas, shown, rects, changed, gap, tested, kept


def replay(deltas, T):
    """Compositing: start from deltas[0]; in frame f overwrite the positions where deltas[f] != T.  Returns every frame's canvas."""
    deltas = np.asarray(deltas).astype(np.int64)
    out = np.empty_like(deltas)
    canvas = deltas[0].copy()
    out[0] = canvas
    for f in range(1, deltas.shape[0]):
        canvas = np.where(deltas[f] != T, deltas[f], canvas)
        out[f] = canvas
    return out


def distances2(ob, frames, palette, shown):
    """SQUARED ICtCp distance (the contract's D) of every position's source pixel to the palette row `shown` names: (F, H, W) float64."""
    frames, shown = np.asarray(frames), np.asarray(shown).astype(np.int64)
    used = remap_ref.palette_rows(palette)
    pmap = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(used)), used.shape[0])
    F, h, w = shown.shape
    out = np.empty((F, h, w))
    for f in range(F):
        px = frames[f][..., :3].reshape(h * w, 3).astype(np.float64) / 255.0
        v = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(px)), h * w)
        d = v - pmap[shown[f].reshape(-1)]
        out[f] = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).reshape(h, w)
    return out
