"""Reference of measure (measure / patolette_amd_measure), stated in numpy on top of what the CPU oracle exports (test infrastructure).
The definition is the one in include/patolette_amd.h:

  * a position whose element equals skip_index enters nothing; every other element must be a used row of the palette;
  * integer part: e = sum_c (b[c] - pal8[a][c])^2 with `remap_ref.pal8`; count, sse and max_se per palette row (as given) and per frame;
  * ICtCp part: D as `delta_ref.distances2` computes it (pixel bytes / 255.0 and the palette's row as given, both through
    `convert("srgb_to_ictcp")`, D = (d0*d0 + d1*d1) + d2*d2); per frame `np.sum` and `np.max` over the positions that were not
    skipped, 0 for a frame with none."""
import numpy as np

from tests import delta_ref, remap_ref


def measure(ob, image, maps, palette, skip_index=None, ictcp=True):
    """image: (H, W, 3|4) or (F, H, W, 3|4) uint8; maps: (H, W) or (F, H, W) integers.
    Returns (entries (K, 3) int64, per_frame (F, 3) int64, ictcp (F, 2) float64 or None); columns as `patolette_amd.measure`."""
    image, maps = np.asarray(image), np.asarray(maps).astype(np.int64)
    if image.ndim == 3:
        image, maps = image[None], maps[None]
    F, h, w = maps.shape
    assert image.shape[:3] == maps.shape and image.dtype == np.uint8 and image.shape[3] in (3, 4)
    rows = np.asarray(palette).shape[0]
    used = remap_ref.palette_rows(palette).shape[0]
    p8 = remap_ref.pal8(palette).astype(np.int64)
    keep = np.ones(maps.shape, dtype=bool) if skip_index is None else maps != int(skip_index)
    assert np.all((maps[keep] >= 0) & (maps[keep] < used))
    safe = np.where(keep, maps, 0)
    diff = image[..., :3].astype(np.int64) - p8[safe]
    e = np.sum(diff * diff, axis=-1)
    entries, per_frame = np.zeros((rows, 3), dtype=np.int64), np.zeros((F, 3), dtype=np.int64)
    entries[:, 0] = np.bincount(safe[keep], minlength=rows)
    np.add.at(entries[:, 1], safe[keep], e[keep])                                    # (integers: bincount's weights are float64)
    np.maximum.at(entries[:, 2], safe[keep], e[keep])
    for f in range(F):
        per_frame[f] = (int(np.sum(keep[f])), int(np.sum(e[f][keep[f]])), int(np.max(e[f][keep[f]], initial=0)))
    if not ictcp:
        return entries, per_frame, None
    D = delta_ref.distances2(ob, image, palette, safe)
    dist = np.zeros((F, 2))
    for f in range(F):
        d = D[f][keep[f]]
        if d.size:
            dist[f] = (np.sum(d), np.max(d))
    return entries, per_frame, dist
