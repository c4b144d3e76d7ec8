"""The model the ColorHistogram tests hold the kernels to: a few lines of numpy, all integers.

  key    = R << 16 | G << 8 | B; a 4th channel does not enter it; with alpha_threshold a pixel with alpha < threshold enters nothing
  count  = pixels per key
  units  = per key the sum of rint(w * 2^32) as uint64 (np.rint: ties to even, the scaling by a power of two is exact)
  weight = the count (unweighted), or units / 2^32 with ONE rounding: uint64 -> float64 (exact below 2^53, nearest-even above), then
           an exact scaling"""
import numpy as np


def units(w):
    return np.rint(np.asarray(w, dtype=np.float64) * 2.0 ** 32).astype(np.uint64)


def weights_ok(w):
    w = np.asarray(w, dtype=np.float64)
    return bool(np.all(np.isfinite(w)) and np.all(w >= 0) and np.all(w <= 2.0 ** 20))


def keys(px):
    px = np.asarray(px)
    flat = px.reshape(-1, px.shape[-1]).astype(np.int64)
    return flat[:, 0] << 16 | flat[:, 1] << 8 | flat[:, 2]


def unit_sums(px, w=None, alpha_threshold=None):
    """(keys ascending, counts int64, unit sums uint64 or None) of the pixels that enter."""
    px = np.asarray(px)
    k = keys(px)
    enter = np.ones(len(k), dtype=bool)
    if alpha_threshold is not None:
        enter = px.reshape(-1, px.shape[-1])[:, 3] >= alpha_threshold
    uniq, inv, counts = np.unique(k[enter], return_inverse=True, return_counts=True)
    if w is None:
        return uniq, counts.astype(np.int64), None
    sums = np.zeros(len(uniq), dtype=np.uint64)
    np.add.at(sums, inv, units(np.asarray(w).reshape(-1)[enter]))
    return uniq, counts.astype(np.int64), sums


def model(px, w=None, alpha_threshold=None):
    """What export() must return: (colors (M, 3) uint8, counts (M,) int64, weights (M,) float64)."""
    uniq, counts, sums = unit_sums(px, w, alpha_threshold)
    colors = np.stack([uniq >> 16, (uniq >> 8) & 255, uniq & 255], axis=1).astype(np.uint8).reshape(-1, 3)
    weights = counts.astype(np.float64) if sums is None else sums.astype(np.float64) / 2.0 ** 32
    return colors, counts, weights
