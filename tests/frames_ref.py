"""Reference of the frames entry (quantize_frames / patolette_amd_frames_u8), stated with what the CPU oracle exports
(test infrastructure).

  * palette: the reference's patolette() up to and including the KMeans refinement on the N = F*H*W pixels of the frames laid one
    after another -- `oracle.binding.patolette(W, F*H, stacked, w, K, palette_only=True, ...)`: with palette_only the reference
    leaves the palette in the quantisation space (patolette.c:266 skips the map stage and its conversions);
  * maps: the reference's map stage (patolette.c:266-324) frame by frame with that palette: `dither` over the frame's own W x H curve
    from an empty queue, or `nn_map`, on the frame and the palette converted as that branch converts them;
  * the returned palette takes the conversions of the branch that was run (for palette_only: none)."""
import numpy as np


def u8_frames(frames):
    """(F, H, W, 3|4) uint8 -> (F, H*W, 3) float64 sRGB in [0, 1], as the 8-bit entries ingest them (v / 255.0)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4
    f, h, w, _ = frames.shape
    return frames[..., :3].reshape(f, h * w, 3).astype(np.float64) / 255.0


def _working(ob, cs, flat):
    """planar sRGB -> the quantisation space (patolette.c:201-207)"""
    if cs == 1:
        return ob.convert("srgb_to_cieluv", flat)
    if cs == 2:
        return ob.convert("srgb_to_ictcp", flat)
    return np.array(flat, dtype=np.float64, copy=True)


def _to_rec2020(ob, cs, flat):
    return ob.convert({0: "srgb_to_rec2020", 1: "cieluv_to_rec2020", 2: "ictcp_to_rec2020"}[cs], flat)


def _nn_space(ob, cs, flat):
    """what the nearest map compares in (patolette.c:300-324): CIELuv takes the detour to ICtCp, the others stay"""
    if cs == 1:
        return ob.convert("srgb_to_ictcp", ob.convert("rec2020_to_srgb", ob.convert("cieluv_to_rec2020", flat)))
    return flat


def working_palette(ob, frames, K, weights=None, color_space=2, kmeans_niter=32, kmeans_max_samples=512 ** 2):
    """The shared palette in the quantisation space: (len, 3) rows (the used ones)."""
    rows = u8_frames(frames)
    f, n, _ = rows.shape
    h, w = frames.shape[1:3]
    wts = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    ec, pal, _ = ob.patolette(w, f * h, ob.planar(rows.reshape(f * n, 3)), wts, K, palette_only=True, color_space=color_space,
                              kmeans_niter=kmeans_niter, kmeans_max_samples=kmeans_max_samples)
    assert ec == 0
    used = ~np.all(pal == -1.0, axis=1)
    length = int(used.sum())
    assert np.all(used[:length])
    return np.ascontiguousarray(pal[:length])


def quantize_frames(ob, frames, K, dither=True, palette_only=False, color_space=2, kmeans_niter=32, kmeans_max_samples=512 ** 2,
                    weights=None):
    """Returns (palette (K,3) float64 with unused rows -1, maps (F,H,W) int64 or None)."""
    frames = np.asarray(frames)
    f, h, w, _ = frames.shape
    cs = int(color_space)
    wp = working_palette(ob, frames, K, weights, cs, kmeans_niter, kmeans_max_samples)
    length = wp.shape[0]
    pflat = ob.planar(wp)
    out = np.full((K, 3), -1.0)
    if palette_only:
        out[:length] = wp
        return np.asfortranarray(out), None
    rows = u8_frames(frames)
    maps = np.zeros((f, h, w), dtype=np.int64)
    if dither:
        pmap = ob.unplanar(_to_rec2020(ob, cs, pflat), length)
        for i in range(f):
            img = _to_rec2020(ob, cs, _working(ob, cs, ob.planar(rows[i])))
            maps[i] = ob.dither(img, w, h, pmap).astype(np.int64).reshape(h, w)       # a fresh call: the queue starts empty
        final = ob.convert("rec2020_to_srgb", ob.planar(pmap))
    else:
        pnn = _nn_space(ob, cs, pflat)
        pmap = ob.unplanar(pnn, length)
        for i in range(f):
            img = _nn_space(ob, cs, _working(ob, cs, ob.planar(rows[i])))
            maps[i] = ob.nn_map(img, w * h, pmap).astype(np.int64).reshape(h, w)
        final = ob.convert("rec2020_to_srgb", ob.convert("ictcp_to_rec2020", pnn))    # patolette.c:321-322, whatever the colour space
    out[:length] = ob.unplanar(final, length)
    return np.asfortranarray(out), maps
