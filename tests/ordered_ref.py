"""Reference of the ordered remap (remap(dither="ordered") / patolette_amd_remap_ordered_u8), stated in numpy on top of what the CPU
oracle exports (test infrastructure).  The definition is the one in include/patolette_amd.h:

  * B(x, y): the 8x8 Bayer index of the pixel's place IN ITS OWN FRAME; t = (B + 0.5) / 64 - 0.5;
  * v = clip(bytes / 255.0 + spread * t, 0, 1), the same shift on R, G and B, one rounding per operation (numpy fuses nothing);
  * palette rows as tests/remap_ref.py takes them; palette and v -> ICtCp (`convert("srgb_to_ictcp")`), then `nn_map`;
  * quantized = pal8[map].

Besides the map, every call reports the smallest relative gap (d2 - d1) / d2 between the best and the second-best row over all
pixels: a bit-for-bit comparison with another implementation of pow means something only away from exact ties."""
import numpy as np

from tests import remap_ref


def bayer8(x, y):
    """The 8x8 Bayer index of (x & 7, y & 7), arrays or scalars."""
    x, y = np.asarray(x, dtype=np.int64) & 7, np.asarray(y, dtype=np.int64) & 7
    v = np.zeros(np.broadcast(x, y).shape, dtype=np.int64)
    for i in range(3):
        v = (v << 2) | ((((x >> i) ^ (y >> i)) & 1) << 1) | ((y >> i) & 1)
    return v


def threshold(h, w):
    """t of every pixel of an (h, w) frame, in (-0.5, 0.5)."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (bayer8(xx, yy).astype(np.float64) + 0.5) / 64.0 - 0.5


def shifted(frame, spread):
    """(h, w, 3|4) uint8 -> the (h*w, 3) float64 values the search sees."""
    h, w = frame.shape[:2]
    s = np.float64(spread) * threshold(h, w)
    v = frame[:, :, :3].astype(np.float64) / 255.0 + s[:, :, None]
    return np.minimum(np.maximum(v, 0.0), 1.0).reshape(h * w, 3)


def _gap(img, pmap, best):
    """min over pixels of (d2 - d1) / d2, d1 <= d2 the two smallest distances (1.0 for a one-row palette; the distances in numpy)."""
    k = pmap.shape[0]
    if k < 2:
        return 1.0
    n = img.shape[0]
    gap = 1.0
    for a in range(0, n, 2048):
        d = img[a:a + 2048, None, :] - pmap[None, :, :]
        d = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        rows = np.arange(d.shape[0])
        d1 = d[rows, best[a:a + 2048]]
        d[rows, best[a:a + 2048]] = np.inf
        d2 = np.min(d, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            g = np.where(d2 > 0.0, (d2 - d1) / d2, 0.0)
        gap = min(gap, float(np.min(g)))
    return gap


def remap(ob, image, palette, spread):
    """image: (H, W, 3|4) or (F, H, W, 3|4) uint8.  Returns (map of the image's shape without the channels, int64; quantized uint8;
    the smallest relative gap between the best and the second-best row over all pixels)."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim in (3, 4) and image.shape[-1] in (3, 4)
    frames = image if image.ndim == 4 else image[None]
    f, h, w, _ = frames.shape
    rows = remap_ref.palette_rows(palette)
    k = rows.shape[0]
    pmap = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(rows)), k)
    maps = np.zeros((f, h, w), dtype=np.int64)
    gap = 1.0
    for i in range(f):
        flat = ob.convert("srgb_to_ictcp", ob.planar(shifted(frames[i], spread)))
        best = ob.nn_map(flat, w * h, pmap).astype(np.int64)
        gap = min(gap, _gap(ob.unplanar(flat, w * h), pmap, best))
        maps[i] = best.reshape(h, w)
    quant = remap_ref.pal8(palette)[maps]
    if image.ndim == 3:
        return maps[0], quant[0], gap
    return maps, quant, gap


def ordered_spread(palette):
    """mean over the used rows of the Euclidean sRGB distance to the nearest other row, / sqrt(3); 0.0 for one row."""
    rows = remap_ref.palette_rows(palette)
    k = rows.shape[0]
    if k < 2:
        return 0.0
    near = []
    for i in range(k):
        d = np.sqrt(np.sum((rows - rows[i]) ** 2, axis=1))
        near.append(np.min(np.delete(d, i)))
    return float(np.mean(near) / np.sqrt(3.0))


def block_rmse(image, quant, block=8):
    """RMSE, in code values, between the block x block means of the image and of its quantized form (what the eye averages)."""
    def means(a):
        a = a[..., :3].astype(np.float64)
        h, w = a.shape[0] // block * block, a.shape[1] // block * block
        return a[:h, :w].reshape(h // block, block, w // block, block, 3).mean(axis=(1, 3))
    return float(np.sqrt(np.mean((means(image) - means(quant)) ** 2)))
