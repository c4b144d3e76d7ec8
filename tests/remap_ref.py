"""Reference of the remap entry (remap / patolette_amd_remap_u8), stated with what the CPU oracle exports (test infrastructure).

  * pixels and a byte palette take the same expression: value = u8 / 255.0;
  * a float palette is taken as it is, after its trailing (-1, -1, -1) rows (the reference's fill of unused rows) are dropped;
  * dither off: palette and pixels -> ICtCp (`convert("srgb_to_ictcp")`), then `nn_map`;
  * dither on: palette and pixels -> linear Rec2020 (`convert("srgb_to_rec2020")`), then a FRESH `dither` call per frame over that
    frame's own W x H curve (the error queue starts empty);
  * quantized = pal8[map], pal8 = the byte palette as given, or clip(palette * 255, 0, 255) truncated for a float one."""
import numpy as np


def palette_rows(palette):
    """The palette's rows as (k, 3) float64 sRGB: bytes / 255.0, or the float rows without the trailing unused ones."""
    pal = np.asarray(palette)
    assert pal.ndim == 2 and pal.shape[1] == 3
    if pal.dtype == np.uint8:
        return pal.astype(np.float64) / 255.0
    pal = np.asarray(pal, dtype=np.float64)
    k = pal.shape[0]
    while k > 0 and np.all(pal[k - 1] == -1.0):
        k -= 1
    assert k >= 1 and np.all(np.isfinite(pal[:k]))
    return np.ascontiguousarray(pal[:k])


def pal8(palette):
    """The bytes `quantized` is made of: one row per row of the palette as given."""
    pal = np.asarray(palette)
    if pal.dtype == np.uint8:
        return np.ascontiguousarray(pal)
    return np.clip(np.asarray(pal, dtype=np.float64) * 255.0, 0.0, 255.0).astype(np.uint8)


def remap(ob, image, palette, dither=True):
    """image: (H, W, 3|4) or (F, H, W, 3|4) uint8.  Returns (map of the image's shape without the channels, int64; quantized uint8)."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim in (3, 4) and image.shape[-1] in (3, 4)
    frames = image if image.ndim == 4 else image[None]
    f, h, w, _ = frames.shape
    rows = palette_rows(palette)
    k = rows.shape[0]
    name = "srgb_to_rec2020" if dither else "srgb_to_ictcp"
    pmap = ob.unplanar(ob.convert(name, ob.planar(rows)), k)
    maps = np.zeros((f, h, w), dtype=np.int64)
    for i in range(f):
        px = frames[i, :, :, :3].reshape(h * w, 3).astype(np.float64) / 255.0
        img = ob.convert(name, ob.planar(px))
        if dither:
            maps[i] = ob.dither(img, w, h, pmap).astype(np.int64).reshape(h, w)       # a fresh call: the queue starts empty
        else:
            maps[i] = ob.nn_map(img, w * h, pmap).astype(np.int64).reshape(h, w)
    quant = pal8(palette)[maps]
    if image.ndim == 3:
        return maps[0], quant[0]
    return maps, quant
