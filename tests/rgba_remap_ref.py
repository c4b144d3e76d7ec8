"""Reference of the remap with alpha (remap_rgba / patolette_amd_remap_rgba_u8), composed in numpy from the references the RGB remaps
and the RGBA entry already have (test infrastructure).  The contract is the one in include/patolette_amd.h:

  * a pixel is transparent iff alpha < alpha_threshold;
  * the palette's used rows without the transparent entry are the OPAQUE ROWS; off = 1 when row 0 is the transparent entry, else 0;
  * nearest / ordered: an opaque pixel's element is off + what `remap_ref.remap(dither=False)` / `ordered_ref.remap(spread)` give that
    pixel on the opaque rows (per pixel, at its place in its own frame: the RGB under transparent pixels cannot matter);
  * Riemersma: per frame `rgba_ref.masked_dither` over the frame's own curve on the opaque rows in linear Rec2020, transparent pixels
    skipped; a frame without a transparent pixel is `remap_ref.remap(dither=True)` of it (the oracle's own walk);
  * transparent pixels: element 0 and (0, 0, 0, 0); opaque pixels: (pal8[element], 255), pal8 = `remap_ref.pal8`."""
import numpy as np

from tests import ordered_ref, remap_ref, rgba_ref

NEAREST, RIEMERSMA, ORDERED = 0, 1, 2


def split(palette, transparent_index=None):
    """-> (the opaque rows in the form `remap_ref` takes: uint8 or float (k, 3); off; palette_rgba, one RGBA row per row of the palette
    as given: (pal8, 255) on opaque rows, (0, 0, 0, 0) on the transparent entry and on unused rows)."""
    pal = np.asarray(palette)
    assert pal.ndim == 2 and pal.shape[0] >= 1
    if pal.shape[1] == 4:                                          # as quantize_rgba returns palette_rgba
        assert pal.dtype == np.uint8
        k = pal.shape[0]
        while k > 0 and not pal[k - 1].any():
            k -= 1
        off = 1 if k > 0 and pal[0, 3] == 0 else 0
        assert transparent_index is None or (0 if off else -1) == transparent_index
        assert k > off and np.all(pal[off:k, 3] == 255)
        prgba = np.zeros((pal.shape[0], 4), dtype=np.uint8)
        prgba[off:k, :3] = pal[off:k, :3]
        prgba[off:k, 3] = 255
        return np.ascontiguousarray(pal[off:k, :3]), off, prgba
    assert pal.shape[1] == 3 and transparent_index in (None, -1, 0)
    off = 1 if transparent_index == 0 else 0
    k = remap_ref.palette_rows(pal).shape[0]
    assert k > off
    prgba = np.zeros((pal.shape[0], 4), dtype=np.uint8)
    prgba[off:k, :3] = remap_ref.pal8(pal)[off:k]
    prgba[off:k, 3] = 255
    return np.ascontiguousarray(pal[off:k]), off, prgba


def remap_rgba(ob, image, palette, transparent_index=None, alpha_threshold=128, mode=RIEMERSMA, spread=None, want_gap=False):
    """image: (H, W, 4) or (F, H, W, 4) uint8.  Returns (map of the image's shape without the channels, int64; quantized (..., 4) uint8;
    for the nearest and the ordered mode with want_gap the smallest relative gap of `ordered_ref.remap` over ALL pixels, else None)."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim in (3, 4) and image.shape[-1] == 4
    frames = image if image.ndim == 4 else image[None]
    f, h, w, _ = frames.shape
    opaque_rows, off, prgba = split(palette, transparent_index)
    opaque = frames[..., 3].astype(np.int64) >= alpha_threshold
    assert off == 1 or opaque.all(), "a transparent pixel and no transparent entry"
    gap = None
    if mode == NEAREST:
        inner, _ = remap_ref.remap(ob, frames, opaque_rows, dither=False)
        if want_gap:
            gap = ordered_ref.remap(ob, frames, opaque_rows, 0.0)[2]
    elif mode == ORDERED:
        if spread is None:
            spread = ordered_ref.ordered_spread(opaque_rows)
        inner, _, gap = ordered_ref.remap(ob, frames, opaque_rows, spread)
    else:
        rows = remap_ref.palette_rows(opaque_rows)
        pmap = ob.unplanar(ob.convert("srgb_to_rec2020", ob.planar(rows)), rows.shape[0])
        inner = np.zeros((f, h, w), dtype=np.int64)
        for i in range(f):
            if max(w, h) <= 1:
                continue                                           # (a 1 x 1 walk visits nothing: entry 0 of the opaque rows)
            if opaque[i].all():
                inner[i] = remap_ref.remap(ob, frames[i], opaque_rows, dither=True)[0]
            elif opaque[i].any():
                px = frames[i, :, :, :3].reshape(h * w, 3).astype(np.float64) / 255.0
                img = ob.unplanar(ob.convert("srgb_to_rec2020", ob.planar(px)), h * w)
                inner[i] = rgba_ref.masked_dither(ob, img, w, h, pmap, opaque[i]).reshape(h, w)
    maps = np.where(opaque, off + inner, 0).astype(np.int64)
    quant = prgba[maps]
    if image.ndim == 3:
        return maps[0], quant[0], gap
    return maps, quant, gap
