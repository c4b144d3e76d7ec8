"""patolette_amd -- MI355X-native drop-in for big-nacho/patolette's `patolette.quantize()`.

Mirrors the reference's Python surface (src/patolette/patolette.pyx:324-344, 441-473):
`quantize(...)` with the same positional/keyword arguments, the same validation messages and
the same `(success, palette, palette_map, message)` return tuple, plus the `ColorSpace_*`
constants.  The work behind it runs in hand-written HIP kernels on gfx950 through the C ABI of
`libpatolette_amd.so` (include/patolette.h); there is no CPU fallback.

`tile_size > 0` derives the saliency weights on the GPU as the reference's binding does on the CPU
(patolette.pyx:203-313).  Additive (not in the reference): the `weights=` keyword (explicit
per-pixel weights instead of the saliency-derived ones), `saliency_weights`, `quantize_batch`, the 8-bit adaptor `quantize_u8` and its
batch form `quantize_u8_batch`, and `quantize_rgba` for RGBA images: a palette built from the visible pixels only, one reserved
transparent index, and a dither that walks past transparent pixels as the reference's walks past positions outside the image;
and `quantize_frames` for an animation: frames of one size that share one palette, each frame dithered along its own curve;
and `remap`, which makes no palette: it maps 8-bit images or frames onto a palette the caller gives (a fixed one, an earlier call's);
`dither="ordered"` (in `remap`, `quantize_u8`, `quantize_frames`) is a position-keyed Bayer dither for animations, `ordered_spread` its
default strength; and `frame_deltas`, which turns an animation's maps into what an encoder writes per frame: unchanged positions made
transparent, and the dirty rectangle; and `measure`, which tells what any of these maps costs -- per palette entry and per frame the
pixel count, the squared error in code values and its maximum, per frame also the squared ICtCp distance the palette was fitted to
and `frame_deltas`' tolerance is stated in -- with `psnr` to read it in decibels;
and, for animations with transparency, `remap_rgba` (RGBA images or frames onto a given palette whose row 0 may be a transparent
entry) and `quantize_rgba_frames` (one shared palette and one transparent index for all frames, composed from `quantize_rgba`'s
palette stage and `remap_rgba`) and `frame_deltas_rgba` (the deltas of such maps: 0 means "leave the canvas", every frame gets its
own disposal, and the rectangle also covers what the next frame makes transparent);
and `frame_deltas_local`, the deltas of a clip whose frames or scenes each have a palette of their own -- the canvas is a colour --
which `write_gif(palette_of=...)` writes with GIF local colour tables;
and `gif_lzw`, which LZW-compresses maps or deltas on the device, with `write_gif`, the GIF89a container around it, and `gif_lzw_lossy`
with `gif_neighbours`, the lossy coder that lets a nearly equal colour continue a dictionary match;
and `ColorHistogram`, for pixels that arrive in chunks (a long clip, a directory of images): an exact colour histogram kept on the
GPU and filled by any number of `add` calls, whose `palette()` is the one shared palette that `remap` then maps every chunk onto --
with `colors` ("how many colours does this have?") and an input of no more than K colours getting exactly those colours back.
"""
import ctypes as C
import types

import numpy as np

from . import _native
from ._native import last_stats, profile, profile_results  # noqa: F401

__version__ = "0.1.0"

# patolette.pyx:324-326
ColorSpace_sRGB = 0
ColorSpace_CIELuv = 1
ColorSpace_ICtCp = 2

# patolette.pyx:328-330
color_mismatch = "The number of colors doesn't match the supplied width and height."
bad_channel_count = 'Expected colors to be in sRGB[0, 1] space. Channel count mismatch: {} found.'
bad_tile_size = 'tile_size parameter expected to be in the range [0, inf]'



def _raise_saliency(code, message):
    """Exit codes of the saliency stage: the reference raises Python exceptions in the same situations
    (patolette.pyx:157-158 / :228-232 shape, numpy LinAlgError for a singular border covariance).  -7, the degenerate map, is the
    one case where the reference raises nothing: it goes on with all-NaN weights (0 / 0 at patolette.pyx:291)."""
    if code == -5 or code == -7:
        raise ValueError(message)
    if code == -6:
        raise np.linalg.LinAlgError("Singular matrix (%s)" % message)


def _dp(a):
    return a.ctypes.data_as(_native.dp) if a is not None and a.size > 0 else None


def quantize(width, height, colors, palette_size, dither=True, palette_only=False,
             color_space=ColorSpace_ICtCp, tile_size=512, kmeans_niter=32, kmeans_max_samples=512 ** 2,
             verbose=False, weights=None):
    """Quantise an image; reference `patolette.quantize` (patolette.pyx:332-466).

    colors: (width*height, 3) float64, sRGB in [0,1], row-scan pixel order.
    Returns (success, palette (K,3) F-ordered | None, palette_map (N,) uintp | None, message).
    """
    colors = np.asarray(colors)
    if colors.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % colors.ndim)
    color_count, channel_count = colors.shape
    # validations the reference does before crossing into C (patolette.pyx:351-373)
    if channel_count != 3:
        return (False, None, None, bad_channel_count.format(channel_count))
    if color_count != width * height:
        return (False, None, None, color_mismatch)
    if tile_size < 0:
        return (False, None, None, bad_tile_size)

    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != color_count:
            raise ValueError("weights must hold width*height values")

    opts = _native.QuantizationOptions(bool(dither), bool(palette_only), int(color_space), int(kmeans_niter),
                                       int(kmeans_max_samples), bool(verbose))
    # The reference transposes into planar R|G|B here (np.asfortranarray, patolette.pyx:388-391): ~60 ms for 16 MP.
    # An F-ordered float64 array goes to the planar entry as is; anything else is handed over row-major (at most a
    # dtype cast) and the first kernel reads it with stride 3.
    if colors.dtype == np.float64 and colors.flags.f_contiguous and not colors.flags.c_contiguous:
        data, entry = colors, "patolette_amd_quantize"
    else:
        data, entry = np.ascontiguousarray(colors, dtype=np.float64), "patolette_amd_quantize_rows"
    palette = np.zeros((palette_size, 3), dtype=np.float64, order='F')
    palette_map = None
    if not opts.palette_only:
        palette_map = np.zeros(width * height, dtype=np.uintp)
    exit_code = C.c_int(0)
    L = _native.lib()
    if verbose and tile_size > 0 and w is None:
        print('patolette ======== Generating saliency map')     # patolette.pyx:408-409
    # tile_size > 0 and no explicit weights: saliency weights derived on the device (patolette.pyx:407-414)
    getattr(L, entry)(width, height, _dp(data), _dp(w), float(tile_size), palette_size, C.byref(opts), _dp(palette),
                             palette_map.ctypes.data_as(_native.zp) if palette_map is not None and palette_map.size > 0 else None,
                             C.byref(exit_code))
    success = exit_code.value == 0
    message = L.get_patolette_exit_code_info_message(exit_code.value).decode('UTF-8')
    _raise_saliency(exit_code.value, message)
    if not success:
        return (success, None, None, message)
    if opts.palette_only:
        return (success, palette, None, message)
    return (success, palette, palette_map, message)


def set_kmeans_update(mode):
    """KMeans centroid update: 0 (default) = the reference's sequential f32 chains, bit for bit; 1 = order-free exact sums rounded
    once: faster and content-independent, but NOT the reference's result -- ~1e-6 of the colour range per iteration, ~1e-4 after
    the default 32 iterations at ~1000 members per centroid (outside the 1e-5 parity target), ~0.02 % of the index map follows
    (tests/test_gpu_kmeans_update.py).  Process-wide; returns the previous setting (include/patolette_amd.h:
    patolette_amd_set_kmeans_update).  Ignored for palettes beyond 4096 entries (the exact update runs)."""
    return int(_native.lib().patolette_amd_set_kmeans_update(int(mode)))


def saliency_weights(width, height, colors, tile_size=512):
    """The weights `quantize` derives when tile_size > 0 (reference `get_weights`, patolette.pyx:203-313),
    computed on the GPU.  colors as for `quantize`.  Returns width*height float64."""
    colors = np.asarray(colors)
    if colors.ndim != 2 or colors.shape[1] != 3 or colors.shape[0] != width * height:
        raise ValueError(color_mismatch)
    data = np.asfortranarray(colors, dtype=np.float64)
    out = np.zeros(width * height, dtype=np.float64)
    L = _native.lib()
    rc = L.patolette_amd_saliency_weights(width, height, _dp(data), float(tile_size), _dp(out))
    if rc == -2:
        _raise_saliency(-5, L.get_patolette_exit_code_info_message(-5).decode('UTF-8'))
    if rc == -3:
        _raise_saliency(-6, L.get_patolette_exit_code_info_message(-6).decode('UTF-8'))
    if rc == -4:
        _raise_saliency(-7, L.get_patolette_exit_code_info_message(-7).decode('UTF-8'))
    if rc != 0:
        raise RuntimeError(_native.last_error())
    return out


# ---- the 8-bit entries: each serves numpy arrays (host entry) and torch CUDA tensors (the `_device` entry: the image, the index map and
# the quantized image stay in HBM, the palettes are numpy arrays either way).  torch is only used to allocate those outputs and to
# order the call after the producer of the image.  Import torch BEFORE patolette_amd in such a process: both link a HIP runtime with
# the same SONAME and torch does not initialise on the one this library would otherwise load first.

def _is_cuda(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _u8_pixels(a, ndims, channels, wanted):
    """`a` as contiguous uint8 pixels -> (pixels, shape as ints, torch device or None for a numpy array); a ValueError asking for
    `wanted` (%s: "array" or "tensor") unless it is uint8 with len(shape) in ndims and shape[-1] in channels."""
    dev = a.device if _is_cuda(a) else None
    if dev is not None:
        import torch
        px, is_u8 = a.contiguous(), a.dtype == torch.uint8
    else:
        px = np.ascontiguousarray(a)
        is_u8 = px.dtype == np.uint8
    shape = tuple(int(v) for v in px.shape)
    if not is_u8 or len(shape) not in ndims or shape[-1] not in channels:
        raise ValueError(wanted % ("tensor" if dev is not None else "array"))
    return px, shape, dev


def _weights(weights, n, dev, what="width*height"):
    """None, or the weights as n contiguous float64 values where the pixels are (dev: see _u8_pixels)."""
    if weights is None:
        return None
    if dev is not None:
        import torch
        w = torch.as_tensor(weights, dtype=torch.float64, device=dev).reshape(-1).contiguous()
    else:
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != n:
        raise ValueError("weights must hold %s values" % what)
    return w


def _options(dither, palette_only, color_space, kmeans_niter, kmeans_max_samples):
    return _native.QuantizationOptions(bool(dither), bool(palette_only), int(color_space), int(kmeans_niter), int(kmeans_max_samples),
                                       False)


def _map_dtype(rows):
    return np.uint8 if rows <= 256 else (np.uint16 if rows <= 65536 else np.uint32)


def _outputs(shape, rows, channels, dev, want_map=True, want_quantized=True):
    """Zeroed (index map of `shape`, bytes per map element, quantized image of shape + (channels,)) next to the pixels; None for
    what is not wanted.  The map's elements: numpy uint8 / uint16 / uint32 by the palette's rows; torch uint8 / int32, as the
    kernels write them (the device entries convert no map)."""
    if dev is None:
        pmap = np.zeros(shape, dtype=_map_dtype(rows)) if want_map else None
        quant = np.zeros(shape + (channels,), dtype=np.uint8) if want_quantized else None
        return pmap, np.dtype(_map_dtype(rows)).itemsize, quant
    import torch
    pmap = torch.zeros(shape, dtype=torch.uint8 if rows <= 256 else torch.int32, device=dev) if want_map else None
    quant = torch.zeros(shape + (channels,), dtype=torch.uint8, device=dev) if want_quantized else None
    return pmap, 1 if rows <= 256 else 4, quant


def _vp(a):
    """The address of a numpy array or a torch tensor as the C ABI types it (double* for float64 arrays, else void*); None for
    None and for empty ones."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr()) if a.numel() > 0 else None
    if a.dtype == np.float64:
        return _dp(a)
    return a.ctypes.data_as(C.c_void_p) if a.size > 0 else None


def _call(name, dev, *args):
    """The C entry `name` for host arrays; `name`_device for a torch device, selected and with its current stream drained first
    (the library runs on its own stream)."""
    L = _native.lib()
    if dev is None:
        return getattr(L, name)(*args)
    import torch
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        return getattr(L, name + "_device")(*args)


def _message(code):
    return _native.lib().get_patolette_exit_code_info_message(code).decode('UTF-8')


def _u8_result(code, palette_u8, pmap, quant, palette):
    message = _message(code)
    _raise_saliency(code, message)
    if code != 0:
        return (False, None, None, None, None, message)
    return (True, palette_u8, pmap, quant, palette, message)


def _quantize_stack(name, lead, px, shape, dev, w, tile_size, palette_size, opts, palette, want_quantized, want_map=True):
    """patolette_amd_u8 (lead = ()) and patolette_amd_frames_u8 (lead = (frames,)) on pixels of `shape` = (..., H, W, channels).
    Neither map nor quantized image wanted, palette_only unset: the palettes as the full call returns them (in sRGB), no map stage."""
    height, width, channels = shape[-3:]
    palette_u8 = np.zeros((max(palette_size, 0), 3), dtype=np.uint8)
    pmap, map_elem, quant = _outputs(shape[:-1], palette_size, 3, dev, want_map and not opts.palette_only,
                                     want_quantized and not opts.palette_only)
    code = C.c_int(0)
    _call(name, dev, *lead, width, height, _vp(px), channels, _vp(w), float(tile_size), palette_size, C.byref(opts), _vp(palette),
          _vp(palette_u8), _vp(pmap), map_elem, _vp(quant), C.byref(code))
    return _u8_result(code.value, palette_u8, pmap, quant, palette)


def quantize_u8(image, palette_size, dither=True, palette_only=False, color_space=ColorSpace_ICtCp, tile_size=512,
                kmeans_niter=32, kmeans_max_samples=512 ** 2, weights=None, want_quantized=True, spread=None):
    """8-bit adaptor (additive): `image` is an (H, W, 3|4) uint8 sRGB array as an image
    decoder returns it, or a torch CUDA tensor of that shape (then nothing but the palettes crosses PCIe).  Does on the GPU what callers of the reference do by hand around `quantize`
    (README.md:147-194): `colors = img/255`, `palette_u8 = clip(palette*255).astype(uint8)` and
    `quantized = palette_u8[palette_map]`; 3 bytes per pixel cross PCIe instead of 24.

    dither="ordered" (with `spread`, see `remap`): composed in Python from two calls -- the palette this call returns with
    dither=False (made without the map stage), then `remap(image, palette, dither="ordered", spread=spread)` with that float
    palette.  A host array is uploaded twice (once per call); a tensor is not copied at all.

    Returns (success, palette_u8 (K,3) uint8, palette_map (H,W) uint8|uint16|uint32 or None,
    quantized (H,W,3) uint8 or None, palette (K,3) float64 as `quantize` returns it, message)."""
    ordered, spread = isinstance(dither, str) and _dither_mode(dither) == 2, _spread_value(spread)   # (any other string: a ValueError)
    px, shape, dev = _u8_pixels(image, (3,), (3, 4), "image must be an (H, W, 3|4) uint8 %s")
    # (unlike its siblings: no tile_size < 0 check -- a negative one derives no weights -- and the palette's rows are not clamped)
    w = _weights(weights, shape[0] * shape[1], dev)
    palette = np.zeros((palette_size, 3), dtype=np.float64, order='F')
    res = _quantize_stack("patolette_amd_u8", (), px, shape, dev, w, tile_size, palette_size,
                          _options(dither and not ordered, palette_only, color_space, kmeans_niter, kmeans_max_samples), palette,
                          want_quantized and not ordered, want_map=not ordered)
    return _then_ordered(res, px, spread, want_quantized) if ordered and not palette_only else res


def quantize_frames(frames, palette_size, dither=True, palette_only=False, color_space=ColorSpace_ICtCp, tile_size=512,
                    kmeans_niter=32, kmeans_max_samples=512 ** 2, weights=None, want_quantized=True, spread=None):
    """Quantise an animation (additive; include/patolette_amd.h: patolette_amd_frames_u8): `frames` is an (F, H, W, 3|4) uint8 sRGB
    array, or a torch CUDA tensor of that shape (then the maps and the quantized frames stay in HBM, as in `quantize_u8`).  All
    frames share ONE palette; every frame gets its own index map.

      * Palette: what `quantize` computes (up to and including the KMeans refinement) for the F*H*W pixels of the frames laid one
        after another; `kmeans_max_samples` applies to all of them.
      * Maps: each frame mapped on its own with that palette -- the nearest entry, or with `dither` the reference's Riemersma walk
        over that frame's own W x H curve from an empty error queue.  No state passes between frames.
      * weights: None or F*H*W values in frame order.  tile_size > 0 without weights: every frame gets the saliency weights
        `quantize_u8` derives for it as an image of its own.
    F == 1 is `quantize_u8` of that image; without dithering the result equals `quantize_u8` of the frames stacked into one
    (F*H, W) image; with dithering the palette equals that call's, the maps do not (one curve would run through all frames).

    Returns (success, palette_u8 (K,3) uint8, maps (F,H,W) uint8|uint16|uint32 or None, quantized (F,H,W,3) uint8 or None
    (= palette_u8[maps]), palette (K,3) float64 as `quantize` returns it, message).

    dither="ordered" (with `spread`, see `remap`) is the mode made for animations: a choice depends on the pixel and its position
    only, so frames that barely differ get maps that barely differ.  It is composed in Python from two calls -- the palette this
    call returns with dither=False (made without the map stage), then `remap(frames, palette, dither="ordered", spread=spread)`
    with that float palette.  A host array is uploaded twice (once per call); a tensor is not copied at all."""
    ordered, spread = isinstance(dither, str) and _dither_mode(dither) == 2, _spread_value(spread)   # (any other string: a ValueError)
    px, shape, dev = _u8_pixels(frames, (4,), (3, 4), "frames must be an (F, H, W, 3|4) uint8 %s")
    if tile_size < 0:
        raise ValueError(bad_tile_size)
    w = _weights(weights, shape[0] * shape[1] * shape[2], dev, "frames*width*height")
    palette = np.zeros((max(palette_size, 0), 3), dtype=np.float64, order='F')
    res = _quantize_stack("patolette_amd_frames_u8", shape[:1], px, shape, dev, w, tile_size, palette_size,
                          _options(dither and not ordered, palette_only, color_space, kmeans_niter, kmeans_max_samples), palette,
                          want_quantized and not ordered, want_map=not ordered)
    return _then_ordered(res, px, spread, want_quantized) if ordered and not palette_only else res


def _remap_palette(palette):
    """(K, 3) uint8 -> (bytes array, None); (K, 3) float -> (None, column-major float64)."""
    pal = np.asarray(palette)
    if pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
        raise ValueError("palette must be a (K, 3) uint8 or float array with at least one row")
    if pal.dtype == np.uint8:
        return np.ascontiguousarray(pal), None
    if pal.dtype.kind != "f":                                  # (other integers would be read as sRGB values far outside [0, 1])
        raise ValueError("palette must be a (K, 3) uint8 or float array with at least one row")
    return None, np.asfortranarray(pal, dtype=np.float64)


def _palette_rows(pal8, palf):
    """The used rows of _remap_palette's result as (k, 3) float64 sRGB: bytes / 255, or the float rows without the trailing fill."""
    if pal8 is not None:
        return pal8.astype(np.float64) / 255.0
    k = palf.shape[0]
    while k > 0 and np.all(palf[k - 1] == -1.0):
        k -= 1
    return np.ascontiguousarray(palf[:k])


def ordered_spread(palette):
    """The default strength of the ordered dither for `palette` ((K, 3) uint8 or float, taken as `remap` takes it): the mean over the
    used rows of the Euclidean sRGB distance to the nearest OTHER row, divided by sqrt(3).  A grey shift of s per channel moves a
    colour by s * sqrt(3), so this is the palette's typical per-channel step: exactly 1/3 for four evenly spaced greys, where 1/3 is
    the optimum.  A one-row palette gives 0.0.  Pure numpy; no GPU."""
    rows = _palette_rows(*_remap_palette(palette))
    k = rows.shape[0]
    if k < 2:
        return 0.0
    nearest = np.empty(k)
    for a in range(0, k, 1024):                                    # (blocks of rows: K x K distances at once is too much for large K)
        d2 = np.sum((rows[a:a + 1024, None, :] - rows[None, :, :]) ** 2, axis=2)
        d2[np.arange(d2.shape[0]), a + np.arange(d2.shape[0])] = np.inf
        nearest[a:a + 1024] = np.sqrt(np.min(d2, axis=1))
    return float(np.mean(nearest) / np.sqrt(3.0))


def _dither_mode(dither):
    """0 nearest, 1 Riemersma, 2 ordered for dither = False, True, "ordered"; anything else is a ValueError."""
    if isinstance(dither, str):
        if dither == "ordered":
            return 2
    elif isinstance(dither, (bool, int, np.bool_, np.integer)) and dither in (0, 1):
        return int(dither)
    raise ValueError('dither must be True, False or "ordered"')


def _spread_value(spread):
    """None, or `spread` as a float: finite and not negative, else a ValueError."""
    if spread is None:
        return None
    try:
        value = float(spread)
    except (TypeError, ValueError):
        raise ValueError("spread must be None or a finite number >= 0") from None
    if not (np.isfinite(value) and value >= 0.0):
        raise ValueError("spread must be None or a finite number >= 0")
    return value


def _then_ordered(res, pixels, spread, want_quantized):
    """dither="ordered" of quantize_u8 / quantize_frames: `res` is that call's return tuple with dither=False and no map stage; the
    ordered remap of the same pixels onto its float palette fills in the map and the quantized image.  (Not the palette_only palette:
    as in the reference, that one stays in the quantisation's colour space; this one has been through the way back to sRGB.  With
    color_space sRGB it is what dither=False returns there, the reference's ICtCp -> sRGB of rows that never were ICtCp.)"""
    if not res[0]:
        return res
    _, palette_u8, _, _, palette, _ = res
    ok, pmap, quant, message = remap(pixels, palette, dither="ordered", want_quantized=want_quantized, spread=spread)
    if not ok:
        return (False, None, None, None, None, message)
    return (True, palette_u8, pmap, quant, palette, message)


def remap(image, palette, dither=True, want_quantized=True, spread=None):
    """Map an 8-bit image, or frames of one size, onto a palette the caller gives (additive; include/patolette_amd.h:
    patolette_amd_remap_u8, patolette_amd_remap_ordered_u8).  No palette is made.

      * image: (H, W, 3|4) or (F, H, W, 3|4) uint8 sRGB, a numpy array or a torch CUDA tensor (then the map and the quantized
        image stay in HBM, as in `quantize_u8`).  A 4th channel is ignored.
      * palette: (K, 3) uint8 (entry = v / 255, as the pixels), or (K, 3) float sRGB in any layout -- so both `palette_u8` and
        `palette` of every return tuple of this module can be passed straight in.  Trailing (-1, -1, -1) rows of a float palette
        (unused rows) are dropped; indices are row numbers of the palette as given.
      * dither=False: the nearest entry in ICtCp; dither=True: the reference's Riemersma walk in linear Rec2020 over each frame's own
        W x H curve from an empty error queue.  No state passes between frames: remap(frames, p)[1][i] == remap(frames[i], p)[1].
      * dither="ordered": the mode for animations.  Every pixel's R, G and B are shifted by the same spread * t, t in (-0.5, 0.5)
        from the 8x8 Bayer matrix at the pixel's place in its own frame, then the nearest entry in ICtCp is taken (the header has the
        exact definition).  A choice depends on the pixel and its position only, so a small change of a frame changes few indices,
        where the Riemersma walk re-rolls the rest of the frame.  spread=None takes `ordered_spread(palette)`; spread=0 is
        dither=False bit for bit.  `spread` is read in this mode only; it must be finite and not negative.
    Remapping a call's quantized image onto that call's `palette_u8` gives back its map.  Remapping the ORIGINAL image onto the float
    palette a `quantize*` call returned is close to, not bit for bit, that call's map (the header says why).

    Returns (success, palette_map (H,W) or (F,H,W) uint8|uint16|uint32 by K, quantized (..., 3) uint8 = pal8[palette_map] or None,
    message)."""
    mode, spread = _dither_mode(dither), _spread_value(spread)
    px, shape, dev = _u8_pixels(image, (3, 4), (3, 4), "image must be an (H, W, 3|4) or (F, H, W, 3|4) uint8 %s")
    if dev is not None and hasattr(palette, "detach"):            # (a tensor image may come with a tensor palette: that one is host data)
        palette = palette.detach().cpu().numpy()
    pal8, palf = _remap_palette(palette)
    if mode == 2 and spread is None:
        spread = ordered_spread(pal8 if pal8 is not None else palf)
    count, (height, width), channels = (shape[0] if len(shape) == 4 else 1), shape[-3:-1], shape[-1]
    rows = (pal8 if pal8 is not None else palf).shape[0]
    pmap, map_elem, quant = _outputs(shape[:-1], rows, 3, dev, True, want_quantized)
    code = C.c_int(0)
    if mode == 2:
        _call("patolette_amd_remap_ordered_u8", dev, count, width, height, _vp(px), channels, _vp(palf), _vp(pal8), rows, spread,
              _vp(pmap), map_elem, _vp(quant), C.byref(code))
    else:
        _call("patolette_amd_remap_u8", dev, count, width, height, _vp(px), channels, _vp(palf), _vp(pal8), rows, mode,
              _vp(pmap), map_elem, _vp(quant), C.byref(code))
    if code.value == -1 and _native.last_error().startswith("patolette_amd_remap:"):
        raise ValueError(_native.last_error())
    message = _message(code.value)
    if code.value != 0:
        return (False, None, None, message)
    return (True, pmap, quant, message)


def _delta_maps(maps):
    """`maps` as contiguous (F, H, W) index maps -> (maps, shape, torch device or None, bytes per element, largest index an element
    holds); numpy uint8 / uint16 / uint32, or a torch uint8 / int32 CUDA tensor (what the device entries write)."""
    dev = maps.device if _is_cuda(maps) else None
    if dev is not None:
        import torch
        m = maps.contiguous()
        sizes = {torch.uint8: (1, 255), torch.int32: (4, 2 ** 31 - 1)}
        elem = sizes.get(m.dtype)
    else:
        m = np.ascontiguousarray(maps)
        elem = (m.dtype.itemsize, int(np.iinfo(m.dtype).max)) if m.dtype in (np.uint8, np.uint16, np.uint32) else None
    shape = tuple(int(v) for v in m.shape)
    if elem is None or len(shape) != 3:
        raise ValueError("maps must be an (F, H, W) uint8 / uint16 / uint32 array or a uint8 / int32 CUDA tensor")
    return m, shape, dev, elem[0], elem[1]


def _delta_row_count(palette, tol):
    """`palette` given as a plain int row count (tolerance 0 only, which reads no colours) -> the count; None for a palette."""
    if not isinstance(palette, (int, np.integer)) or isinstance(palette, (bool, np.bool_)):
        return None
    if tol > 0.0:
        raise ValueError("a tolerance above 0 compares colours: pass the palette itself, not its row count")
    if int(palette) < 1:
        raise ValueError("the palette's row count must be at least 1")
    return int(palette)


def _delta_setup(maps, tolerance, frames, want_shown, palette_rules):
    """What `frame_deltas` and `frame_deltas_rgba` do around their own palette rules, in the order their errors have always come: the
    maps, the tolerance, then palette_rules(tol, elem, elem_max) -> (pal8, palf, rows), then the frames against the maps.  The exact
    mode drops what it does not read; the outputs are allocated where the maps live.  Returns a namespace of what the entry takes."""
    m, shape, dev, elem, elem_max = _delta_maps(maps)
    try:
        tol = float(tolerance)
    except (TypeError, ValueError):
        raise ValueError("tolerance must be a finite number >= 0") from None
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("tolerance must be a finite number >= 0")
    pal8, palf, rows = palette_rules(tol, elem, elem_max)
    px, channels = None, 3
    if frames is not None:
        px, pshape, pdev = _u8_pixels(frames, (4,), (3, 4), "frames must be an (F, H, W, 3|4) uint8 %s")
        if pshape[:3] != shape:
            raise ValueError("frames of shape %s do not match maps of shape %s" % (pshape, shape))
        if pdev != dev:
            raise ValueError("frames and maps must live in the same place (both numpy arrays, or tensors of one device)")
        channels = pshape[3]
    if tol > 0.0 and px is None:
        raise ValueError("a tolerance above 0 needs the frames' pixels: pass frames=")
    if tol == 0.0:
        px = pal8 = palf = None                                   # (the exact mode reads none of them)
    if dev is None:
        deltas = np.zeros(shape, dtype=m.dtype)
        shown = np.zeros(shape, dtype=m.dtype) if want_shown else None
    else:
        import torch
        deltas = torch.zeros(shape, dtype=m.dtype, device=dev)
        shown = torch.zeros(shape, dtype=m.dtype, device=dev) if want_shown else None
    count, height, width = shape
    return types.SimpleNamespace(m=m, dev=dev, elem=elem, count=count, width=width, height=height, rows=rows, px=px, channels=channels,
                                 pal8=pal8, palf=palf, tol=tol, deltas=deltas, shown=shown, rects=np.zeros((count, 4), dtype=np.int32),
                                 changed=np.zeros(count, dtype=np.uint64), code=C.c_int(0))


def _delta_message(name, code):
    """The entry's own complaints about its arguments are the caller's mistake: a ValueError.  Otherwise the code's message."""
    if code == -1 and _native.last_error().startswith(name + ":"):
        raise ValueError(_native.last_error())
    return _message(code)


def frame_deltas(maps, palette, transparent_index=None, frames=None, tolerance=0.0, want_shown=False):
    """The inter-frame deltas of an animation's index maps (additive; include/patolette_amd.h: patolette_amd_frame_deltas): what a
    GIF or APNG encoder makes of every frame -- the map with "same as what is already on screen" replaced by a transparent index, and
    the dirty rectangle -- without the maps leaving the GPU.

      * maps: (F, H, W) uint8 / uint16 / uint32 numpy array as `quantize_frames` / `remap` return it, or a torch uint8 / int32 CUDA
        tensor (then the deltas and the shown maps stay on its device).
      * palette: what `remap` takes ((K, 3) uint8 or float), or a plain int row count (allowed with tolerance 0 only, which reads
        no colours).
      * transparent_index: an index no palette entry uses; default K.  It must fit the maps' element type: uint8 maps of a 256-row
        palette have no free index -- make the palette with one row less (`quantize_frames(frames, 255, ...)`).
      * tolerance 0: a position is transparent in frame f iff its index equals what the canvas shows there.  tolerance > 0 (lossy,
        the largest lever on GIF size): the displayed entry also stays while it lies within `tolerance` (ICtCp, Euclidean) of the
        frame's SOURCE pixel, so `frames` -- the (F, H, W, 3|4) uint8 pixels, where the maps live -- is required; the comparison is
        always with the current source, so no error accumulates.
      * want_shown: also return what the canvas shows after every frame (== maps when tolerance is 0).
    Frame 0 is the full first map.  Compositing the deltas (overwrite where delta != transparent_index) gives back `shown`.
    `write_gif(file, deltas, palette, rects, transparent_index=...)` writes them as a GIF.
    Maps that carry a transparent entry of their own (`remap_rgba`, `quantize_rgba_frames`) go to `frame_deltas_rgba`: 0 as the
    deltas' transparent index, a disposal per frame, and the lossy mode (here their index 0 compares like any row).

    Returns (success, deltas (F,H,W) as maps, rects (F,4) int32 rows (x0, y0, w, h) -- (0,0,0,0) for an unchanged frame --,
    changed (F,) int64, shown (F,H,W) or None, message)."""
    T = None

    def palette_rules(tol, elem, elem_max):
        nonlocal T
        pal8 = palf = None
        rows = _delta_row_count(palette, tol)
        if rows is None:
            pal8, palf = _remap_palette(palette.detach().cpu().numpy() if hasattr(palette, "detach") else palette)
            rows = (pal8 if pal8 is not None else palf).shape[0]
        T = rows if transparent_index is None else int(transparent_index)
        if T < rows:
            raise ValueError("transparent_index must be at least the palette's row count (%d): an index no entry uses" % rows)
        if T > elem_max:
            raise ValueError("no free index: transparent_index %d does not fit the maps' %d-byte elements -- make the palette with one row "
                             "less, or pass wider maps" % (T, elem))
        return pal8, palf, rows

    d = _delta_setup(maps, tolerance, frames, want_shown, palette_rules)
    _call("patolette_amd_frame_deltas", d.dev, d.count, d.width, d.height, _vp(d.m), d.elem, d.rows, T, _vp(d.px), d.channels, _vp(d.palf),
          _vp(d.pal8), d.tol, _vp(d.deltas), _vp(d.shown), d.rects.ctypes.data_as(C.POINTER(C.c_int32)),
          d.changed.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(d.code))
    message = _delta_message("patolette_amd_frame_deltas", d.code.value)
    if d.code.value != 0:
        return (False, None, None, None, None, message)
    return (True, d.deltas, d.rects, d.changed.astype(np.int64), d.shown, message)


def _local_tables(palettes, palette_of, count, max_rows, name="palettes"):
    """Per-frame palettes as the contiguous (P, K, 3) uint8 stack and the frames' tables as (count,) int32: `palette_of` None means
    frame f takes table f, which needs P == count."""
    pal = np.asarray(palettes.detach().cpu().numpy() if hasattr(palettes, "detach") else palettes)
    if pal.ndim != 3 or pal.shape[2] != 3 or pal.dtype != np.uint8 or pal.shape[0] < 1 or pal.shape[1] < 1:
        raise ValueError("%s must be a (P, K, 3) uint8 array: P tables of K rows" % name)
    if pal.shape[1] > max_rows:
        raise ValueError("a GIF colour table holds at most 256 rows" if max_rows == 256 else
                         "every table may have at most %d rows: a one-byte map needs an index no table uses" % max_rows)
    if pal.shape[0] > 65536:
        raise ValueError("%s may hold at most 65536 tables" % name)
    if palette_of is None:
        if pal.shape[0] != count:
            raise ValueError("without palette_of every frame has its own table: %d tables do not match %d frames" % (pal.shape[0], count))
        of = np.arange(count, dtype=np.int32)
    else:
        of = np.asarray(palette_of.detach().cpu().numpy() if hasattr(palette_of, "detach") else palette_of)
        if of.shape != (count,) or of.dtype.kind not in "iu" or of.dtype == np.bool_:
            raise ValueError("palette_of must be None or %d integers, the table of every frame" % count)
        if np.any(of < 0) or np.any(of >= pal.shape[0]):
            raise ValueError("every palette_of value must lie in [0, %d), the number of tables" % pal.shape[0])
        of = np.ascontiguousarray(of.astype(np.int32))
    return np.ascontiguousarray(pal), of


def frame_deltas_local(maps, palettes, palette_of=None, transparent_index=None, frames=None, tolerance=0.0, want_shown=False):
    """`frame_deltas` for a clip whose frames, or scenes, each have a palette of their own (additive; include/patolette_amd.h:
    patolette_amd_frame_deltas_local) -- what `quantize_u8_batch` or `quantize_frames` per scene return.  Indices of two tables do not
    compare, so the canvas is a colour, as a viewer's is: a position is transparent in frame f iff its entry's three bytes equal the
    colour on the canvas (tolerance 0), or the colour on the canvas lies within `tolerance` (ICtCp) of the frame's source pixel.

      * maps: (F, H, W) uint8 numpy array, or a torch uint8 CUDA tensor (then the deltas and the shown colours stay on its device).
      * palettes: (P, K, 3) uint8, K <= 255: P tables of K rows.
      * palette_of: None (frame f is drawn with table f; P == F), or F integers in [0, P): the table of every frame -- a palette
        per scene is `palette_of=[0, 0, 0, 1, 1, 1]`.
      * transparent_index: the one index no table uses, K <= T <= 255, the same in every frame; default K.
      * frames, tolerance: as `frame_deltas` takes them.
      * want_shown: also return what a viewer shows after every frame, as colours.
    Drawing deltas[f] with table palette_of[f] over the canvas, skipping the transparent index, shows shown_rgb[f]; at tolerance 0 that
    is the frame's own colours.  With one table whose rows are all distinct the deltas are `frame_deltas`' own.
    `write_gif(file, deltas, palettes, rects, transparent_index=T, palette_of=palette_of)` writes them with local colour tables.
    Out of scope: maps with a transparent entry of their own and per-frame disposal (a local `frame_deltas_rgba`); APNG, which has one
    PLTE; `measure` across tables (measure per group of frames, or compare `shown_rgb` with the source).

    Returns (success, deltas (F,H,W) uint8, rects (F,4) int32, changed (F,) int64, shown_rgb (F,H,W,3) uint8 or None, message)."""
    T, pal, of = None, None, None

    def palette_rules(tol, elem, elem_max):
        nonlocal T, pal, of
        if elem != 1:
            raise ValueError("maps must be uint8: a GIF colour table has at most 256 rows")
        pal, of = _local_tables(palettes, palette_of, int(maps.shape[0]), 255)
        rows = pal.shape[1]
        if transparent_index is not None and (isinstance(transparent_index, (bool, np.bool_)) or not isinstance(transparent_index, (int, np.integer))):
            raise ValueError("transparent_index must be None or an integer")
        T = rows if transparent_index is None else int(transparent_index)
        if not rows <= T <= 255:
            raise ValueError("transparent_index must lie in [%d, 255]: an index no table uses, in a one-byte element" % rows)
        return None, None, rows

    d = _delta_setup(maps, tolerance, frames, False, palette_rules)
    shown = None
    if want_shown:
        shape = (d.count, d.height, d.width, 3)
        if d.dev is None:
            shown = np.zeros(shape, dtype=np.uint8)
        else:
            import torch
            shown = torch.zeros(shape, dtype=torch.uint8, device=d.dev)
    _call("patolette_amd_frame_deltas_local", d.dev, d.count, d.width, d.height, _vp(d.m), _vp(pal), pal.shape[0], d.rows,
          of.ctypes.data_as(C.POINTER(C.c_int32)), T, _vp(d.px), d.channels, d.tol, _vp(d.deltas), _vp(shown),
          d.rects.ctypes.data_as(C.POINTER(C.c_int32)), d.changed.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(d.code))
    message = _delta_message("patolette_amd_frame_deltas_local", d.code.value)
    if d.code.value != 0:
        return (False, None, None, None, None, message)
    return (True, d.deltas, d.rects, d.changed.astype(np.int64), shown, message)


def frame_deltas_rgba(maps, palette, frames=None, tolerance=0.0, loop=True, want_shown=False, transparent_index=None):
    """`frame_deltas` for maps whose index 0 is the transparent entry -- those of `remap_rgba` / `quantize_rgba_frames` (additive;
    include/patolette_amd.h: patolette_amd_frame_deltas_rgba).  In the deltas 0 means "leave the canvas as it is", which is what a GIF
    decoder does with the transparent index under disposal 1, so no free index is needed.  A pixel that turns from opaque to
    transparent cannot be drawn over the canvas: the frame before it gets disposal 2 over a rectangle that covers the pixel, and what
    was unchanged inside that rectangle is drawn again.  Every frame so has its own disposal (1 or 2) and a rectangle that holds its
    changed positions and the positions that vanish in the next frame.

      * maps: (F, H, W) uint8 / uint16 / uint32 numpy array, or a torch uint8 / int32 CUDA tensor, as in `frame_deltas`.
      * palette: as `remap_rgba` takes it -- (K, 4) uint8 RGBA whose row 0 has alpha 0, or (K, 3) uint8 / float with
        transparent_index=0 -- or a plain int row count (tolerance 0 only).  Row 0's colour is never read.  A palette without a
        transparent entry is a ValueError: such maps go to `frame_deltas`.
      * frames, tolerance, want_shown: as in `frame_deltas`; frames are (F, H, W, 3|4) uint8 (the alpha byte is not read: the maps
        say what is transparent).  The lossy mode never changes whether a position is transparent.
      * loop: whether the animation repeats: then the last frame's disposal and rectangle look at frame 0.
    `write_gif(file, deltas, palette_rgba[:, :3], rects, transparent_index=0, disposal=disposals)` writes the result as a GIF; a viewer
    then shows `shown` (== maps when tolerance is 0), on every pass of the loop.

    Returns (success, deltas (F,H,W) as maps, rects (F,4) int32 rows (x0, y0, w, h) -- (0,0,0,0) for a frame that changes and clears
    nothing --, disposals (F,) int32 of 1 or 2, changed (F,) int64, shown (F,H,W) or None, message)."""
    no_entry = "the palette has no transparent entry: maps without one go to frame_deltas"

    def palette_rules(tol, elem, elem_max):
        if not isinstance(loop, (bool, np.bool_)) and not (isinstance(loop, (int, np.integer)) and int(loop) in (0, 1)):
            raise ValueError("loop must be True or False")
        pal8 = palf = None
        rows = _delta_row_count(palette, tol)
        if rows is not None:
            if transparent_index is not None:                     # (a row count has no alpha column: row 0 is the entry unless told otherwise)
                if isinstance(transparent_index, (bool, np.bool_)) or not isinstance(transparent_index, (int, np.integer)) \
                        or int(transparent_index) not in (-1, 0):
                    raise ValueError("transparent_index must be None, -1 (no transparent entry) or 0 (row 0)")
                if int(transparent_index) == -1:
                    raise ValueError(no_entry)
        else:
            pal8, palf, _, tidx, _ = _rgba_palette(palette.detach().cpu().numpy() if hasattr(palette, "detach") else palette, transparent_index)
            if tidx != 0:
                raise ValueError(no_entry)
            rows = (pal8 if pal8 is not None else palf).shape[0]
        return pal8, palf, rows

    d = _delta_setup(maps, tolerance, frames, want_shown, palette_rules)
    disposals = np.zeros(d.count, dtype=np.int32)
    _call("patolette_amd_frame_deltas_rgba", d.dev, d.count, d.width, d.height, _vp(d.m), d.elem, d.rows, _vp(d.px), d.channels, _vp(d.palf),
          _vp(d.pal8), d.tol, 1 if loop else 0, _vp(d.deltas), _vp(d.shown), d.rects.ctypes.data_as(C.POINTER(C.c_int32)),
          disposals.ctypes.data_as(C.POINTER(C.c_int32)), d.changed.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(d.code))
    message = _delta_message("patolette_amd_frame_deltas_rgba", d.code.value)
    if d.code.value != 0:
        return (False, None, None, None, None, None, message)
    return (True, d.deltas, d.rects, disposals, d.changed.astype(np.int64), d.shown, message)


def measure(image, maps, palette, skip_index=None, ictcp=True):
    """What a map costs, per palette entry and per frame (additive; include/patolette_amd.h: patolette_amd_measure) -- the error of
    any map on 8-bit pixels, computed where the pixels and the maps are.

      * image: (H, W, 3|4) or (F, H, W, 3|4) uint8 sRGB, a numpy array or a torch CUDA tensor.  A 4th channel is ignored.
      * maps: (H, W) or (F, H, W) index maps in the element types `frame_deltas` accepts (numpy uint8 / uint16 / uint32, torch uint8 /
        int32), in the same place as the image: a map of `remap` / `quantize_*`, the `shown` of a lossy `frame_deltas`, its deltas.
      * palette: what `remap` takes, (K, 3) uint8 or float; trailing (-1, -1, -1) rows of a float one are dropped.
      * skip_index: positions whose element equals it enter nothing -- the transparent index of `frame_deltas`' deltas, index 0 of a
        `quantize_rgba` map.  It may name a palette row.  Every other element must be a used row (else a ValueError).
      * ictcp=False leaves out the ICtCp part: no pixel is converted.

    Returns (success, entries (K, 3) int64, per_frame (F, 3) int64, ictcp (F, 2) float64 or None, message).  The columns of entries
    and per_frame are count, sse, max_se: how many positions, the sum and the largest of their squared errors
    e = sum_c (pixel[c] - pal8[index][c])^2 in code values, pal8 being the bytes `quantized` is made of -- all exact integers.  The
    columns of ictcp are d_sum, d_max: sum and largest of the squared ICtCp distance D between the pixel and its entry, the D of
    `frame_deltas`' tolerance (compare d_max with tolerance ** 2); d_sum has the same bits on every call with the same arguments.
    The results are small and always numpy arrays.  `psnr` turns entries or per_frame into decibels."""
    px, shape, dev = _u8_pixels(image, (3, 4), (3, 4), "image must be an (H, W, 3|4) or (F, H, W, 3|4) uint8 %s")
    if not hasattr(maps, "shape") or len(maps.shape) not in (2, 3):
        raise ValueError("maps must be an (H, W) or (F, H, W) uint8 / uint16 / uint32 array or a uint8 / int32 CUDA tensor")
    m, mshape, mdev, elem, elem_max = _delta_maps(maps if len(maps.shape) == 3 else maps[None])
    given = shape
    if len(shape) == 3:
        shape = (1,) + shape
    if mshape != shape[:3] or len(maps.shape) + 1 != len(given):
        raise ValueError("maps of shape %s do not match an image of shape %s" % (tuple(maps.shape), given))
    if mdev != dev:
        raise ValueError("image and maps must live in the same place (both numpy arrays, or tensors of one device)")
    if hasattr(palette, "detach"):
        palette = palette.detach().cpu().numpy()
    pal8, palf = _remap_palette(palette)
    rows = (pal8 if pal8 is not None else palf).shape[0]
    skip = -1
    if skip_index is not None:
        if isinstance(skip_index, (bool, np.bool_)) or not isinstance(skip_index, (int, np.integer)) or int(skip_index) < 0:
            raise ValueError("skip_index must be None or an index >= 0")
        skip = int(skip_index)
        if skip > elem_max:
            skip = -1                                              # (no element can hold it: nothing is skipped)
    count, height, width, channels = shape
    ent = [np.zeros(rows, dtype=np.uint64), np.zeros(rows, dtype=np.uint64), np.zeros(rows, dtype=np.uint32)]
    per = [np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint32)]
    dist = np.zeros((2, count), dtype=np.float64) if ictcp else None
    u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    code = C.c_int(0)
    _call("patolette_amd_measure", dev, count, width, height, _vp(px), channels, _vp(m), elem, _vp(palf), _vp(pal8), rows, skip,
          ent[0].ctypes.data_as(u64), ent[1].ctypes.data_as(u64), ent[2].ctypes.data_as(u32),
          per[0].ctypes.data_as(u64), per[1].ctypes.data_as(u64), per[2].ctypes.data_as(u32),
          dist[0].ctypes.data_as(_native.dp) if ictcp else None, dist[1].ctypes.data_as(_native.dp) if ictcp else None, C.byref(code))
    if code.value == -1 and _native.last_error().startswith("patolette_amd_measure:"):
        raise ValueError(_native.last_error())
    message = _message(code.value)
    if code.value != 0:
        return (False, None, None, None, message)
    return (True, np.stack([a.astype(np.int64) for a in ent], axis=1), np.stack([a.astype(np.int64) for a in per], axis=1),
            np.ascontiguousarray(dist.T) if ictcp else None, message)


def psnr(stats):
    """Peak signal-to-noise ratio in dB of `measure`'s entries or per_frame ((.., 3) rows of count, sse, max_se; or one such row):
    10 * log10(3 * 255^2 * count / sse) -- inf where sse is 0, nan where count is 0.  Pure numpy; no GPU."""
    s = np.asarray(stats)
    if s.ndim < 1 or s.shape[-1] != 3:
        raise ValueError("psnr takes rows of (count, sse, max_se) as `measure` returns them")
    count, sse = s[..., 0].astype(np.float64), s[..., 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 10.0 * np.log10(3.0 * 255.0 * 255.0 * count / sse)
    out = np.where(count == 0, np.nan, np.where(sse == 0, np.inf, out))
    return out if out.ndim else float(out)


def _gif_rects(rects, count, height, width):
    """`rects` as (count, 4) int32 rows (x0, y0, w, h) inside the frame; None: the full frame every time; an empty one, as
    `frame_deltas` reports an unchanged frame, becomes (0, 0, 1, 1)."""
    if rects is None:
        return np.tile(np.array([0, 0, width, height], dtype=np.int32), (count, 1))
    r = np.asarray(rects)
    if r.shape != (count, 4) or r.dtype.kind not in "iu":
        raise ValueError("rects must be None or (F, 4) integer rows (x0, y0, w, h), one per frame")
    r = r.astype(np.int64)
    r[(r[:, 2] == 0) & (r[:, 3] == 0)] = (0, 0, 1, 1)
    if width > 0 and height > 0 and count > 0:
        if np.any(r[:, :2] < 0) or np.any(r[:, 2:] < 1) or np.any(r[:, 0] + r[:, 2] > width) or np.any(r[:, 1] + r[:, 3] > height):
            raise ValueError("every rectangle must lie inside the frame and have w, h >= 1 (or be the empty (0, 0, 0, 0))")
    return np.ascontiguousarray(r.astype(np.int32))


def _gif_maps(maps):
    """`maps` as contiguous (F, H, W) one-byte maps -> (maps, shape, torch device or None)."""
    if not hasattr(maps, "shape") or len(maps.shape) not in (2, 3):
        raise ValueError("maps must be an (H, W) or (F, H, W) uint8 array or a uint8 CUDA tensor")
    m, shape, dev, elem, _ = _delta_maps(maps if len(maps.shape) == 3 else maps[None])
    if elem != 1:
        raise ValueError("maps must be uint8: a GIF palette has at most 256 entries")
    return m, shape, dev


def _gif_segment(segment):
    if segment is None:
        return 0
    if isinstance(segment, (bool, np.bool_)) or not isinstance(segment, (int, np.integer)) or not 1 <= int(segment) <= 2 ** 24:
        raise ValueError("segment must be None (the default, 8192) or an integer in [1, 2^24]")
    return int(segment)


def gif_lzw_bound(rects, segment=None):
    """Bytes that always hold the streams of `gif_lzw` for these (F, 4) rectangles: 12 bits for each of at most
    area + 2 * nseg + area / 3000 + 2 codes per frame (include/patolette_amd.h)."""
    seg = _gif_segment(segment) or 8192
    area = np.asarray(rects)[:, 2].astype(np.int64) * np.asarray(rects)[:, 3].astype(np.int64)
    nseg = (area + seg - 1) // seg
    return int(np.sum((12 * (area + 2 * nseg + area // 3000 + 2) + 7) // 8))


def _gif_lzw_args(maps, rects, min_code_size, segment):
    """What `gif_lzw` and `gif_lzw_lossy` check alike, before any library call -> (maps, (F, H, W), torch device or None, m, the C
    entry's segment, (F, 4) int32 rectangles)."""
    m, shape, dev = _gif_maps(maps)
    count, height, width = shape
    if isinstance(min_code_size, (bool, np.bool_)) or not isinstance(min_code_size, (int, np.integer)) or not 2 <= int(min_code_size) <= 8:
        raise ValueError("min_code_size must be an integer in [2, 8]")
    return m, shape, dev, int(min_code_size), _gif_segment(segment), _gif_rects(rects, count, height, width)


def _gif_lzw_run(name, m, shape, dev, mcs, seg, segment, r, extra):
    """The C entry `name` (patolette_amd_gif_lzw or its lossy twin, whose `extra` arguments stand ahead of `out`) -> what `gif_lzw` returns."""
    count, height, width = shape
    out = np.empty(gif_lzw_bound(r, segment), dtype=np.uint8)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    code = C.c_int(0)
    _call(name, dev, count, width, height, _vp(m), r.ctypes.data_as(C.POINTER(C.c_int32)) if count else None,
          mcs, seg, *extra, out.ctypes.data_as(C.c_void_p), out.size, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(code))
    if code.value == -1 and _native.last_error().startswith(name + ":"):
        raise ValueError(_native.last_error())
    message = _message(code.value)
    if code.value != 0:
        return (False, None, None, message)
    return (True, out[:int(offsets[count])], offsets.astype(np.int64), message)


def gif_lzw(maps, rects=None, min_code_size=8, segment=None):
    """Index maps LZW-compressed as a GIF's image data, on the device (additive; include/patolette_amd.h: patolette_amd_gif_lzw).

      * maps: (F, H, W) or (H, W) uint8 numpy array, or a torch uint8 CUDA tensor (the maps then never leave the GPU; only the
        compressed streams do).  Maps, deltas and shown maps of the other entries all qualify.
      * rects: None, or (F, 4) rows (x0, y0, w, h) as `frame_deltas` returns them: only the rectangle is compressed.  An empty
        rectangle (an unchanged frame) is replaced by (0, 0, 1, 1): its one delta is the transparent index by definition, so a
        decoder keeps the canvas.
      * min_code_size: 2 .. 8; every element inside a rectangle must be below 2 ** min_code_size (else a ValueError).
      * segment: symbols per independently compressed segment (default 8192): smaller is more parallel and a little larger.

    Returns (success, data uint8 numpy array, offsets (F + 1,) int64, message): frame f's raw LZW stream -- not yet cut into
    sub-blocks -- is data[offsets[f]:offsets[f + 1]].  The result is always numpy.  `write_gif` wraps it in the container."""
    m, shape, dev, mcs, seg, r = _gif_lzw_args(maps, rects, min_code_size, segment)
    return _gif_lzw_run("patolette_amd_gif_lzw", m, shape, dev, mcs, seg, segment, r, ())


def _gif_near(near, mcs):
    """`near` as the contiguous (256, 16) uint8 table of the lossy coder, checked as the library checks it at minimum code size `mcs`."""
    t = np.asarray(near.detach().cpu().numpy() if hasattr(near, "detach") else near)
    if t.shape != (256, 16) or t.dtype != np.uint8:
        raise ValueError("near must be a (256, 16) uint8 array: per symbol the count, then up to 15 candidates (`gif_neighbours` makes one)")
    t = np.ascontiguousarray(t)
    rows = t[:1 << mcs]
    if np.any(rows[:, 0] > 15):
        raise ValueError("near: a row below 2 ** min_code_size has a count above 15")
    if np.any((rows[:, 1:] >= (1 << mcs)) & (np.arange(1, 16)[None, :] <= rows[:, :1])):
        raise ValueError("near: a candidate of a row below 2 ** min_code_size is not below 2 ** min_code_size")
    return t


def gif_neighbours(palette, tolerance, transparent_index=None, max_neighbours=15):
    """The table `gif_lzw_lossy` and `write_gif(near=...)` take, for a palette (include/patolette_amd.h: patolette_amd_gif_neighbours).
    Host code: no GPU is needed.

      * palette: as `remap` takes it, (K, 3) uint8 or float64 with K <= 256 (trailing (-1, -1, -1) rows of a float palette are unused).
      * tolerance: an ICtCp distance, the unit of `frame_deltas` and `measure`: row s lists the OTHER used rows within `tolerance` of it,
        nearest first (ties by index), at most `max_neighbours` (0 .. 15) of them.  0 lists identical rows only.
      * transparent_index: None, or an index in [0, 255] that neither gets candidates nor is one: transparency is never lossy.

    What the tolerance means: a coded entry lies within `tolerance` of the MAP's entry, not of the source pixel.  Behind
    `frame_deltas(tolerance=t1)` every pixel a viewer shows lies within t1 + tolerance of its frame's source, or within `tolerance`
    of the frame's own choice; nothing accumulates over the frames, because every drawn pixel is coded from that frame's own entry.
    `measure` on the composited `coded` maps of `gif_lzw_lossy` gives the true cost.

    Returns (success, near (256, 16) uint8, message)."""
    pal8, palf = _remap_palette(palette)
    rows = (pal8 if pal8 is not None else palf).shape[0]
    if rows > 256:
        raise ValueError("a GIF colour table holds at most 256 rows")
    if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (int, float, np.integer, np.floating)) \
            or not np.isfinite(tolerance) or tolerance < 0:
        raise ValueError("tolerance must be a finite number that is not negative")
    if transparent_index is not None and (isinstance(transparent_index, (bool, np.bool_)) or not isinstance(transparent_index, (int, np.integer))
                                          or not 0 <= int(transparent_index) <= 255):
        raise ValueError("transparent_index must be None or an index in [0, 255]")
    if isinstance(max_neighbours, (bool, np.bool_)) or not isinstance(max_neighbours, (int, np.integer)) or not 0 <= int(max_neighbours) <= 15:
        raise ValueError("max_neighbours must be an integer in [0, 15]")
    if palf is not None and not np.all(np.isfinite(palf)):
        raise ValueError("the palette holds a value that is not finite")
    near = np.zeros((256, 16), dtype=np.uint8)
    code = C.c_int(0)
    _native.lib().patolette_amd_gif_neighbours(_vp(palf), _vp(pal8), rows, -1 if transparent_index is None else int(transparent_index),
                                               float(tolerance), int(max_neighbours), near.ctypes.data_as(C.c_void_p), C.byref(code))
    if code.value == -1 and _native.last_error().startswith("patolette_amd_gif_neighbours:"):
        raise ValueError(_native.last_error())
    if code.value != 0:
        return (False, None, _message(code.value))
    return (True, near, _message(code.value))


def gif_lzw_lossy(maps, near, rects=None, min_code_size=8, segment=None, want_coded=False):
    """`gif_lzw` by the lossy coder (additive; include/patolette_amd.h: patolette_amd_gif_lzw_lossy): where the next symbol would end the
    current dictionary match, one of its candidates in `near` that continues the match is coded in its place -- the exact symbol
    first, then the row's order.  Ordered-dithered maps, which break every long match of the exact coder, gain most.

      * maps, rects, min_code_size, segment: as `gif_lzw` takes them.
      * near: (256, 16) uint8, per symbol the count (0 .. 15) and then the candidates in order of preference, all below
        2 ** min_code_size; `gif_neighbours(palette, tolerance, transparent_index)` makes it.  A symbol with an empty row that appears
        in no row -- the transparent index -- is never replaced and never replaces.  An all-zero table gives `gif_lzw`'s bytes.
      * want_coded: also return what the streams decode to: a copy of `maps` overwritten inside the rectangles (numpy), or a cloned
        tensor that stays on the GPU (a CUDA tensor in).  `gif_lzw(coded, ...)` returns the same bytes as this call.

    What the tolerance of the table means: a coded entry lies within it of the MAP's entry, not of the source pixel.  Behind
    `frame_deltas(tolerance=t1)` and a table at t2 every pixel a viewer shows lies within t1 + t2 of its frame's source, or within t2
    of the frame's own choice; nothing accumulates, because every drawn pixel is coded from that frame's own entry.  `measure` on the
    composited `coded` maps gives the true cost.

    Returns (success, data, offsets, coded or None, message), data and offsets as `gif_lzw` returns them."""
    m, shape, dev, mcs, seg, r = _gif_lzw_args(maps, rects, min_code_size, segment)
    table = _gif_near(near, mcs)
    coded = None
    if want_coded:
        coded = m.clone() if dev is not None else m.copy()
    ok, data, offsets, message = _gif_lzw_run("patolette_amd_gif_lzw_lossy", m, shape, dev, mcs, seg, segment, r,
                                              (table.ctypes.data_as(C.c_void_p), _vp(coded)))
    if not ok:
        return (False, None, None, None, message)
    return (True, data, offsets, coded.reshape(tuple(maps.shape)) if want_coded else None, message)


def _gif_lossy_by_table(m, near, tables, of, r, mcs, segment):
    """`gif_lzw_lossy` for frames with a table each: `near` is a (tables, 256, 16) stack, the frames are grouped by their table `of`,
    coded once per table in use, and the streams put back in frame order -> what `gif_lzw` returns."""
    stack = np.asarray(near.detach().cpu().numpy() if hasattr(near, "detach") else near)
    if stack.shape != (tables, 256, 16) or stack.dtype != np.uint8:
        raise ValueError("with (P, K, 3) tables near must be a (P, 256, 16) uint8 stack: one `gif_neighbours` table per palette")
    used = [int(g) for g in np.unique(of)]
    checked = {g: _gif_near(stack[g], mcs) for g in used}
    streams = [None] * len(of)
    message = ""
    for g in used:
        which = np.nonzero(of == g)[0]
        group = m[which] if not hasattr(m, "detach") else m[__import__("torch").as_tensor(which, device=m.device)]
        ok, data, offsets, _, message = gif_lzw_lossy(group, checked[g], r[which], mcs, segment)
        if not ok:
            return (False, None, None, message)
        for i, f in enumerate(which):
            streams[f] = data[int(offsets[i]):int(offsets[i + 1])]
    offsets = np.zeros(len(of) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(x) for x in streams])
    return (True, np.concatenate(streams), offsets, message)


def write_gif(file, maps, palette_u8, rects=None, transparent_index=None, delay=0.04, loop=0, disposal=1, palette_of=None, segment=None,
              near=None):
    """Write an animation's maps as a GIF89a file: a small pure-Python container around `gif_lzw`, so that
    `quantize_frames(frames, 255, dither="ordered")` -> `frame_deltas` -> `write_gif` yields a file any viewer opens.

      * file: a path, an object with `write`, or None.  The bytes are always returned.
      * maps: (F, H, W) or (H, W) uint8 maps or deltas (numpy, or a torch CUDA tensor); rects: as `gif_lzw` takes them.
      * palette_u8: (K, 3) uint8, K <= 256: the global colour table, padded with zero rows to the next power of two that holds every
        row and, if given, transparent_index (<= 255).  That power of two is 2 ** min_code_size (at least 4).
      * delay: seconds per frame, a number or one per frame (written in 1/100 s); loop: the NETSCAPE2.0 repeat count (0 = for ever),
        None for no loop block; disposal: every frame's disposal method (1: leave in place, what `frame_deltas`' deltas need), or a
        sequence of F of them, one per frame: `frame_deltas_rgba` returns the ones its deltas need --
        `write_gif(file, deltas, palette_rgba[:, :3], rects, transparent_index=0, disposal=disposals)`.
      * near: None for the exact coder, or the table of `gif_neighbours(palette_u8, tolerance, transparent_index)`: the streams come from
        `gif_lzw_lossy` and the file is smaller.  A shown entry then lies within that tolerance (ICtCp) of the MAP's entry, not of the
        source pixel: behind `frame_deltas(tolerance=t1)` within t1 + tolerance of its frame's source; nothing accumulates over the
        frames.  `measure` on the composited `coded` maps of `gif_lzw_lossy` gives the true cost.
      * palette_u8 may also be (P, K, 3): P tables, with palette_of the table of every frame as `frame_deltas_local` takes it (None:
        frame f takes table f, P == F).  Table palette_of[0] is written as the global colour table, and every frame with another
        table carries it as a local colour table behind its image descriptor.  All tables are padded to the same power of two, so
        the file has one min_code_size and one `gif_lzw` call codes every frame.  `near` is then a (P, 256, 16) stack, one
        `gif_neighbours` table per palette: the frames are coded by `gif_lzw_lossy` group by group, once per table in use.
    Out of scope: interlace; a transparent entry of the maps' own together with local tables (`frame_deltas_rgba` has no local
    variant).  `write_apng` writes the same animations as APNG, which has one PLTE and so no per-frame tables."""
    import os
    m, shape, dev = _gif_maps(maps)
    count, height, width = shape
    pal = np.asarray(palette_u8.detach().cpu().numpy() if hasattr(palette_u8, "detach") else palette_u8)
    of = None
    if pal.ndim == 3:
        pal, of = _local_tables(pal, palette_of, count, 256, "palette_u8")
    elif palette_of is not None:
        raise ValueError("palette_of needs palette_u8 as (P, K, 3) tables")
    elif pal.ndim != 2 or pal.shape[1] != 3 or pal.dtype != np.uint8 or pal.shape[0] < 1:
        raise ValueError("palette_u8 must be a (K, 3) uint8 array, or (P, K, 3) tables with palette_of")
    if pal.shape[-2] > 256:
        raise ValueError("a GIF colour table holds at most 256 rows")
    need = pal.shape[-2]
    if transparent_index is not None:
        if isinstance(transparent_index, (bool, np.bool_)) or not isinstance(transparent_index, (int, np.integer)) \
                or not 0 <= int(transparent_index) <= 255:
            raise ValueError("transparent_index must be None or an index in [0, 255]")
        need = max(need, int(transparent_index) + 1)
    bits = max(1, int(need - 1).bit_length())                      # the table has 2 ** bits rows
    mcs = max(2, bits)
    if count < 1 or not 1 <= width <= 65535 or not 1 <= height <= 65535:
        raise ValueError("a GIF needs at least one frame, of 1 .. 65535 pixels a side")
    r = _gif_rects(rects, count, height, width)
    delays = np.asarray(delay, dtype=np.float64)
    if delays.ndim == 0:
        delays = np.full(count, float(delays))
    if delays.shape != (count,) or not np.all(np.isfinite(delays)) or np.any(delays < 0) or np.any(np.round(delays * 100) > 65535):
        raise ValueError("delay must be a number of seconds or one per frame, each in [0, 655.35]")
    if loop is not None and (isinstance(loop, (bool, np.bool_)) or not isinstance(loop, (int, np.integer)) or not 0 <= int(loop) <= 65535):
        raise ValueError("loop must be None or a repeat count in [0, 65535]")
    if isinstance(disposal, (list, tuple, np.ndarray)) or hasattr(disposal, "detach"):
        disposals = np.asarray(disposal.detach().cpu().numpy() if hasattr(disposal, "detach") else disposal)
        if disposals.shape != (count,) or disposals.dtype.kind not in "iu" or np.any(disposals < 0) or np.any(disposals > 3):
            raise ValueError("disposal must be 0, 1, 2 or 3, or one such integer per frame")
        disposals = [int(v) for v in disposals]
    else:
        if isinstance(disposal, (bool, np.bool_)) or not isinstance(disposal, (int, np.integer)) or not 0 <= int(disposal) <= 3:
            raise ValueError("disposal must be 0, 1, 2 or 3")
        disposals = [int(disposal)] * count
    _gif_segment(segment)
    if near is None:
        ok, data, offsets, message = gif_lzw(m, r, mcs, segment)
    elif of is None:
        ok, data, offsets, _, message = gif_lzw_lossy(m, _gif_near(near, mcs), r, mcs, segment)
    else:
        ok, data, offsets, message = _gif_lossy_by_table(m, near, pal.shape[0], of, r, mcs, segment)
    if not ok:
        raise RuntimeError(message)
    tables = np.zeros(((1 if of is None else pal.shape[0]), 1 << bits, 3), dtype=np.uint8)
    tables[:, :pal.shape[-2]] = pal
    table = tables[0 if of is None else of[0]]
    u16 = lambda v: int(v).to_bytes(2, "little")
    parts = [b"GIF89a", u16(width), u16(height), bytes([0x80 | 7 << 4 | (bits - 1), 0, 0]), table.tobytes()]
    if loop is not None:
        parts += [b"\x21\xff\x0bNETSCAPE2.0\x03\x01", u16(loop), b"\x00"]
    flag, tidx = (1, int(transparent_index)) if transparent_index is not None else (0, 0)
    raw = data.tobytes()
    for f in range(count):
        parts += [b"\x21\xf9\x04", bytes([disposals[f] << 2 | flag]), u16(int(np.round(delays[f] * 100))), bytes([tidx, 0])]
        x0, y0, w, h = (int(v) for v in r[f])
        if of is None or of[f] == of[0]:
            parts += [b"\x2c", u16(x0), u16(y0), u16(w), u16(h), b"\x00", bytes([mcs])]
        else:                                                      # a local colour table, behind the descriptor
            parts += [b"\x2c", u16(x0), u16(y0), u16(w), u16(h), bytes([0x80 | (bits - 1)]), tables[of[f]].tobytes(), bytes([mcs])]
        stream = raw[int(offsets[f]):int(offsets[f + 1])]
        for i in range(0, len(stream), 255):
            block = stream[i:i + 255]
            parts += [bytes([len(block)]), block]
        parts.append(b"\x00")
    parts.append(b"\x3b")
    blob = b"".join(parts)
    if file is not None:
        if hasattr(file, "write"):
            file.write(blob)
        else:
            with open(os.fspath(file), "wb") as fh:
                fh.write(blob)
    return blob


def _png_segment(segment):
    if segment is None:
        return 0
    if isinstance(segment, (bool, np.bool_)) or not isinstance(segment, (int, np.integer)) or not 1 <= int(segment) <= 32768:
        raise ValueError("segment must be None (the default, 16384) or an integer in [1, 32768]")
    return int(segment)


def png_deflate_bound(rects, segment=None):
    """Bytes that always hold the streams of `png_deflate` for these (F, 4) rectangles: per frame 9 bits for each of its h * (w + 1)
    filtered bytes and 10 per segment (include/patolette_amd.h)."""
    seg = _png_segment(segment) or 16384
    r = np.asarray(rects).astype(np.int64)
    flen = r[:, 3] * (r[:, 2] + 1)
    nseg = (flen + seg - 1) // seg
    return int(np.sum((9 * flen + 10 * nseg + 7) // 8))


def png_deflate(maps, rects=None, segment=None):
    """Index maps deflated as an indexed PNG's image data, on the device (additive; include/patolette_amd.h: patolette_amd_png_deflate).

      * maps: (F, H, W) or (H, W) uint8 numpy array, or a torch uint8 CUDA tensor (the maps then never leave the GPU; only the
        compressed streams do).  Every byte value is a legal element.
      * rects: None, or (F, 4) rows (x0, y0, w, h) as `frame_deltas` returns them: only the rectangle is coded.  An empty rectangle
        (an unchanged frame) is replaced by (0, 0, 1, 1), as `gif_lzw` does.
      * segment: filtered bytes per independently parsed segment (default 16384, at most 32768): smaller is more parallel and a
        little larger.  A match may still start before its segment.

    What is coded per frame is PNG's scanline stream at bit depth 8 with filter type 0: every row of the rectangle behind a zero byte.
    Returns (success, data uint8 numpy array, offsets (F + 1,) int64, adler (F,) uint32, message): frame f's raw deflate stream
    (RFC 1951, no zlib wrapper) is data[offsets[f]:offsets[f + 1]] and adler[f] the Adler-32 of what it inflates to.  The result is
    always numpy.  `write_png` and `write_apng` wrap it in the containers."""
    m, shape, dev = _gif_maps(maps)
    count, height, width = shape
    seg = _png_segment(segment)
    r = _gif_rects(rects, count, height, width)
    name = "patolette_amd_png_deflate"
    out = np.empty(png_deflate_bound(r, segment), dtype=np.uint8)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    adler = np.zeros(count, dtype=np.uint32)
    code = C.c_int(0)
    _call(name, dev, count, width, height, _vp(m), r.ctypes.data_as(C.POINTER(C.c_int32)) if count else None, seg,
          out.ctypes.data_as(C.c_void_p), out.size, offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
          adler.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(code))
    if code.value == -1 and _native.last_error().startswith(name + ":"):
        raise ValueError(_native.last_error())
    message = _message(code.value)
    if code.value != 0:
        return (False, None, None, None, message)
    return (True, out[:int(offsets[count])], offsets.astype(np.int64), adler, message)


def _png_chunk(kind, body):
    import zlib
    return len(body).to_bytes(4, "big") + kind + body + zlib.crc32(kind + body).to_bytes(4, "big")


def _png_palette(palette, transparent_index):
    """The PLTE and tRNS chunks of a (K, 3) or (K, 4) uint8 palette: PLTE padded with zero rows up to transparent_index; tRNS from the
    alpha column, or opaque entries up to a transparent one."""
    pal = np.asarray(palette.detach().cpu().numpy() if hasattr(palette, "detach") else palette)
    if pal.ndim != 2 or pal.shape[1] not in (3, 4) or pal.dtype != np.uint8 or pal.shape[0] < 1:
        raise ValueError("palette must be a (K, 3) or (K, 4) uint8 array")
    if pal.shape[0] > 256:
        raise ValueError("a PNG palette holds at most 256 rows")
    rows = pal.shape[0]
    if transparent_index is not None:
        if isinstance(transparent_index, (bool, np.bool_)) or not isinstance(transparent_index, (int, np.integer)) \
                or not 0 <= int(transparent_index) <= 255:
            raise ValueError("transparent_index must be None or an index in [0, 255]")
        rows = max(rows, int(transparent_index) + 1)
    table = np.zeros((rows, 3), dtype=np.uint8)
    table[:pal.shape[0]] = pal[:, :3]
    alpha = np.full(rows, 255, dtype=np.uint8)
    if pal.shape[1] == 4:
        alpha[:pal.shape[0]] = pal[:, 3]
    if transparent_index is not None:
        alpha[int(transparent_index)] = 0
    chunks = [_png_chunk(b"PLTE", table.tobytes())]
    if np.any(alpha != 255):
        last = int(np.max(np.nonzero(alpha != 255)[0]))                # entries behind the last one that is not opaque need no byte
        chunks.append(_png_chunk(b"tRNS", alpha[:last + 1].tobytes()))
    return chunks


def _png_zlib(data, offsets, adler, f):
    """Frame f's zlib stream: the two header bytes, its raw deflate stream, the Adler-32."""
    return b"\x78\x9c" + data[int(offsets[f]):int(offsets[f + 1])].tobytes() + int(adler[f]).to_bytes(4, "big")


def _png_put(file, blob):
    import os
    if file is not None:
        if hasattr(file, "write"):
            file.write(blob)
        else:
            with open(os.fspath(file), "wb") as fh:
                fh.write(blob)
    return blob


_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _png_ihdr(width, height):
    return _png_chunk(b"IHDR", width.to_bytes(4, "big") + height.to_bytes(4, "big") + bytes([8, 3, 0, 0, 0]))


def write_png(file, map, palette, transparent_index=None, segment=None):
    """Write one (H, W) uint8 map as an indexed PNG: a small pure-Python container around `png_deflate`, so that
    `quantize_u8` -> `write_png` yields the file without the map's deflate running on a CPU core.

      * file: a path, an object with `write`, or None.  The bytes are always returned.
      * map: (H, W) uint8, numpy or a torch CUDA tensor.
      * palette: (K, 3) uint8, or (K, 4) uint8 as `quantize_rgba` returns it: tRNS then comes from the alpha column.
      * transparent_index: None, or an index in [0, 255] written as fully transparent; PLTE is padded with zero rows up to it.
      * segment: as `png_deflate` takes it.
    The file: signature, IHDR (depth 8, colour type 3, no interlace), PLTE, tRNS where an entry is not opaque, one IDAT, IEND.
    Out of scope: bit depths below 8, filters, interlace, true colour."""
    if not hasattr(map, "shape") or len(map.shape) != 2:
        raise ValueError("map must be an (H, W) uint8 array or a uint8 CUDA tensor")
    m, shape, dev = _gif_maps(map)
    _, height, width = shape
    chunks = _png_palette(palette, transparent_index)
    if not 1 <= width < 2 ** 31 or not 1 <= height < 2 ** 31:
        raise ValueError("a PNG has 1 .. 2^31 - 1 pixels a side")
    _png_segment(segment)
    ok, data, offsets, adler, message = png_deflate(m, None, segment)
    if not ok:
        raise RuntimeError(message)
    blob = b"".join([_PNG_SIGNATURE, _png_ihdr(width, height)] + chunks
                    + [_png_chunk(b"IDAT", _png_zlib(data, offsets, adler, 0)), _png_chunk(b"IEND", b"")])
    return _png_put(file, blob)


def write_apng(file, maps, palette, rects=None, transparent_index=None, delay=0.04, loop=0, disposal=1, segment=None):
    """Write an animation's maps as an APNG file: the container around `png_deflate`, for the pipelines `write_gif` serves and for
    the RGBA one: `quantize_rgba_frames(..., dither="ordered")` -> `frame_deltas_rgba` ->
    `write_apng(file, deltas, palette_rgba, rects, transparent_index=0, disposal=disposals)`.

      * file, maps, rects, transparent_index, segment: as `write_gif` takes them; palette: as `write_png` takes it.  Frame 0 is always
        written with the full-frame rectangle: APNG requires it of the default image.
      * delay: seconds per frame, a number or one per frame, written as n / 100 s; loop: acTL's num_plays (0 = for ever).
      * disposal: every frame's disposal in GIF's numbering, or one per frame, as `frame_deltas_rgba` returns them: 0 and 1 become
        APNG_DISPOSE_OP_NONE, 2 BACKGROUND, 3 PREVIOUS.  blend_op is OVER when there is a transparent index, else SOURCE.
    The file: signature, IHDR, acTL, PLTE, tRNS, then per frame fcTL and its data: IDAT for frame 0, fdAT for the others; IEND.
    Out of scope: per-frame palettes, and everything `write_png` leaves out."""
    m, shape, dev = _gif_maps(maps)
    count, height, width = shape
    chunks = _png_palette(palette, transparent_index)
    if count < 1 or not 1 <= width < 2 ** 31 or not 1 <= height < 2 ** 31:
        raise ValueError("an APNG needs at least one frame, of 1 .. 2^31 - 1 pixels a side")
    r = _gif_rects(rects, count, height, width)
    r[0] = (0, 0, width, height)
    delays = np.asarray(delay, dtype=np.float64)
    if delays.ndim == 0:
        delays = np.full(count, float(delays))
    if delays.shape != (count,) or not np.all(np.isfinite(delays)) or np.any(delays < 0) or np.any(np.round(delays * 100) > 65535):
        raise ValueError("delay must be a number of seconds or one per frame, each in [0, 655.35]")
    if isinstance(loop, (bool, np.bool_)) or not isinstance(loop, (int, np.integer)) or not 0 <= int(loop) < 2 ** 31:
        raise ValueError("loop must be a play count in [0, 2^31 - 1]")
    if isinstance(disposal, (list, tuple, np.ndarray)) or hasattr(disposal, "detach"):
        disposals = np.asarray(disposal.detach().cpu().numpy() if hasattr(disposal, "detach") else disposal)
        if disposals.shape != (count,) or disposals.dtype.kind not in "iu" or np.any(disposals < 0) or np.any(disposals > 3):
            raise ValueError("disposal must be 0, 1, 2 or 3, or one such integer per frame")
        disposals = [int(v) for v in disposals]
    else:
        if isinstance(disposal, (bool, np.bool_)) or not isinstance(disposal, (int, np.integer)) or not 0 <= int(disposal) <= 3:
            raise ValueError("disposal must be 0, 1, 2 or 3")
        disposals = [int(disposal)] * count
    _png_segment(segment)
    ok, data, offsets, adler, message = png_deflate(m, r, segment)
    if not ok:
        raise RuntimeError(message)
    u32 = lambda v: int(v).to_bytes(4, "big")
    u16 = lambda v: int(v).to_bytes(2, "big")
    blend = 1 if transparent_index is not None else 0
    parts = [_PNG_SIGNATURE, _png_ihdr(width, height), _png_chunk(b"acTL", u32(count) + u32(loop))] + chunks
    sequence = 0
    for f in range(count):
        x0, y0, w, h = (int(v) for v in r[f])
        dispose = (0, 0, 1, 2)[disposals[f]]
        parts.append(_png_chunk(b"fcTL", u32(sequence) + u32(w) + u32(h) + u32(x0) + u32(y0) + u16(int(np.round(delays[f] * 100))) + u16(100)
                                + bytes([dispose, blend])))
        sequence += 1
        if f == 0:
            parts.append(_png_chunk(b"IDAT", _png_zlib(data, offsets, adler, 0)))
        else:
            parts.append(_png_chunk(b"fdAT", u32(sequence) + _png_zlib(data, offsets, adler, f)))
            sequence += 1
    parts.append(_png_chunk(b"IEND", b""))
    return _png_put(file, b"".join(parts))


def quantize_rgba(image, palette_size, alpha_threshold=128, dither=True, palette_only=False, color_space=ColorSpace_ICtCp,
                  tile_size=512, kmeans_niter=32, kmeans_max_samples=512 ** 2, weights=None, want_quantized=True):
    """Quantise an (H, W, 4) uint8 RGBA image (additive; include/patolette_amd.h: patolette_amd_rgba).  `image` is a numpy array,
    or a torch CUDA tensor (then the map and the quantized image stay in HBM, as in `quantize_u8`).

    A pixel is transparent iff its alpha < alpha_threshold (an integer in [0, 256]); the others are opaque.
      * No transparent pixel (always for alpha_threshold=0): bit for bit `quantize_u8` of the RGB bytes; alpha 255 on the used
        palette rows; transparent_index = -1.
      * Some: entry 0 is the transparent one (palette row (0, 0, 0), palette_rgba (0, 0, 0, 0)); entries 1 .. palette_size-1 are
        what `quantize` returns with palette_size-1 colours for the opaque pixels in row-scan order (their weights); the map is 0 on
        transparent pixels and 1 + the opaque pixel's index otherwise.  The dither walks the whole image's Hilbert curve and skips
        transparent pixels exactly like positions outside the image (no dithering, the error queue unchanged).
      * All transparent: success, row 0 the transparent entry, every other row unused, the map all 0.
    weights: None or width*height values (the opaque pixels' are used).  tile_size > 0 without weights: the saliency weights of
    the full image's RGB as `quantize_u8` derives them (the RGB hidden under transparent pixels reaches the saliency map too),
    restricted to the opaque pixels.  palette_size < 2 with opaque and transparent pixels both present fails (exit code -3).

    Returns (success, palette_rgba (K,4) uint8, palette_map (H,W) uint8|uint16|uint32 or None, quantized (H,W,4) uint8 or None
    (= palette_rgba[palette_map]), palette (K,3) float64, transparent_index (0 or -1), message)."""
    px, shape, dev = _u8_pixels(image, (3,), (4,), "image must be an (H, W, 4) uint8 %s")
    if tile_size < 0:
        raise ValueError(bad_tile_size)
    height, width = shape[:2]
    w = _weights(weights, width * height, dev)
    if isinstance(alpha_threshold, bool) or int(alpha_threshold) != alpha_threshold or not 0 <= alpha_threshold <= 256:
        raise ValueError("alpha_threshold must be an integer in [0, 256]")
    opts = _options(dither, palette_only, color_space, kmeans_niter, kmeans_max_samples)
    palette = np.zeros((max(palette_size, 0), 3), dtype=np.float64, order='F')
    palette_rgba = np.zeros((max(palette_size, 0), 4), dtype=np.uint8)
    pmap, map_elem, quant = _outputs(shape[:2], palette_size, 4, dev, not palette_only, want_quantized and not palette_only)
    code, tidx = C.c_int(0), C.c_int(-1)
    _call("patolette_amd_rgba", dev, width, height, _vp(px), int(alpha_threshold), _vp(w), float(tile_size), palette_size, C.byref(opts),
          _vp(palette), _vp(palette_rgba), _vp(pmap), map_elem, _vp(quant), C.byref(tidx), C.byref(code))
    message = _message(code.value)
    _raise_saliency(code.value, message)
    if code.value == -1 and _native.last_error().startswith("patolette_amd_rgba:"):
        raise ValueError(_native.last_error())
    if code.value != 0:
        return (False, None, None, None, None, None, message)
    return (True, palette_rgba, pmap, quant, palette, tidx.value, message)


def _alpha_threshold(alpha_threshold):
    if isinstance(alpha_threshold, (bool, np.bool_)) or not isinstance(alpha_threshold, (int, np.integer)) or not 0 <= alpha_threshold <= 256:
        raise ValueError("alpha_threshold must be an integer in [0, 256]")
    return int(alpha_threshold)


def _rgba_palette(palette, transparent_index):
    """The palette of `remap_rgba` -> (bytes (k, 3) or None, float (k, 3) column-major or None, rows the maps are sized by, 0 or -1,
    the opaque rows as `ordered_spread` takes them).  Every rule of the docstring; ValueError for what breaks one."""
    if transparent_index is not None and (isinstance(transparent_index, (bool, np.bool_)) or not isinstance(transparent_index, (int, np.integer))
                                          or int(transparent_index) not in (-1, 0)):
        raise ValueError("transparent_index must be None, -1 (no transparent entry) or 0 (row 0)")
    pal = np.asarray(palette)
    if pal.ndim == 2 and pal.shape[1] == 4:
        if pal.dtype != np.uint8 or pal.shape[0] < 1:
            raise ValueError("a (K, 4) palette must be uint8 RGBA rows, as quantize_rgba returns palette_rgba")
        k = pal.shape[0]
        while k > 0 and not pal[k - 1].any():
            k -= 1                                                 # (trailing (0, 0, 0, 0) rows: unused)
        used = pal[:k]
        tidx = 0 if k > 0 and used[0, 3] == 0 else -1
        if np.any(used[1:, 3] == 0):
            raise ValueError("palette row %d has alpha 0: only row 0 can be the transparent entry" % (1 + int(np.argmax(used[1:, 3] == 0))))
        opaque = used[1:] if tidx == 0 else used
        if np.any(opaque[:, 3] != 255):
            raise ValueError("palette rows must have alpha 255 (or 0 in row 0, the transparent entry)")
        if transparent_index is not None and int(transparent_index) != tidx:
            raise ValueError("transparent_index %d contradicts the palette's alpha column (which says %d)" % (int(transparent_index), tidx))
        if opaque.shape[0] < 1:
            raise ValueError("the palette has no opaque row")
        pal8 = np.ascontiguousarray(used[:, :3])
        return pal8, None, pal.shape[0], tidx, pal8[1:] if tidx == 0 else pal8
    pal8, palf = _remap_palette(palette)
    tidx = -1 if transparent_index is None else int(transparent_index)
    opaque = _palette_rows(pal8, palf)[1 if tidx == 0 else 0:]
    if opaque.shape[0] < 1:
        raise ValueError("the palette has no opaque row")
    return pal8, palf, (pal8 if pal8 is not None else palf).shape[0], tidx, opaque


def remap_rgba(image, palette, transparent_index=None, alpha_threshold=128, dither=True, want_quantized=True, spread=None):
    """Map an RGBA image, or RGBA frames of one size, onto a palette the caller gives, of which row 0 may be a transparent entry
    (additive; include/patolette_amd.h: patolette_amd_remap_rgba_u8).  What `remap` is to `quantize_u8`, this is to `quantize_rgba`.

      * image: (H, W, 4) or (F, H, W, 4) uint8, a numpy array or a torch CUDA tensor (then the map and the quantized image stay in
        HBM).  A pixel is transparent iff its alpha < alpha_threshold (an integer in [0, 256]).
      * palette, one of
          - (K, 4) uint8, as `quantize_rgba` returns `palette_rgba`: trailing (0, 0, 0, 0) rows are unused and dropped; row 0 with
            alpha 0 is the transparent entry; every other used row must have alpha 255.  transparent_index may be left None, and must
            not contradict the rows.
          - (K, 3) uint8 or float, as `remap` takes it: transparent_index=0 makes row 0 the transparent entry (its colour is never a
            candidate), None or -1 means there is none.
      * Opaque pixels take the entry `remap` would give them with the opaque rows alone, plus 1 when row 0 is the transparent entry:
        dither=False the nearest in ICtCp, dither="ordered" the Bayer dither (spread=None: `ordered_spread` of the opaque rows),
        dither=True the Riemersma walk over each frame's own curve, on which transparent pixels are skipped like positions outside
        the image (as in `quantize_rgba`).  No state passes between frames.
      * Transparent pixels get index 0 and quantized (0, 0, 0, 0); a transparent pixel while the palette has no transparent entry
        is a ValueError.
    These maps go into `frame_deltas_rgba` and `measure(..., skip_index=0)`.

    Returns (success, palette_map (H,W) or (F,H,W) uint8|uint16|uint32 by K, quantized (..., 4) uint8 or None, message)."""
    mode, spread = _dither_mode(dither), _spread_value(spread)
    px, shape, dev = _u8_pixels(image, (3, 4), (4,), "image must be an (H, W, 4) or (F, H, W, 4) uint8 %s")
    thr = _alpha_threshold(alpha_threshold)
    if hasattr(palette, "detach"):
        palette = palette.detach().cpu().numpy()
    pal8, palf, rows, tidx, opaque = _rgba_palette(palette, transparent_index)
    if mode == 2 and spread is None:
        spread = ordered_spread(opaque)
    count, (height, width) = (shape[0] if len(shape) == 4 else 1), shape[-3:-1]
    pmap, map_elem, quant = _outputs(shape[:-1], rows, 4, dev, True, want_quantized)
    code = C.c_int(0)
    _call("patolette_amd_remap_rgba_u8", dev, count, width, height, _vp(px), thr, _vp(palf), _vp(pal8),
          (pal8 if pal8 is not None else palf).shape[0], tidx, mode, 0.0 if spread is None else spread, _vp(pmap), map_elem, _vp(quant),
          C.byref(code))
    if code.value == -1 and _native.last_error().startswith("patolette_amd_remap_rgba:"):
        raise ValueError(_native.last_error())
    message = _message(code.value)
    if code.value != 0:
        return (False, None, None, message)
    return (True, pmap, quant, message)


def quantize_rgba_frames(frames, palette_size, alpha_threshold=128, dither=True, palette_only=False, color_space=ColorSpace_ICtCp,
                         tile_size=512, kmeans_niter=32, kmeans_max_samples=512 ** 2, weights=None, want_quantized=True, spread=None):
    """Quantise an animation with transparency: (F, H, W, 4) uint8 RGBA frames (numpy, or a torch CUDA tensor) get ONE shared palette
    with ONE transparent index, and every frame its own map.  Composed in Python from two library calls, as dither="ordered" is:

      * Palette: `quantize_rgba`'s entry on the frames viewed as one (F*H, W, 4) image, without its map stage -- the palette of the
        opaque pixels of all frames, entry 0 transparent iff any pixel of any frame is.
      * weights: None or F*H*W values in frame order.  tile_size > 0 without weights: every frame's weights are `saliency_weights` of
        that frame's RGB as an image of its own, handed over as explicit weights -- one host round trip per frame.
      * Maps: `remap_rgba(frames, palette, transparent_index, alpha_threshold, dither, spread=spread)` with the float palette just
        made; dither may be "ordered".  As with dither="ordered" elsewhere, the maps are the remap of the RETURNED palette: close to,
        not bit for bit, the map the pipeline itself would have made (the palette has been through the way back to sRGB).
      * palette_only stops after the first call (and, as in the reference, leaves the palette in the quantisation's colour space).

    Returns (success, palette_rgba (K,4) uint8, maps (F,H,W) or None, quantized (F,H,W,4) uint8 or None (= palette_rgba[maps]),
    palette (K,3) float64, transparent_index (0 or -1), message)."""
    mode, spread = _dither_mode(dither), _spread_value(spread)
    px, shape, dev = _u8_pixels(frames, (4,), (4,), "frames must be an (F, H, W, 4) uint8 %s")
    if tile_size < 0:
        raise ValueError(bad_tile_size)
    thr = _alpha_threshold(alpha_threshold)
    count, height, width = shape[:3]
    n = width * height
    w = _weights(weights, count * n, dev, "frames*width*height")
    if w is None and tile_size > 0:
        host = px.cpu().numpy() if dev is not None else px
        w = _weights(np.concatenate([saliency_weights(width, height, host[f, :, :, :3].reshape(n, 3) / 255.0, tile_size)
                                     for f in range(count)]), count * n, dev)
    rows = max(palette_size, 0)
    palette = np.zeros((rows, 3), dtype=np.float64, order='F')
    palette_rgba = np.zeros((rows, 4), dtype=np.uint8)
    code, tidx = C.c_int(0), C.c_int(-1)
    opts = _options(False, palette_only, color_space, kmeans_niter, kmeans_max_samples)
    _call("patolette_amd_rgba", dev, width, count * height, _vp(px), thr, _vp(w), 0.0, palette_size, C.byref(opts), _vp(palette),
          _vp(palette_rgba), None, 1, None, C.byref(tidx), C.byref(code))
    message = _message(code.value)
    _raise_saliency(code.value, message)
    if code.value == -1 and _native.last_error().startswith("patolette_amd_rgba:"):
        raise ValueError(_native.last_error())
    if code.value != 0:
        return (False, None, None, None, None, None, message)
    if palette_only:
        return (True, palette_rgba, None, None, palette, tidx.value, message)
    if tidx.value == 0 and not palette_rgba[1:].any():            # every pixel of every frame transparent: index 0 throughout
        pmap, _, quant = _outputs(shape[:3], rows, 4, dev, True, want_quantized)
        return (True, palette_rgba, pmap, quant, palette, 0, message)
    ok, pmap, quant, message = remap_rgba(px, palette, tidx.value, thr, dither if mode != 2 else "ordered", want_quantized, spread)
    if not ok:
        return (False, None, None, None, None, None, message)
    return (True, palette_rgba, pmap, quant, palette, tidx.value, message)


def quantize_batch(width, height, images, palette_size, weights=None, dither=True, palette_only=False,
                   color_space=ColorSpace_ICtCp, tile_size=512, kmeans_niter=32, kmeans_max_samples=512 ** 2, verbose=False):
    """Quantise a list of independent images of identical size on the current GPU through
    `patolette_amd_batch` (up to six images in flight: uploads and host-side work of one image
    overlap kernels of another).  Per-image results are identical to separate `quantize` calls
    with the same arguments (batch extension).  `weights`: None or one entry (array or None) per image;
    images without explicit weights get the saliency-derived ones when tile_size > 0, as in `quantize`.
    Returns a list of `quantize` tuples."""
    if tile_size < 0:
        return [(False, None, None, bad_tile_size)] * len(images)
    count = len(images)
    n = width * height
    # all planar (F-ordered float64) -> the planar entry as is; otherwise every image goes row-major (no transposes)
    arrs = [np.asarray(im) for im in images]
    planar = all(a.ndim == 2 and a.dtype == np.float64 and a.flags.f_contiguous and not a.flags.c_contiguous for a in arrs)
    datas = arrs if planar else [np.ascontiguousarray(a, dtype=np.float64) for a in arrs]
    for d in datas:
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError(bad_channel_count.format(d.shape[1] if d.ndim == 2 else "?"))
        if d.shape[0] != n:
            raise ValueError(color_mismatch)
    if weights is not None and len(weights) != count:
        raise ValueError("weights must hold one entry (array or None) per image")
    ws = [None] * count if weights is None else [None if w is None else np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
                                                  for w in weights]
    for w in ws:
        if w is not None and w.size != n:
            raise ValueError("weights must hold width*height values")
    opts = _native.QuantizationOptions(bool(dither), bool(palette_only), int(color_space), int(kmeans_niter),
                                       int(kmeans_max_samples), bool(verbose))
    pals = [np.zeros((palette_size, 3), dtype=np.float64, order='F') for _ in range(count)]
    maps = [None if palette_only else np.zeros(n, dtype=np.uintp) for _ in range(count)]
    PD = _native.dp * count
    PZ = _native.zp * count
    d_arr = PD(*[_dp(d) for d in datas])
    w_arr = None if weights is None else PD(*[_dp(w) if w is not None else _native.dp() for w in ws])
    p_arr = PD(*[_dp(p) for p in pals])
    m_arr = None if palette_only else PZ(*[m.ctypes.data_as(_native.zp) for m in maps])
    codes = (C.c_int * count)()
    L = _native.lib()
    (L.patolette_amd_batch if planar else L.patolette_amd_batch_rows)(count, width, height, d_arr, w_arr, float(tile_size), palette_size,
                                                                      C.byref(opts), p_arr, m_arr, codes)
    out = []
    for i in range(count):
        msg = L.get_patolette_exit_code_info_message(codes[i]).decode('UTF-8')
        _raise_saliency(codes[i], msg)
        if codes[i] != 0:
            out.append((False, None, None, msg))
        else:
            out.append((True, pals[i], maps[i], msg))
    return out


def quantize_u8_batch(images, palette_size, weights=None, dither=True, palette_only=False, color_space=ColorSpace_ICtCp,
                      tile_size=512, kmeans_niter=32, kmeans_max_samples=512 ** 2, want_quantized=True):
    """`quantize_u8` for a list of (H, W, 3|4) uint8 images of identical shape through `patolette_amd_batch_u8`: up to six
    images in flight on the current GPU, and 3 bytes per pixel over PCIe instead of 24, so a host-fed batch is bound by the
    kernels rather than by the upload.  Per-image results are identical to separate `quantize_u8` calls.
    Returns a list of `quantize_u8` tuples."""
    if tile_size < 0:
        return [(False, None, None, None, None, bad_tile_size)] * len(images)
    imgs = [np.ascontiguousarray(im) for im in images]
    count = len(imgs)
    if count == 0:
        return []
    shape = imgs[0].shape
    for im in imgs:
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] not in (3, 4) or im.shape != shape:
            raise ValueError("images must be (H, W, 3|4) uint8 arrays of one shape")
    height, width, channels = shape
    n = width * height
    if weights is not None and len(weights) != count:
        raise ValueError("weights must hold one entry (array or None) per image")
    ws = [_weights(w, n, None) for w in (weights if weights is not None else [None] * count)]
    opts = _options(dither, palette_only, color_space, kmeans_niter, kmeans_max_samples)
    pals = [np.zeros((palette_size, 3), dtype=np.float64, order='F') for _ in range(count)]
    pal8 = [np.zeros((max(palette_size, 0), 3), dtype=np.uint8) for _ in range(count)]
    maps, map_elems, quants = zip(*[_outputs((height, width), palette_size, 3, None, not palette_only, want_quantized and not palette_only)
                                    for _ in range(count)])
    vp = lambda a: _vp(a) or C.c_void_p()   # noqa: E731  (an array of pointers wants a null pointer, not None)
    PV = C.c_void_p * count
    PD = _native.dp * count
    codes = (C.c_int * count)()
    L = _native.lib()
    L.patolette_amd_batch_u8(count, width, height, PV(*[vp(im) for im in imgs]), channels,
                             None if weights is None else PD(*[_dp(w) if w is not None else _native.dp() for w in ws]),
                             float(tile_size), palette_size, C.byref(opts), PD(*[_dp(p) for p in pals]), PV(*[vp(p) for p in pal8]),
                             None if palette_only else PV(*[vp(m) for m in maps]), map_elems[0],
                             PV(*[vp(q) for q in quants]) if (want_quantized and not palette_only) else None, codes)
    return [_u8_result(codes[i], pal8[i], maps[i], quants[i], pals[i]) for i in range(count)]


def _current_device_index():
    """The HIP device the calling thread is on: torch's, where torch has initialised its runtime in this process, else 0 -- also
    when the thread has selected another device by other means, which nothing here can see."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        return int(torch.cuda.current_device())
    return 0


class ColorHistogram:
    """One palette for pixels that arrive in chunks (additive; include/patolette_amd.h, "ColorHistogram"): an exact histogram of
    8-bit colours kept on the GPU, filled by as many `add` calls as the caller likes -- the frames of a clip a few at a time, the
    images of a directory, what a decoder hands out -- and the palette made from it at the end:

        h = ColorHistogram()
        for chunk in chunks:                      # (F, H, W, 3) uint8 each, any F
            h.add(chunk)
        ok, palette_u8, palette, msg = h.palette(256)
        maps = [remap(chunk, palette, dither="ordered")[1] for chunk in chunks]

      * The key of a pixel is R << 16 | G << 8 | B; per key the table holds a 64-bit count and, with weighted=True (fixed at
        construction), the sum of the pixels' weights as integers in units of 2^-32 (each weight rint(w * 2^32); 0 <= w <= 2^20).
      * Exact and order-free: the same pixels added whole, frame by frame, row by row or backwards give the same bits.
      * A refused add (a ValueError) leaves the histogram as it was.  A weight sum beyond 2^64 units raises OverflowError; after it
        every method but `clear()` raises OverflowError too.
      * The table (128 MB, weighted 256 MB) is allocated and cleared on the current device at construction and freed by `close()`,
        by leaving the `with` block, or with the object.  The device is recorded as torch's current one where torch has already
        initialised CUDA in the process, otherwise as device 0: a histogram made before the first torch CUDA call counts as
        device 0's, whatever device the thread is on.
    One histogram is used by one thread at a time; several histograms may be filled by several threads and merged."""

    def __init__(self, weighted=False):
        self._ptr = None
        self._weighted = bool(weighted)
        self._device = _current_device_index()
        L = _native.lib()
        ptr = L.patolette_amd_malloc(L.patolette_amd_hist_bytes(int(self._weighted)))
        if not ptr:
            raise MemoryError("ColorHistogram: no device memory for the table (%s)" % _native.last_error())
        self._ptr = C.c_void_p(ptr)
        try:
            self.clear()
        except Exception:
            self.close()
            raise

    # -- lifetime
    def close(self):
        """Free the table.  Every later use raises ValueError; closing twice is fine."""
        ptr, self._ptr = self._ptr, None
        if ptr is not None:
            _native.lib().patolette_amd_free(ptr)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _alive(self):
        if self._ptr is None:
            raise ValueError("this ColorHistogram has been closed")

    def _there(self):
        """A context in which the histogram's device is the current one (torch's, where torch runs in this process)."""
        import contextlib
        import sys
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
            return torch.cuda.device(self._device)
        return contextlib.nullcontext()

    @staticmethod
    def _raise(code):
        """Nothing for 0; the saliency stage's exceptions; OverflowError / ValueError for the histogram's own refusals."""
        if code == 0:
            return
        message = _message(code) if -7 <= code <= 0 else "exit code %d" % code
        _raise_saliency(code, message)
        if code == -1:
            err = _native.last_error()
            if err.startswith("patolette_amd_hist") and ": overflow:" in err:
                raise OverflowError(err)
            if err.startswith("patolette_amd_hist"):
                raise ValueError(err)
            raise RuntimeError(err or message)
        raise ValueError(message)

    # -- filling
    @property
    def weighted(self):
        return self._weighted

    def clear(self):
        """Empty the histogram (also after an overflow).  Returns self."""
        self._alive()
        with self._there():
            self._raise(_native.lib().patolette_amd_hist_clear(self._ptr, int(self._weighted)))
        return self

    def add(self, image, weights=None, tile_size=0, alpha_threshold=None):
        """Add the pixels of an (H, W, 3|4) image or of (F, H, W, 3|4) frames, uint8 sRGB, a numpy array or a torch CUDA tensor on
        the histogram's device (then nothing crosses PCIe).  A 4th channel does not enter the key; with alpha_threshold (0..255) a
        pixel whose alpha is below it enters nothing.  A weighted histogram needs `weights` (one per pixel, finite, in [0, 2^20]) or
        tile_size > 0 (every frame gets the saliency weights `quantize_frames` derives for it); an unweighted one takes neither.
        Returns self."""
        self._alive()
        px, shape, dev = _u8_pixels(image, (3, 4), (3, 4), "image must be an (H, W, 3|4) or (F, H, W, 3|4) uint8 %s")
        if len(shape) == 3:
            shape = (1,) + shape
        count, height, width, channels = shape
        if dev is not None and (self._device if dev.index is None else dev.index) != self._device:
            raise ValueError("the tensor lives on %s, the histogram on device %d" % (dev, self._device))
        if not isinstance(tile_size, (int, float, np.integer, np.floating)) or not tile_size >= 0:
            raise ValueError(bad_tile_size)
        if not self._weighted and (weights is not None or tile_size > 0):
            raise ValueError("an unweighted ColorHistogram takes neither weights nor a tile_size above 0")
        if self._weighted and weights is None and not tile_size > 0:
            raise ValueError("a weighted ColorHistogram needs weights, or a tile_size above 0 to derive them")
        thr = -1
        if alpha_threshold is not None:
            if channels != 4:
                raise ValueError("alpha_threshold needs pixels of 4 channels")
            thr = _alpha_threshold(alpha_threshold)
            if thr > 255:
                raise ValueError("alpha_threshold must lie in [0, 255]")
        w = _weights(weights, count * height * width, dev, "frames*height*width")
        code = C.c_int(0)
        with self._there():
            _call("patolette_amd_hist_add_u8", dev, self._ptr, int(self._weighted), count, width, height, _vp(px), channels, thr, _vp(w),
                  float(tile_size), C.byref(code))
        self._raise(code.value)
        return self

    def merge(self, other):
        """Add another histogram of the same mode and device into this one, bin by bin (`other` is unchanged).  Returns self."""
        self._alive()
        if not isinstance(other, ColorHistogram) or other is self:
            raise ValueError("merge takes another ColorHistogram")
        other._alive()
        if other._weighted != self._weighted or other._device != self._device:
            raise ValueError("merge needs two histograms of the same mode (weighted or not) on the same device")
        with self._there():
            self._raise(_native.lib().patolette_amd_hist_merge(self._ptr, other._ptr, int(self._weighted)))
        return self

    # -- reading
    def _totals(self):
        self._alive()
        px, colors, code = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        with self._there():
            _native.lib().patolette_amd_hist_totals(self._ptr, int(self._weighted), C.byref(px), C.byref(colors), C.byref(code))
        self._raise(code.value)
        return int(px.value), int(colors.value)

    @property
    def pixels(self):
        """How many pixels have entered."""
        return self._totals()[0]

    @property
    def colors(self):
        """How many distinct colours have entered."""
        return self._totals()[1]

    def export(self):
        """Every colour with a count above 0, ascending by key: (colors (M, 3) uint8, counts (M,) int64, weights (M,) float64 -- the
        counts again for an unweighted histogram, the summed weights (units / 2^32, rounded once) for a weighted one).  numpy."""
        m = self._totals()[1]
        colors, counts, weights = np.zeros((m, 3), dtype=np.uint8), np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.float64)
        code = C.c_int(0)
        with self._there():
            _native.lib().patolette_amd_hist_export(self._ptr, int(self._weighted), m, _vp(colors),
                                                    counts.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(weights), C.byref(code))
        self._raise(code.value)
        return colors, counts.astype(np.int64), weights

    def palette(self, palette_size, color_space=ColorSpace_ICtCp, kmeans_niter=32, kmeans_max_samples=512 ** 2):
        """The palette of `palette_size` rows for everything added so far.  Of the colours with a weight above 0 (a ValueError if
        there is none): no more than palette_size of them are returned as they are, in key order, and no quantiser runs; more are
        quantised with their counts (or summed weights) as weights -- bit for bit
        `quantize_u8(colors[None], palette_size, dither=False, tile_size=0, weights=w, want_quantized=False)` on the exported list.
        Returns (success, palette_u8 (K, 3) uint8, palette (K, 3) float64 as `quantize` returns it, message); both palettes go
        straight into `remap`, `frame_deltas` and `write_gif`."""
        self._alive()
        palette_size = int(palette_size)
        palette = np.zeros((max(palette_size, 0), 3), dtype=np.float64, order='F')
        palette_u8 = np.zeros((max(palette_size, 0), 3), dtype=np.uint8)
        opts = _options(False, False, color_space, kmeans_niter, kmeans_max_samples)
        code = C.c_int(0)
        with self._there():
            _native.lib().patolette_amd_hist_palette(self._ptr, int(self._weighted), max(palette_size, 0), C.byref(opts), _vp(palette),
                                                     _vp(palette_u8), C.byref(code))
        if code.value in (-1, -5, -6, -7):
            self._raise(code.value)
        message = _message(code.value)
        if code.value != 0:
            return (False, None, None, message)
        return (True, palette_u8, palette, message)


__all__ = [
    "__doc__",
    "ColorHistogram",
    "__version__",
    "quantize",
    "quantize_batch",
    "quantize_u8",
    "quantize_u8_batch",
    "quantize_rgba",
    "quantize_rgba_frames",
    "quantize_frames",
    "remap",
    "remap_rgba",
    "ordered_spread",
    "frame_deltas",
    "frame_deltas_rgba",
    "frame_deltas_local",
    "measure",
    "psnr",
    "gif_lzw",
    "gif_lzw_bound",
    "gif_lzw_lossy",
    "gif_neighbours",
    "write_gif",
    "png_deflate",
    "png_deflate_bound",
    "write_png",
    "write_apng",
    "saliency_weights",
    "ColorSpace_sRGB",
    "ColorSpace_CIELuv",
    "ColorSpace_ICtCp",
]
