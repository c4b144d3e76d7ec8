/*
 * patolette_amd.h -- additive C-ABI extensions of libpatolette_amd.so (not in the reference).
 *
 * The reference exports one monolithic call (include/patolette.h).  The entry points below
 * expose (1) the same call with inputs already resident in HBM, (2) the call with the Python
 * binding's `tile_size` (saliency-derived weights computed on the device) and with row-major
 * colours, (3) 8-bit adaptors around it, (4) a batch call for independent images, (5) each
 * stage of the path on its own -- every one names the reference function it replaces -- so
 * parity tests can check the HIP path stage by stage against the oracle, and (6) kernel
 * timing / run statistics for bench.py.  Plain pointers and sizes only.
 */
#ifndef PATOLETTE_AMD_H
#define PATOLETTE_AMD_H

#include <stddef.h>
#include <stdint.h>

#include "patolette.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device management ------------------------------------------------------------------ */
int  patolette_amd_device_count(void);                 /* 0 if no usable HIP device */
int  patolette_amd_set_device(int ordinal);            /* 0 ok */
const char *patolette_amd_last_error(void);            /* message of the last failure on this thread (kept with the thread's engine:
                                                          "" after patolette_amd_release_workspace or a change of device) */
void *patolette_amd_malloc(size_t bytes);              /* hipMalloc; NULL on failure */
void patolette_amd_free(void *dptr);
int  patolette_amd_memcpy_h2d(void *dst, const void *src, size_t bytes);
int  patolette_amd_memcpy_d2h(void *dst, const void *src, size_t bytes);
int  patolette_amd_synchronize(void);
/* Every calling thread works on an engine (HIP stream + workspace, ~170 bytes per pixel of the largest image it has
 * seen) taken from a per-device pool and handed back when the thread exits.  This call frees the calling thread's
 * engine and every idle pooled one (the reference frees all internals before patolette() returns,
 * lib/src/patolette.c:338-341; here the workspace is kept between calls for speed and released on request). */
void patolette_amd_release_workspace(void);
/* synthetic inputs generated directly in HBM: planar image of n pixels,
 * plane p pixel i = u(1000*seed + p, i); weights = 1 + 3*u(1000*seed + 7, i) */
int  patolette_amd_fill_image(double *d_planar, size_t n, uint64_t seed);
int  patolette_amd_fill_weights(double *d_weights, size_t n, uint64_t seed);

/* ---- the full path with HBM-resident inputs/outputs --------------------------------------
 * Same semantics as patolette() (lib/src/patolette.c:157-343) except that d_data / d_weights
 * are device pointers and the index map is left in HBM at d_palette_map with elements of
 * map_elem_bytes (1 when palette_size <= 256, else 4; 8 always allowed).  `palette` is host
 * memory, (palette_size,3) column-major. */
void patolette_amd_device(size_t width, size_t height, const double *d_data, const double *d_weights,
                          size_t palette_size, const patolette__QuantizationOptions *options,
                          double *palette, void *d_palette_map, int map_elem_bytes, int *exit_code);

/* ---- saliency-derived weights ----------------------------------------------
 * What the reference's Python binding computes before calling patolette() when tile_size > 0
 * (`get_weights`, src/patolette/patolette.pyx:203-313, called at :407-414): minimum-barrier-distance
 * saliency of the channel-mean image (3 raster scans), Mahalanobis colour contrast against the four
 * border bands in CIELAB, centre prior, sigmoid; weight = 1 + sal^2 * width*height / tile_size^2.
 *
 * patolette_amd_quantize = patolette() with the binding's tile_size semantics: `weights` non-NULL ->
 * used as given; else tile_size > 0 -> weights derived on the device (never leave HBM); else
 * unweighted.  Extra exit codes (messages via get_patolette_exit_code_info_message): -5 the image
 * shape cannot be processed (the reference raises for it too: a side <= 3 pixels, fewer than 100
 * pixels, or a border band of floor(0.1*sqrt(w*h)) pixels that does not fit), -6 a border band has
 * a singular colour covariance (numpy raises LinAlgError in the reference), -7 the saliency map is
 * degenerate: one of the maxima it is normalised by is 0 or not finite (an image whose channel mean
 * is constant has barrier distance 0 everywhere), for which the reference's weights are all NaN. */
void patolette_amd_quantize(size_t width, size_t height, const double *data, const double *weights,
                            double tile_size, size_t palette_size,
                            const patolette__QuantizationOptions *options, double *palette,
                            size_t *palette_map, int *exit_code);
/* The same with the colours as (width*height, 3) ROW-MAJOR f64 -- the layout of `img.reshape(-1, 3)` in numpy
 * (README.md:156) -- so a binding need not transpose into the planar layout patolette() takes
 * (np.asfortranarray at patolette.pyx:388-391 costs ~60 ms on a 16 MP image, six times the device time). */
void patolette_amd_quantize_rows(size_t width, size_t height, const double *rows, const double *weights,
                                 double tile_size, size_t palette_size,
                                 const patolette__QuantizationOptions *options, double *palette,
                                 size_t *palette_map, int *exit_code);
/* the stage alone, host buffers: data as for patolette(); weights_out[width*height].  Returns 0,
 * -1 (HIP error), -2 (shape), -3 (singular covariance), -4 (degenerate map: what -7 stands for above). */
int patolette_amd_saliency_weights(size_t width, size_t height, const double *data, double tile_size,
                                   double *weights_out);

/* mbd(img, iters) alone (patolette.pyx:156-201): img / out f32 row-major (rows, cols), host buffers.
 * Returns 0, -1 (HIP error) or -2 (rows <= 3 or cols <= 3: the reference returns None). */
int patolette_amd_mbd(size_t rows, size_t cols, const float *img, int iters, float *out);

/* ---- 8-bit adaptors around the path ---------------------------------------
 * Replace what every caller of the reference does by hand around quantize():
 *   ingest          colors = img.reshape(-1,3).astype(float64) / 255           (README.md:156-158)
 *   palette_u8      clip(palette * 255, 0, 255).astype(uint8)                  (README.md:178-181)
 *   quantized       palette_u8[palette_map]                                    (README.md:186-187)
 * pixels: width*height interleaved 8-bit sRGB, `channels` (3 or 4) bytes per pixel (a 4th byte is
 * ignored).  weights / tile_size: as for patolette_amd_quantize().  Outputs, each optional (NULL):
 * palette (palette_size,3) column-major f64 exactly as patolette() returns it; palette_u8
 * palette_size x 3 interleaved (unused rows 0); palette_map with elements of map_elem_bytes
 * (1, 2, 4 or 8; must be able to hold palette_size-1); quantized = width*height x 3 interleaved.
 * The conversion v/255.0 happens in the first kernel (3 B/px cross PCIe instead of 24), results
 * are identical to the f64 entry point fed with the by-hand conversion.  The *_device flavour takes
 * device pointers for pixels / weights / palette_map / quantized (map_elem_bytes 1 when
 * palette_size <= 256, else 4); palette and palette_u8 stay host memory. */
void patolette_amd_u8(size_t width, size_t height, const unsigned char *pixels, int channels, const double *weights,
                      double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                      unsigned char *palette_u8, void *palette_map, int map_elem_bytes, unsigned char *quantized,
                      int *exit_code);
void patolette_amd_u8_device(size_t width, size_t height, const unsigned char *d_pixels, int channels,
                             const double *d_weights, double tile_size, size_t palette_size,
                             const patolette__QuantizationOptions *options, double *palette,
                             unsigned char *palette_u8, void *d_palette_map, int map_elem_bytes,
                             unsigned char *d_quantized, int *exit_code);

/* ---- an animation: frames of one size, ONE palette, every frame dithered on its own ----------------
 * pixels: `frames` images of width x height, interleaved 8-bit sRGB with `channels` (3 or 4; a 4th byte is ignored) bytes per pixel,
 * one after another (the (frames, height, width, channels) array of numpy).  n = width*height, N = frames*n.  Options as patolette_amd_u8().
 *   Weights.  weights non-NULL: N values in frame order, used as they are.  Else tile_size > 0: frame f's weights are what
 *       patolette_amd_u8() derives for frame f as an image of its own (saliency per frame, that frame's rows x cols in the formula).
 *       Else unweighted.
 *   Palette.  What patolette() computes up to and including the KMeans refinement (patolette.c:201-264) for the N pixels of the frames
 *       laid one after another in frame order, with the weights above in the same order.  The quantisers and the KMeans subsample see a
 *       list of N colours (geometry does not enter); kmeans_max_samples applies to N.
 *   Maps.  For each frame separately, patolette()'s map stage (patolette.c:266-324) with that palette on the frame's n pixels: without
 *       dithering the nearest entry (for CIELuv after the reference's detour to ICtCp, palette and pixels alike); with dithering
 *       patolette__DITHER_riemersma over that frame's own width x height curve, starting from an empty error queue.  No state passes
 *       from one frame to the next.
 *   Outputs, each optional (NULL): palette (palette_size,3) column-major f64, unused rows -1, and palette_u8 as patolette_amd_u8()
 *       makes them (the palette takes the conversions of the branch that was run, dither or nearest); palette_map: N elements of
 *       map_elem_bytes (1, 2, 4 or 8; able to hold palette_size-1), frame after frame; quantized = N x 3 interleaved =
 *       palette_u8[palette_map].  palette_only: no maps.
 * Hence, bit for bit: frames == 1 is patolette_amd_u8() on that image, every output.  Without dithering every output equals
 * patolette_amd_u8() on the frames stacked into one width x (frames*height) image (explicit or no weights).  With dithering the
 * palette equals that stacked call's; the maps in general do not (the stacked call walks ONE curve through all frames).
 * Exit codes as patolette_amd_u8(); frames == 0 is -2 like an empty image; N above 2^31 pixels fails with -4 (the dither numbers the
 * pixels and their places in its run layout with 32 bits; patolette_amd_last_error says so), bad channels / map_elem_bytes with -1.
 * Statistics (patolette_amd_last_stats): dither_segments is the number of runs over all frames -- the same number in every frame, so
 * no run straddles a frame start; dither_repairs / rounds / jumps / solo count over all frames.
 * The *_device flavour takes device pointers for pixels / weights / palette_map / quantized (map_elem_bytes 1 when palette_size <= 256,
 * else 4); palette and palette_u8 stay host memory. */
void patolette_amd_frames_u8(size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels, const double *weights,
                             double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                             unsigned char *palette_u8, void *palette_map, int map_elem_bytes, unsigned char *quantized, int *exit_code);
void patolette_amd_frames_u8_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int channels,
                                    const double *d_weights, double tile_size, size_t palette_size,
                                    const patolette__QuantizationOptions *options, double *palette, unsigned char *palette_u8,
                                    void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized, int *exit_code);

/* ---- remap: 8-bit images and frames onto a palette the CALLER gives --------------------------------
 * No palette is made: the index map of the pixels on the given palette, as patolette()'s map stage takes it for colour space sRGB.
 *   Pixels.  `frames` images of width x height, interleaved 8-bit sRGB with `channels` (3 or 4; a 4th byte is ignored) bytes per pixel, one
 *       after another, exactly as patolette_amd_frames_u8() takes them; frames == 1 is the single image.  Pixel value = v / 255.0.
 *       n = width*height, N = frames*n.
 *   Palette.  Exactly one of
 *       palette_u8: palette_rows x 3 interleaved bytes; entry value = v / 255.0, the expression the pixels take;
 *       palette:    (palette_rows, 3) column-major f64 sRGB as patolette() and the entries above return it.  Trailing rows equal to
 *                   (-1, -1, -1) (the fill of unused rows) are dropped; what remains must be at least one row and all finite.  Values
 *                   outside [0, 1] are taken as they are (the conversions are defined for them as the reference's are).
 *       Map indices are row numbers of the palette as given.  Rows: what the map kernels take (no limit of this entry's own).
 *   Maps, frame by frame, no state passing from one frame to the next:
 *       dither == 0: palette and pixels go sRGB -> ICtCp (patolette__COLOR_sRGB_Matrix_to_ICtCp_Matrix), then
 *           patolette__PALETTE_fill_palette_map_nearest -- the space in which the reference takes its nearest map for both of its
 *           perceptual colour spaces (patolette.c:300-324).  Ties: the lowest index.
 *       dither != 0: palette and pixels go sRGB -> linear Rec2020 (patolette__COLOR_sRGB_Matrix_to_Linear_Rec2020_Matrix), then
 *           patolette__DITHER_riemersma over that frame's own width x height curve from an empty error queue (patolette.c:268-299 for
 *           colour space sRGB).
 *   Outputs, each optional (NULL): palette_map, N elements of map_elem_bytes (1, 2, 4 or 8; able to hold palette_rows-1), frame after
 *       frame; quantized = N x 3 interleaved = pal8[palette_map], where pal8 is palette_u8 as given, or for an f64 palette
 *       clip(palette * 255, 0, 255) truncated to bytes (what patolette_amd_u8() returns as palette_u8; dropped rows 0).
 *   Exit codes: 0; -2 an empty image or frames == 0; -4 more than 2^31 pixels in all with dithering (more than 40000^2 without); -1 bad
 *       channels / map_elem_bytes, both or neither palette given, no usable or a non-finite palette row (patolette_amd_last_error says
 *       which).  A failed call leaves the thread's engine usable.
 *   Statistics (patolette_amd_last_stats): ms_upload, ms_map, ms_download, ms_total and the dither counters (as
 *       patolette_amd_frames_u8() counts them); every quantiser field is 0.  patolette_amd_last_map_palette: the palette in the map's space.
 * Hence: a pixel whose bytes equal a palette_u8 entry's takes the same conversion of the same value -- in the reference's arithmetic it is
 * at distance exactly 0 from that entry (here the pixels are converted on the device and the palette on the host, which agree to the
 * 0.52 ulp of patolette_amd_pow: far below what separates two distinct byte rows); remapping the quantized image of an 8-bit call onto
 * that call's palette_u8 (distinct rows) returns that call's map and image, dither on or off.
 * NOT promised: that a remap with the F64 palette some earlier call returned is bit for bit that call's own map.  The returned palette
 * has been through the map space -> sRGB conversion, and the way back costs an ulp or two: on the CPU reference this moved 0 of
 * 60 000 nearest choices but 44 of 12 288 dithered ones on one of three synthetic scenes (a dither chain that meets a near-tie
 * diverges from there on).  With the 8-bit palette of that call the difference is large (about 30 % of the map): the bytes are a
 * different palette.
 * The *_device flavour takes device pointers for pixels / palette_map / quantized (map_elem_bytes 1 for up to 256 palette rows, else
 * 4); both palettes stay host memory. */
void patolette_amd_remap_u8(size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels, const double *palette,
                            const unsigned char *palette_u8, size_t palette_rows, int dither, void *palette_map, int map_elem_bytes,
                            unsigned char *quantized, int *exit_code);
void patolette_amd_remap_u8_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int channels,
                                   const double *palette, const unsigned char *palette_u8, size_t palette_rows, int dither,
                                   void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized, int *exit_code);
/* TESTS ONLY: by default a remap converts its pixels inside the map kernels where those exist -- the nearest map from 2^22 pixels on
 * with 8 .. 256 palette rows, the dither where it runs one lane per run (patolette_amd_dither_layout_in_use) -- so that no f64 image is
 * written; 1 makes every remap convert the image into f64 planes first (the route every other case takes), 0 restores the default.
 * Same map either way.  Process-wide; returns the previous setting. */
int patolette_amd_debug_remap_two_pass(int on);

/* ---- remap, ordered: a position-keyed (Bayer 8x8) dither, stable from frame to frame -----------
 * The Riemersma walk makes every choice depend on the sixteen before it along the curve, so one changed code value re-rolls the
 * rest of a frame: animations shimmer and their inter-frame deltas compress badly.  Here a choice depends on the pixel's bytes and
 * its position alone.  Arguments, palette handling (exactly one of the two; trailing -1 rows of the f64 one dropped), outputs, exit
 * codes and patolette_amd_last_error texts are those of patolette_amd_remap_u8; the pixel cap is that of dither == 0.
 * For the pixel at column x, row y OF ITS OWN FRAME, with bytes b[0..2] (a 4th byte is ignored), palette P and spread >= 0:
 *
 *   B(x, y)   = 8x8 Bayer index: v = 0; for i in 0,1,2: v = (v << 2) | ((((x>>i) ^ (y>>i)) & 1) << 1) | ((y>>i) & 1)
 *               taken on (x & 7, y & 7); first row 0 32 8 40 2 34 10 42, second row 48 16 56 24 50 18 58 26; a permutation of 0..63
 *   t         = ((double)B + 0.5) / 64.0 - 0.5                            in (-0.5, 0.5), mean 0 over a tile
 *   v[c]      = fmin(fmax((double)b[c] / 255.0 + spread * t, 0.0), 1.0)   the same grey shift on R, G, B; no FMA
 *   index     = nearest row of P to v, both through sRGB -> ICtCp exactly as patolette_amd_remap_u8(dither == 0) converts and
 *               compares: d = (d0*d0 + d1*d1) + d2*d2 in f64, ascending rows, strict '<' (lowest index on ties)
 *
 *   - spread == 0 is patolette_amd_remap_u8 with dither == 0, bit for bit.
 *   - No state passes between pixels or frames: the tile pattern restarts at every frame's origin.
 *   - quantized = pal8[index], as for the other remaps.
 *   - The shift is a lightness shift in gamma-encoded sRGB, the space in which equal steps look roughly equal; the comparison stays in
 *     ICtCp like every nearest map here.  A useful spread is the palette's typical per-channel step (Python: ordered_spread).
 *   spread not finite or negative: -1 with a "patolette_amd_remap:" text; a failed call leaves the thread's engine usable.
 *   Statistics: the ms_* fields as for a remap; every dither counter 0.  patolette_amd_last_map_palette: the palette in ICtCp.
 * One kernel (k_ordered_map): shift, conversion and an exact f64 search of the palette held in LDS; no f64 image, no tables. */
void patolette_amd_remap_ordered_u8(size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels,
                                    const double *palette, const unsigned char *palette_u8, size_t palette_rows, double spread,
                                    void *palette_map, int map_elem_bytes, unsigned char *quantized, int *exit_code);
void patolette_amd_remap_ordered_u8_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int channels,
                                           const double *palette, const unsigned char *palette_u8, size_t palette_rows, double spread,
                                           void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized, int *exit_code);

/* ---- frame deltas: an animation's index maps with "same as what is on screen" made transparent --
 * What a GIF or APNG encoder makes of every frame: the map with the unchanged positions replaced by a transparent index, and the dirty
 * rectangle.  n = width * height; m[f][p]: the input maps, frame after frame, as every *_frames_u8 / remap entry writes them, with
 * elements of map_elem_bytes (1, 2, 4 or 8; the *_device flavour: 1 or 4).  T = transparent_index: at least palette_rows and
 * representable in an element, so that it is an index no entry uses (1-byte maps with 256 rows have none: make the palette with one
 * row less).  palette_rows counts the rows of the palette as given, in [1, 2^31].
 *
 *   frame 0:      delta[0] = m[0], shown[0] = m[0]; the canvas is c = m[0]; rects[0] = (0, 0, width, height), changed[0] = n.
 *   frame f >= 1, every position p on its own, with a = m[f][p]:
 *     keep = (a == c[p]) || (tolerance > 0 && D <= tolerance * tolerance)
 *     D    = distance between the SOURCE pixel pixels[f][p] and the entry ON THE CANVAS, row c[p] of the palette, both through
 *            sRGB -> ICtCp exactly as patolette_amd_remap_u8(dither == 0) converts them (the pixel's bytes / 255.0, a byte palette
 *            likewise): D = (d0*d0 + d1*d1) + d2*d2 in f64, no FMA; evaluated only when a != c[p]
 *     keep:       delta[f][p] = T, the canvas stays.       otherwise: delta[f][p] = a, c[p] = a.       Both: shown[f][p] = c[p].
 *   rects[f]   = (x0, y0, w, h), four int32 per frame: the tight bounding box of the positions with delta[f] != T; (0, 0, 0, 0)
 *                when there is none.  changed[f] = their number.
 *
 * tolerance == 0 (the exact mode): pixels, channels and both palettes are not read; the pointers may be NULL.
 * tolerance > 0 (the lossy mode): pixels (frames x n, interleaved, channels = 3 or 4 bytes each; a 4th byte is ignored) and exactly
 *   one of palette (planar (palette_rows,3) f64 sRGB) and palette_u8, in the forms patolette_amd_remap_u8 takes; trailing
 *   (-1, -1, -1) rows of the f64 one are dropped.
 * Every element must be below palette_rows and must not name a dropped row: an element that does is never used as a palette
 *   address, the kernel raises a flag, and the call fails with -1 and a "patolette_amd_frame_deltas:" text (checked in both modes;
 *   what the outputs then hold is not defined).
 * Consequences:
 *   - Compositing the deltas gives back `shown`: start from delta[0]; in frame f overwrite the positions where delta[f] != T.
 *   - tolerance == 0: shown == the input maps.
 *   - tolerance > 0: every shown entry is the frame's own choice or lies within `tolerance` (ICtCp, Euclidean) of THAT frame's source
 *     pixel.  The comparison is always with the current source, never with an earlier frame: no error accumulates.
 *   - The device converts pixels with patolette_amd_pow (0.52 ulp): a D within an ulp or two of tolerance^2 may fall on the other
 *     side than in libm arithmetic.
 * Every output pointer may be NULL (delta_maps, shown_maps: frames x n elements of map_elem_bytes; rects: 4 * frames; changed:
 * frames).  delta_maps may be palette_maps itself.  The *_device flavour takes device pointers for palette_maps, pixels, delta_maps
 * and shown_maps; rects, changed and both palettes stay host memory.
 * Exit codes: -2 frames == 0 or an empty image; -4 beyond the pixel cap of patolette_amd_remap_u8(dither == 0); -1 (with a
 * "patolette_amd_frame_deltas:" text in patolette_amd_last_error) for a bad map_elem_bytes, no maps, bad channels, T < palette_rows,
 * T not representable, a tolerance that is negative or not finite, missing pixels or both or neither palette in the lossy mode, a
 * palette value that is not finite, or the flag above.  A failed call leaves the thread's engine usable.
 * Statistics: the ms_* fields as for a remap (ms_map: the kernel and its results), every other field 0.
 * Maps that already carry a transparent entry (those of patolette_amd_rgba and patolette_amd_remap_rgba_u8): here their index 0 is
 * compared like any other row; patolette_amd_frame_deltas_rgba below is the entry for them -- 0 as the deltas' transparent index,
 * per-frame disposal, and the lossy mode.
 * One kernel for all frames (k_frame_deltas): a lane owns a position, walks the frames and keeps the canvas entry in a register. */
void patolette_amd_frame_deltas(size_t frames, size_t width, size_t height, const void *palette_maps, int map_elem_bytes,
                                size_t palette_rows, size_t transparent_index, const unsigned char *pixels, int channels,
                                const double *palette, const unsigned char *palette_u8, double tolerance, void *delta_maps,
                                void *shown_maps, int32_t *rects, uint64_t *changed, int *exit_code);
void patolette_amd_frame_deltas_device(size_t frames, size_t width, size_t height, const void *d_palette_maps, int map_elem_bytes,
                                       size_t palette_rows, size_t transparent_index, const unsigned char *d_pixels, int channels,
                                       const double *palette, const unsigned char *palette_u8, double tolerance, void *d_delta_maps,
                                       void *d_shown_maps, int32_t *rects, uint64_t *changed, int *exit_code);

/* ---- frame deltas of RGBA maps: index 0 is the transparent entry, per-frame disposal -----------
 * The same step for the maps of patolette_amd_rgba / patolette_amd_remap_rgba_u8 with a transparent entry: index 0 means "this pixel
 * is transparent", indices 1 .. palette_rows-1 are opaque rows.  A GIF frame has one transparent index, and in a delta it has to mean
 * "leave the canvas as it is" -- which is what a decoder does with it under disposal 1 -- so here 0 in a delta means exactly that, and
 * no free index is needed (a one-byte map may use all 256 rows).  What a delta drawn over the canvas cannot express is a pixel that
 * turns from opaque to transparent: the frame BEFORE must be disposed to background (disposal 2) over a rectangle that covers the
 * pixel, and whatever was unchanged inside that rectangle is drawn again.
 *   frames, width, height, palette_maps, map_elem_bytes, palette_rows, pixels, channels, tolerance, the outputs' element sizes and the
 *       host / device flavours: as patolette_amd_frame_deltas takes them.  m[f][p]: the maps.
 *   palette, palette_u8: read in the lossy mode only, exactly one of them, in the forms patolette_amd_remap_rgba_u8 takes (trailing
 *       (-1, -1, -1) rows of the f64 one dropped).  Row 0's colour is never read, whatever it holds.
 *   loop: 1 when the animation repeats (frame 0 follows the last frame), 0 when it is shown once.
 *
 * Frame after frame; the canvas c starts as all 0.
 *   next(f) = f + 1; for the last frame 0 with loop, none without.
 *   V[f] = the tight box of the positions with m[f][p] != 0 && m[next(f)][p] == 0; empty without a next frame.  From the maps alone.
 *   disposals[f] = 2 if V[f] is not empty, otherwise 1.
 *   every position p on its own, with a = m[f][p]:
 *     a == 0: delta[f][p] = 0 (the canvas entry is 0 there already).
 *     a != 0: keep = c[p] != 0 && (a == c[p] || (tolerance > 0 && D <= tolerance * tolerance))
 *             D: exactly the D of patolette_amd_frame_deltas -- the source pixel pixels[f][p] against palette row c[p], through
 *             sRGB -> ICtCp, (d0*d0 + d1*d1) + d2*d2 in f64, no FMA; evaluated only where c[p] != 0 && a != c[p].
 *             keep: delta[f][p] = 0.     otherwise: delta[f][p] = a, c[p] = a.
 *     shown[f][p] = c[p].
 *   C[f] = the tight box of delta[f] != 0; changed[f] = their number.
 *   rects[f] = (x0, y0, w, h) of the smallest box holding C[f] and V[f]; (0, 0, 0, 0) when both are empty.
 *   then, if disposals[f] == 2: c[p] = 0 for every p inside rects[f].
 * Consequences:
 *   - shown[f] != 0 exactly where m[f] != 0: transparency is never lossy.
 *   - tolerance == 0: shown == the input maps.
 *   - A viewer that draws delta[f] inside rects[f] wherever it is not 0, then clears rects[f] where disposals[f] == 2, shows shown[f].
 *   - With loop the same holds on every later pass, whether or not the player resets the canvas at the restart: frame 0's deltas
 *     are all of its opaque positions, and V of the last frame clears what frame 0 shows as transparent.
 *   - An empty rectangle only occurs with disposal 1.  A frame whose deltas are all 0 can still have a rectangle (its V).
 *   - Maps without any 0 (fully opaque): every disposal is 1, and from frame 1 on deltas, shown, rects and changed are those of
 *     patolette_amd_frame_deltas with T read as 0.
 * Outputs, each may be NULL: delta_maps, shown_maps (frames x n elements of map_elem_bytes; delta_maps may be palette_maps itself);
 *   rects (int32[4 * frames]); disposals (int32[frames], each 1 or 2); changed (uint64[frames]).  The *_device flavour takes device
 *   pointers for palette_maps, pixels, delta_maps and shown_maps; rects, disposals, changed and both palettes stay host memory.
 * Every element must be below palette_rows and must not name a dropped row: an element that does is never used as a palette
 *   address, the kernel raises a flag, and the call fails with -1 and a "patolette_amd_frame_deltas_rgba:" text (both modes; what the
 *   outputs then hold is not defined).
 * Exit codes: -2 frames == 0 or an empty image; -4 beyond the pixel cap of patolette_amd_remap_u8(dither == 0); -1 (with a
 *   "patolette_amd_frame_deltas_rgba:" text in patolette_amd_last_error) for a bad map_elem_bytes, no maps, palette_rows outside
 *   [1, 2^31], a tolerance that is negative or not finite, a loop that is not 0 or 1, and in the lossy mode bad channels, missing
 *   pixels, both or neither palette, a palette value that is not finite; or the flag above.  A failed call leaves the thread's engine
 *   usable.
 * Statistics: as patolette_amd_frame_deltas.
 * Kernels: k_rgba_vanish, one launch for every frame's V and the flag; then k_frame_delta_rgba once per frame on the library's
 *   stream -- rects[f - 1] is a grid-wide result that frame f's canvas needs, so the chain over frames is a chain of launches; no
 *   host turn and no wait in between.  The host unites C and V once at the end.
 * Out of scope: disposal 3; a colour table per frame (patolette_amd_frame_deltas_local has them for maps without a transparent
 *   entry of their own). */
void patolette_amd_frame_deltas_rgba(size_t frames, size_t width, size_t height, const void *palette_maps, int map_elem_bytes,
                                     size_t palette_rows, const unsigned char *pixels, int channels, const double *palette,
                                     const unsigned char *palette_u8, double tolerance, int loop, void *delta_maps, void *shown_maps,
                                     int32_t *rects, int32_t *disposals, uint64_t *changed, int *exit_code);
void patolette_amd_frame_deltas_rgba_device(size_t frames, size_t width, size_t height, const void *d_palette_maps, int map_elem_bytes,
                                            size_t palette_rows, const unsigned char *d_pixels, int channels, const double *palette,
                                            const unsigned char *palette_u8, double tolerance, int loop, void *d_delta_maps,
                                            void *d_shown_maps, int32_t *rects, int32_t *disposals, uint64_t *changed, int *exit_code);

/* TESTS ONLY: k_frame_deltas (and the kernels of patolette_amd_frame_deltas_rgba) give a lane four consecutive positions (one 4- or
 * 16-byte access) where width * height is a multiple of
 * 4, the buffers are aligned for it and the frame is large enough to keep the GPU full with a quarter of the wavefronts (2^21 pixels
 * on an MI355X); otherwise one.  1 takes four wherever sizes and addresses allow, 0 never, -1 restores that rule.  Same results
 * either way.  Process-wide; returns the previous mode. */
int patolette_amd_debug_delta_quad(int mode);

/* ---- frame deltas with a colour table per frame: colour-keyed, for GIF local colour tables -------
 * patolette_amd_frame_deltas for a clip whose frames (or scenes) each have a palette of their own.  Indices of two tables do not
 * compare, so the canvas is what a viewer's canvas is: a colour.
 *   frames, width, height, pixels, channels, tolerance, rects, changed, exit_code and the host / device flavours: as
 *       patolette_amd_frame_deltas takes them; the same pixel cap.  n = width * height.
 *   palette_maps: m[f][p], frames x n elements of ONE byte (a GIF table has at most 256 rows: there is no map_elem_bytes).
 *   palettes_u8: host memory, palette_count x palette_rows x 3 bytes: P = palette_count tables of K = palette_rows rows each, K in
 *       [1, 255], P in [1, 65536].  Bytes only: a GIF stores bytes, and the exact mode compares bytes.
 *   palette_of: host memory, int32[frames], each in [0, P): frame f is drawn with table g(f) = palette_of[f] -- a palette per scene,
 *       per frame, or any grouping.  NULL: g(f) = f, which requires P == frames.
 *   transparent_index T, in [K, 255]: the one index no table uses, the same in every frame.
 *   col(f, a): the three bytes of row a of table g(f).
 *
 *   frame 0:      delta[0] = m[0]; the canvas colour is C[p] = col(0, m[0][p]); shown_rgb[0][p] = C[p];
 *                 rects[0] = (0, 0, width, height), changed[0] = n.
 *   frame f >= 1, every position p on its own, with a = m[f][p]:
 *     keep = (col(f, a) == C[p]) || (tolerance > 0 && D <= tolerance * tolerance)        (the equality: over the three bytes)
 *     D    = exactly the D of patolette_amd_frame_deltas: the SOURCE pixel pixels[f][p] against the colour ON THE CANVAS, both
 *            through sRGB -> ICtCp as that entry converts a pixel and a row of a byte palette, D = (d0*d0 + d1*d1) + d2*d2 in f64,
 *            no FMA; evaluated only where the bytes differ.  The canvas colour's ICtCp value is that of the palette row it was drawn
 *            from, prepared as patolette_amd_frame_deltas prepares palette_u8; equal bytes give equal values, whichever row.
 *     keep:       delta[f][p] = T, the canvas stays.       otherwise: delta[f][p] = a, C[p] = col(f, a).       Both: shown_rgb[f][p] = C[p].
 *   rects[f], changed[f]: as patolette_amd_frame_deltas -- the tight box of delta[f] != T, (0, 0, 0, 0) when there is none; their number.
 *
 * Outputs, each may be NULL: delta_maps (frames x n bytes; may be palette_maps itself); shown_rgb (frames x n x 3 bytes, interleaved:
 *   what a viewer shows after each frame -- colours, because indices of different tables do not compare); rects (int32[4 * frames]);
 *   changed (uint64[frames]).  The *_device flavour takes device pointers for palette_maps, pixels, delta_maps and shown_rgb;
 *   palettes_u8, palette_of, rects and changed stay host memory.
 * tolerance == 0: pixels and channels are not read.
 * Consequences:
 *   (a) Drawing delta[f] with table g(f) over the canvas, skipping T, shows shown_rgb[f].
 *   (b) tolerance == 0: shown_rgb[f][p] == col(f, m[f][p]).
 *   (c) Every table identical: with pairwise distinct rows, delta_maps, rects and changed are those of patolette_amd_frame_deltas with
 *       that table as palette_u8, bit for bit, at every tolerance (P == 1 is the simplest case).  With duplicate rows, a position
 *       whose index changed but whose colour did not is kept here and drawn there.
 *   (d) tolerance > 0: every shown colour is the frame's own choice or lies within `tolerance` of THAT frame's source pixel; nothing
 *       accumulates.
 * Every element must be below K: one that is not is never used as an address, the kernel raises a flag, and the call fails with -1 and
 *   a "patolette_amd_frame_deltas_local:" text (both modes; what the outputs then hold is not defined).
 * Exit codes: -2 and -4 as patolette_amd_frame_deltas; -1 (with a "patolette_amd_frame_deltas_local:" text in
 *   patolette_amd_last_error) for no maps, K, P or T out of range, no palettes, a palette_of value out of range, NULL palette_of with
 *   P != frames, a tolerance that is negative or not finite, in the lossy mode bad channels or missing pixels; or the flag above.
 *   A failed call leaves the thread's engine usable.
 * Statistics: as patolette_amd_frame_deltas.
 * One kernel for all frames (k_frame_deltas_local, then k_delta_boxes as there): a lane keeps the canvas colour's packed word and, for
 *   the lossy compare, the row it came from; the P K rows' words are staged in LDS where they are few, read from global memory
 *   otherwise.  The outputs are a function of the arguments alone.
 * Out of scope: maps with a transparent entry of their own and per-frame disposal (a local patolette_amd_frame_deltas_rgba). */
void patolette_amd_frame_deltas_local(size_t frames, size_t width, size_t height, const unsigned char *palette_maps,
                                      const unsigned char *palettes_u8, size_t palette_count, size_t palette_rows, const int32_t *palette_of,
                                      size_t transparent_index, const unsigned char *pixels, int channels, double tolerance,
                                      unsigned char *delta_maps, unsigned char *shown_rgb, int32_t *rects, uint64_t *changed, int *exit_code);
void patolette_amd_frame_deltas_local_device(size_t frames, size_t width, size_t height, const unsigned char *d_palette_maps,
                                             const unsigned char *palettes_u8, size_t palette_count, size_t palette_rows,
                                             const int32_t *palette_of, size_t transparent_index, const unsigned char *d_pixels, int channels,
                                             double tolerance, unsigned char *d_delta_maps, unsigned char *d_shown_rgb, int32_t *rects,
                                             uint64_t *changed, int *exit_code);

/* TESTS ONLY: where k_frame_deltas_local reads the tables' packed rows.  -1: the launcher's rule (LDS when P * K is at most 4096 and at
 * most 256 * frames, so that a block's fill costs no more than its element loads), 0: always global memory, 1: LDS whenever P * K is
 * at most 4096.  Same results.  Process-wide; returns the previous mode.  patolette_amd_debug_delta_local_route: what the last launch
 * of this process took -- 1 LDS, 0 global memory, -1 before the first. */
int patolette_amd_debug_delta_local_tables(int mode);
int patolette_amd_debug_delta_local_route(void);

/* ---- measure: what a map costs, per palette entry and per frame ---------------------------------
 * The error of any map this library (or anything else) made of 8-bit pixels on a palette, without pixels, maps or quantized images
 * leaving the GPU: the figures a caller needs to choose a palette size, a dither mode, a spread or a frame-delta tolerance, and the
 * per-entry pixel counts encoders sort palettes by.  n = width * height, N = frames * n.
 *   pixels, channels, palette, palette_u8, palette_rows: exactly as patolette_amd_remap_u8 takes them -- interleaved 8-bit sRGB with 3
 *       or 4 channels (a 4th byte is ignored); exactly one of palette (column-major f64, trailing (-1, -1, -1) rows dropped) and
 *       palette_u8.
 *   palette_maps, map_elem_bytes: as patolette_amd_frame_deltas takes them -- m[f][p], frame after frame, elements of 1, 2, 4 or 8
 *       bytes (the *_device flavour: 1 or 4).
 *   skip_index: -1 for none, or an index whose positions are left out (a transparent index).
 *
 * For frame f and position p with a = m[f][p]:
 *   skip_index >= 0 and a == skip_index: the position is SKIPPED and enters nothing.  This test comes first, so skip_index may be
 *       a palette row (index 0 of patolette_amd_rgba's maps) or lie beyond the rows (the T of patolette_amd_frame_deltas).  A
 *       skip_index that no element of map_elem_bytes can hold skips nothing.
 *   otherwise a must be a used row (below palette_rows, not a dropped trailing row).  An element that is not is never used as an
 *       address; the kernel raises a flag and the call fails with -1 and a "patolette_amd_measure:" text (what the outputs then hold
 *       is not defined).
 *   Integer part.  pal8 = the byte palette of the remap contract: palette_u8 as given, or clip(palette * 255, 0, 255) truncated.
 *       e = sum over c of (b[c] - pal8[a][c])^2, an integer in [0, 195075], b the pixel's bytes.
 *       entry_count[a] += 1; entry_sse[a] += e; entry_max_se[a] = max(entry_max_se[a], e); the same three for frame f.
 *       Rows that nothing names hold 0, a frame with every position skipped holds 0.  Sums of integers: exact, independent of any
 *       order.  This is the squared error, in code values, of the `quantized` image every entry here returns for that map;
 *       3 * 255^2 * count / sse is the argument of the PSNR's logarithm.
 *   ICtCp part, evaluated only when frame_d_sum or frame_d_max is given (otherwise no pixel is converted).
 *       D = exactly the D of the frame-deltas contract: the pixel's bytes / 255.0 and row a of the palette AS GIVEN (the f64 rows,
 *       not pal8; a byte palette's v / 255.0), both through sRGB -> ICtCp as patolette_amd_remap_u8(dither == 0) converts them;
 *       D = (d0*d0 + d1*d1) + d2*d2 in f64, no FMA.  frame_d_sum[f] = sum of D, frame_d_max[f] = max of D, both 0 for a frame with
 *       nothing in it.  This is the quantity the palette was fitted to, and the square of the unit of the frame deltas' tolerance.
 *       frame_d_max is exact given the D's.  frame_d_sum is a sum in an order that depends on (frames, width, height, the number
 *       of used palette rows) only: it is a function of the arguments alone -- the same call gives the same bits every time, on any
 *       stream, engine or workspace history, from this entry and the *_device one alike.  No floating-point atomic is involved.
 *       The device converts with patolette_amd_pow (0.52 ulp), so the D's agree with libm arithmetic to about 1e-15 relative.
 * Outputs, host memory in both flavours, each may be NULL: entry_count, entry_sse (uint64) and entry_max_se (uint32), palette_rows
 *   values each; frame_count, frame_sse (uint64), frame_max_se (uint32), frame_d_sum, frame_d_max (f64), `frames` values each.
 * The *_device flavour takes device pointers for pixels and palette_maps; both palettes stay host memory.
 * Exit codes: 0; -2 frames == 0 or an empty image; -4 beyond the pixel cap of patolette_amd_remap_u8(dither == 0); -1 (with a
 *   "patolette_amd_measure:" text in patolette_amd_last_error) for bad channels or map_elem_bytes, no pixels, no maps, both or
 *   neither palette, palette_rows outside [1, 2^31], no usable palette row or one that is not finite, skip_index < -1, or the flag
 *   above.  A failed call leaves the thread's engine usable.
 * Statistics: the ms_* fields as for a remap (ms_map: the kernels and their results), every other field 0.
 * Two kernels: k_measure, one launch for all frames (integer LDS atomics per entry, a plain store per tile), and k_measure_fold. */
void patolette_amd_measure(size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels,
                           const void *palette_maps, int map_elem_bytes, const double *palette, const unsigned char *palette_u8,
                           size_t palette_rows, long long skip_index, uint64_t *entry_count, uint64_t *entry_sse,
                           uint32_t *entry_max_se, uint64_t *frame_count, uint64_t *frame_sse, uint32_t *frame_max_se,
                           double *frame_d_sum, double *frame_d_max, int *exit_code);
void patolette_amd_measure_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int channels,
                                  const void *d_palette_maps, int map_elem_bytes, const double *palette,
                                  const unsigned char *palette_u8, size_t palette_rows, long long skip_index, uint64_t *entry_count,
                                  uint64_t *entry_sse, uint32_t *entry_max_se, uint64_t *frame_count, uint64_t *frame_sse,
                                  uint32_t *frame_max_se, double *frame_d_sum, double *frame_d_max, int *exit_code);

/* ---- gif_lzw: index maps LZW-compressed as a GIF's image data, on the device ------------------
 * The last step of the animation pipeline: the GIF flavour of LZW over every frame's map (or over its dirty rectangle), so that what
 * leaves the GPU is the compressed stream and not the map.  A GIF decoder forgets its dictionary at every Clear code, so a frame's
 * symbols are cut into segments that are compressed independently, each ending in a Clear, and the segments' bit strings are put end
 * to end: any decoder reads the result as one stream.
 *   maps: frames x width x height elements of ONE byte (a GIF palette has at most 256 entries), frame after frame, as every
 *       *_frames_u8 / remap / frame_deltas entry writes 1-byte maps.  Host memory; the *_device flavour takes a device pointer.
 *   rects: host memory, int32[4 * frames], rows (x0, y0, w, h) as patolette_amd_frame_deltas writes them, or NULL for the full frame
 *       every time.  Every rectangle must lie inside the frame and have w, h >= 1 (an empty one -- frame_deltas' (0, 0, 0, 0) -- is
 *       a -1: pass (0, 0, 1, 1), whose one delta is the transparent index).  Elements outside the rectangles are not read by the kernels.
 *   min_code_size m, in [2, 8]: every element inside a rectangle must be below 2^m.
 *   segment: symbols per segment; 0 takes the default 8192, otherwise it must lie in [1, 2^24].  Segments cost size (the dictionary
 *       starts again at each) and buy parallelism: one chain per segment.
 * Outputs, host memory in both flavours: out, with `capacity` bytes; offsets, uint64[frames + 1].  Frame f's stream is
 *   out[offsets[f] : offsets[f + 1]]; the streams lie back to back and each starts on a byte.  A stream is the raw LZW byte stream,
 *   NOT yet cut into the container's 255-byte sub-blocks.
 *
 * Per frame: the elements of its rectangle in row-scan order, q -> (y0 + q / w, x0 + q % w), are a sequence of area = w * h symbols,
 * cut into nseg = ceil(area / segment) segments of `segment` symbols, the last one shorter.  clear = 2^m, eoi = clear + 1; codes are
 * packed least-significant bit first.
 *   - The stream opens with `clear` at width m + 1.
 *   - Every segment starts from an empty dictionary with free = eoi + 1 and width = m + 1 and runs the classic greedy LZW over its
 *     symbols, the first symbol being the first prefix.  For every further symbol `byte`: if (prefix, byte) is in the dictionary, its
 *     code becomes the prefix.  On a miss: emit prefix at width; then, if free < 4096, enter the pair as code `free`, increment width
 *     if free == 2^width and width < 12, then increment free; otherwise (the dictionary is full) emit clear at width and reset the
 *     dictionary, free and width.  Either way `byte` becomes the new prefix.
 *   - At the segment's end: emit the pending prefix at width; then, if free < 4096, free == 2^width and width < 12, increment width
 *     (the decoder makes an entry on that code too); then emit the closing code at width: clear for every segment but the last,
 *     eoi for the last.
 *   - The last byte is padded with zero bits.
 *   tests/lzw_ref.py states the same in Python; the device's bytes equal its bytes.
 * The flag: an element >= 2^m inside a rectangle is never used as a dictionary key; the kernel raises a flag and the call fails with
 *   -1 and a "patolette_amd_gif_lzw:" text (what `out` then holds is not defined).
 * Capacity: a frame emits at most area + 2 * nseg + area / 3000 + 2 codes of at most 12 bits, so
 *   sum over the frames of ceil(12 * (area + 2 * nseg + area / 3000 + 2) / 8) bytes always suffice.  If `capacity` is smaller than the
 *   streams, the call fails with -1, offsets (all of them; offsets[frames] = the bytes needed) are written and nothing is copied to out.
 * Exit codes: 0; -2 frames == 0 or an empty image; -4 beyond the pixel cap of patolette_amd_remap_u8(dither == 0); -1 (with a
 *   "patolette_amd_gif_lzw:" text in patolette_amd_last_error) for no maps, no offsets, no out with a capacity, min_code_size or
 *   segment out of range, a rectangle that is empty or not inside the frame, the flag, or the capacity.  A
 *   failed call leaves the thread's engine usable.
 * Statistics: the ms_* fields as for a remap (ms_map: the kernels and the offsets), every other field 0.
 * Three kernels, one launch each for all frames, integers only: k_lzw_segments (a wavefront per segment, its dictionary a hash table in
 *   LDS), k_lzw_offsets (the segments' and frames' places), k_lzw_pack (the segments' bits shifted together).
 * Out of scope: the container (Python: write_gif, local colour tables included: this stage reads no palette), interlaced images. */
void patolette_amd_gif_lzw(size_t frames, size_t width, size_t height, const unsigned char *maps, const int32_t *rects,
                           int min_code_size, size_t segment, unsigned char *out, size_t capacity, uint64_t *offsets, int *exit_code);
void patolette_amd_gif_lzw_device(size_t frames, size_t width, size_t height, const unsigned char *d_maps, const int32_t *rects,
                                  int min_code_size, size_t segment, unsigned char *out, size_t capacity, uint64_t *offsets,
                                  int *exit_code);

/* ---- gif_lzw_lossy: the same streams, shorter, where a nearly equal colour may continue a match ---
 * The lossy LZW coder of the GIF tools: when the next symbol would end the current dictionary match, the coder may continue the match
 * with a NEARLY EQUAL colour instead.  Ordered-dithered maps, whose pattern breaks every long match of the exact coder, gain most.
 * Everything of patolette_amd_gif_lzw stays -- maps, rects, min_code_size m, segment, out, capacity, offsets, the segments, the opening
 * Clear, the width rule, the closing code, the Clear of a full dictionary, frames from byte boundaries, the capacity bound (still at
 * most one code per symbol) -- but the step.  With the current prefix P and the next symbol s (never the first symbol of a segment,
 * which is taken as it is):
 *     for c in [s] + near[s][1 .. near[s][0]], in this order:
 *         if (P, c) is in the dictionary: P = its code; the step has coded c; next symbol
 *     no candidate is in the dictionary -- exactly the old miss: emit P; enter (P, s) if free < 4096 (the width step as before), else
 *         emit Clear and reset; P = s; the step has coded s.
 * Greedy, one step of look-ahead, deterministic: the exact symbol wins over any candidate, an earlier candidate over a later one, and
 * a miss enters the TRUE symbol.  tests/lzw_lossy_ref.py states the same in Python; the device's bytes and coded maps equal its own.
 *   near: host memory in both flavours, 4096 bytes, uint8[256][16].  near[s][0] is the count, in [0, 15]; near[s][1 .. count] are the
 *       candidates in order of preference; the rest of a row is not read, nor is any row at or above 2^m.  Checked before anything is
 *       enqueued: every count read must be <= 15 and every candidate read below 2^m, else -1.  Duplicates and a candidate equal to s are
 *       allowed and harmless.  NULL is a -1.  patolette_amd_gif_neighbours makes the table of a palette; any table of this layout serves.
 *   coded: NULL, or frames x width x height bytes that do not overlap maps (-1 if they do): inside every rectangle, at the position
 *       each symbol came from, the symbol its step coded.  Positions outside the rectangles are not written.  Host memory; the
 *       *_device flavour takes device pointers for maps and coded.
 * What follows from the rule:
 *   (a) frame f's stream decodes to coded[f] inside its rectangle;
 *   (b) the stream of `maps` under `near` is bit for bit the EXACT coder's stream of `coded` (by induction over the steps: the exact
 *       coder on the coded symbols hits where this one hit and misses where it missed, with the same dictionary): patolette_amd_gif_lzw
 *       on `coded` returns the same bytes;
 *   (c) every coded element is the map's element or one of its row's candidates;
 *   (d) a symbol with an empty row that appears in no row -- a transparent index -- is never replaced and never replaces: transparency
 *       is never lossy;
 *   (e) with every count 0 the bytes are patolette_amd_gif_lzw's;
 *   (f) the first symbol of every segment is exact.
 * With the table of patolette_amd_gif_neighbours at tolerance t, a coded entry lies within t (ICtCp) of the MAP's entry, not of the
 * source pixel.  Behind patolette_amd_frame_deltas(tolerance t1) every pixel a viewer shows lies within t1 + t of its frame's source
 * or within t of the frame's own choice; nothing accumulates over the frames, because every drawn pixel is coded from that frame's own
 * entry.  patolette_amd_measure on the composited coded maps gives the true cost.
 * Flag, capacity, exit codes and statistics: as patolette_amd_gif_lzw, the text starting "patolette_amd_gif_lzw_lossy:"; -1 also for
 *   no near, a bad table, and coded overlapping maps.  What coded holds after a failed call is not defined.
 * Three kernels, one launch each: k_lzw_lossy_segments (lane j < 16 of the segment's wavefront probes the dictionary for candidate j in
 *   the same step; a ballot's lowest hit wins), then k_lzw_offsets and k_lzw_pack as they are. */
void patolette_amd_gif_lzw_lossy(size_t frames, size_t width, size_t height, const unsigned char *maps, const int32_t *rects,
                                 int min_code_size, size_t segment, const unsigned char *near, unsigned char *coded, unsigned char *out,
                                 size_t capacity, uint64_t *offsets, int *exit_code);
void patolette_amd_gif_lzw_lossy_device(size_t frames, size_t width, size_t height, const unsigned char *d_maps, const int32_t *rects,
                                        int min_code_size, size_t segment, const unsigned char *near, unsigned char *d_coded,
                                        unsigned char *out, size_t capacity, uint64_t *offsets, int *exit_code);

/* ---- png_deflate: index maps deflated as an indexed PNG's image data, on the device ---------------
 * The other way out of the pipeline: PNG and APNG.  What leaves the GPU is every frame's raw deflate stream (RFC 1951, no zlib
 * wrapper) and the Adler-32 the zlib trailer needs; the container is a few bytes around them (Python: write_png, write_apng).
 *   maps, rects, out, capacity, offsets: as patolette_amd_gif_lzw takes them.  Every byte value is a legal element: no min_code_size
 *       and no flag.  Elements outside the rectangles are not read.
 *   segment: filtered bytes per segment; 0 takes the default 16384, otherwise it must lie in [1, 32768].
 *   adler: host memory, uint32[frames]: the Adler-32 of every frame's filtered stream (zlib's adler32).
 * What is coded: per frame the PNG scanline stream of its rectangle at bit depth 8 with filter type 0 -- h rows, each a zero byte and
 *   the row's w indices: the filtered stream, h * (w + 1) bytes.  It is cut into nseg = ceil(h * (w + 1) / segment) segments; a
 *   wavefront codes a segment as ONE deflate block, the last of a frame carrying BFINAL; the blocks lie bit to bit, every frame starts
 *   on a byte and its last byte is padded with zero bits.  zlib's inflate of out[offsets[f] : offsets[f + 1]] (raw, window 15) returns
 *   the filtered stream byte for byte: that, not a model of the coder, is what the tests check.
 *   - A segment is parsed on its own and gets its own code tables, but a match may start up to 32768 bytes back in the same frame's
 *     filtered stream, before the segment's start too; no match runs beyond its segment's end.  Lengths 3 .. 258, distances 1 .. 32768.
 *   - Candidates at every position: the distances 1, 2, 4, 8, R - 1, R, R + 1, 2R, 4R, 8R with R = w + 1 (the pixel above, its
 *     neighbours, and the rows of an 8 x 8 ordered dither's period), up to four distances that the segment's explorations have found,
 *     and the last earlier position of the segment with the same three bytes (a hash table; the latest position wins, never the first
 *     lane to arrive).  The longest wins, among equals the first in that order; a match of 3 further back than 4096 is dropped; one
 *     step of lazy evaluation (the match one byte on, if longer).
 *   - An exploration tries EVERY distance of the window at one position (the first free one of a step of 64 positions) and keeps the
 *     longest match, the nearest among equals; 8 bytes and more put its distance in front of the four remembered ones.  It runs when
 *     the step before left more than 2 tokens; one that finds nothing makes the next ones wait 1, 3, 7, 15, 15, ... steps.  An
 *     image repeats at few distances (a dither's tile, a row, a sprite's step) which a one-entry hash bucket does not find.
 *   - Block type: dynamic Huffman with length-limited codes (15 bits; 7 for the code-length code), or the fixed code where that is
 *     no larger.  csrc/deflate_codes.h holds the tables' routines for the host and the device alike.
 *   The bytes are a function of the arguments alone.
 * Capacity: a block under the fixed code takes at most 9 bits a byte and 10 more, so
 *   sum over the frames of ceil((9 * h * (w + 1) + 10 * nseg) / 8) bytes always suffice.  With less `capacity` than the streams
 *   need the call fails with -1, offsets (all of them; offsets[frames] = the bytes needed) and adler are written and nothing is copied.
 * Exit codes: as patolette_amd_gif_lzw, the text starting "patolette_amd_png_deflate:"; -1 also for no adler; -4 also when the
 *   segments number 2^31 and more.  A failed call leaves the thread's engine usable.
 * Statistics: as patolette_amd_gif_lzw.
 * Four kernels, one launch each for all frames, integers only: k_png_filter (the filtered streams), k_deflate_segments (parse, tables
 *   and bits of a segment, a wavefront each), then k_lzw_offsets and k_lzw_pack as they are.
 * Out of scope: bit depths below 8, filters other than 0, interlace, true-colour PNG, lossy coding. */
void patolette_amd_png_deflate(size_t frames, size_t width, size_t height, const unsigned char *maps, const int32_t *rects, size_t segment,
                               unsigned char *out, size_t capacity, uint64_t *offsets, uint32_t *adler, int *exit_code);
void patolette_amd_png_deflate_device(size_t frames, size_t width, size_t height, const unsigned char *d_maps, const int32_t *rects,
                                      size_t segment, unsigned char *out, size_t capacity, uint64_t *offsets, uint32_t *adler,
                                      int *exit_code);
/* tests: one deflate block as the HOST writes it for a token list, by the routines the kernel shares with it (csrc/deflate_codes.h,
 *   write_block).  Host code only: it never touches the device and works without one.
 *   tokens[count]: a literal (0 .. 255) or 0x80000000 | (length - 3) << 16 | (distance - 1) with length 3 .. 258 and distance
 *   1 .. 32768; the end of block is appended here.  final_block: BFINAL.  The block starts at bit 0 of out[0]; *bits = its bits, and
 *   its ceil(bits / 8) bytes go to out when capacity holds them (the last byte's unused bits zero).
 * Returns 0; -1 for a null argument, a token that is none of the above or too little capacity (*bits is still written then). */
int patolette_amd_debug_deflate_block(const uint32_t *tokens, size_t count, int final_block, unsigned char *out, size_t capacity,
                                      uint64_t *bits);

/* The lossy coder's table for a palette.  Host code only: it never touches the device and works without one.
 *   palette / palette_u8, palette_rows: exactly one of the two, as patolette_amd_remap_u8 takes them (trailing (-1, -1, -1) rows of an
 *       f64 palette are dropped); palette_rows in [1, 256].
 *   Every used row goes through the sRGB -> ICtCp conversion exactly as patolette_amd_frame_deltas prepares its palette, and
 *   D = (d0*d0 + d1*d1) + d2*d2 in f64, no FMA, between two rows is the D of that contract.
 *   near_out: 4096 bytes, all written.  Row s lists the OTHER used rows e with D <= tolerance^2, by (D ascending, e ascending), cut to
 *       max_neighbours in [0, 15].  transparent_index (-1: none, else in [0, 255]) is left out both as s and as e.  Dropped rows and
 *       rows >= palette_rows have count 0 and appear nowhere.  At tolerance 0 only identical rows are neighbours.
 * Exit codes: 0; -1 with a "patolette_amd_gif_neighbours:" text for both or neither palette, palette_rows, transparent_index or
 *   max_neighbours out of range, a tolerance that is negative or not finite, a palette value that is not finite, every row the
 *   unused-row fill, or no near_out. */
void patolette_amd_gif_neighbours(const double *palette, const unsigned char *palette_u8, size_t palette_rows, int transparent_index,
                                  double tolerance, int max_neighbours, unsigned char *near_out, int *exit_code);

/* ---- RGBA images: a transparent palette slot, an alpha-aware dither ---------------------------
 * pixels: width*height interleaved 8-bit RGBA.  Pixel i is TRANSPARENT iff alpha_i < alpha_threshold (an integer in [0, 256]);
 * every other pixel is OPAQUE.  M = number of opaque pixels, N = width*height.
 *   M == N (no transparent pixel; always for alpha_threshold 0): bit for bit what patolette_amd_u8() returns for the RGB bytes with
 *       the same options (f64 palette, palette bytes, map); palette_rgba[:, 3] = 255 on used rows; *transparent_index = -1.
 *   0 < M < N: index 0 is the transparent entry -- f64 palette row 0 = (0, 0, 0), palette_rgba[0] = (0, 0, 0, 0),
 *       *transparent_index = 0.  Rows 1 .. palette_size-1 are what patolette() returns with palette_size-1 colours for the (M, 3)
 *       list of opaque pixels in row-scan order (their weights, in the same order; same options); unused rows -1 in the f64 palette
 *       and (0, 0, 0, 0) in palette_rgba.  Map: 0 for a transparent pixel, 1 + that call's nearest-entry index for an opaque one; with
 *       dithering, 1 + the choice of the reference's Riemersma walk over the width x height image on which transparent pixels are
 *       treated exactly like positions outside the image (not dithered, the error queue unchanged): the chain visits the opaque
 *       pixels in Hilbert order.
 *   M == 0: success; row 0 is the transparent entry, every other row unused; the map is all 0; *transparent_index = 0.
 * quantized: width*height x 4 interleaved = palette_rgba[palette_map] (opaque pixels have alpha 255).
 * weights: NULL or N values, of which the opaque pixels' are used.  tile_size > 0 and no weights: the saliency weights are computed
 * over the full image's RGB exactly as patolette_amd_u8() computes them (the RGB hidden under transparent pixels reaches the
 * saliency map too), then restricted to the opaque pixels.  palette_only: the palettes as above, no map.
 * Exit codes: as patolette_amd_u8(); -3 also for palette_size < 2 when opaque and transparent pixels are both present; -1 for an
 * alpha_threshold outside [0, 256] (patolette_amd_last_error says why).  map_elem_bytes: 1, 2, 4 or 8, able to hold palette_size-1.
 * Every output but exit_code may be NULL.  The *_device flavour takes device pointers for pixels / weights / palette_map /
 * quantized (palette_map and quantized aligned to their element size, as hipMalloc returns them); palette, palette_rgba and
 * transparent_index stay host memory. */
void patolette_amd_rgba(size_t width, size_t height, const unsigned char *pixels, int alpha_threshold, const double *weights,
                        double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                        unsigned char *palette_rgba, void *palette_map, int map_elem_bytes, unsigned char *quantized,
                        int *transparent_index, int *exit_code);
void patolette_amd_rgba_device(size_t width, size_t height, const unsigned char *d_pixels, int alpha_threshold, const double *d_weights,
                               double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                               unsigned char *palette_rgba, void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized,
                               int *transparent_index, int *exit_code);

/* ---- remap with alpha: RGBA images and frames onto a palette the CALLER gives -------------------
 * What patolette_amd_remap_u8 is to patolette_amd_u8, this is to patolette_amd_rgba: no palette is made; `frames` images of
 * width x height, interleaved 8-bit RGBA (4 bytes per pixel), one after another, are mapped onto the given palette, of which row 0 may
 * be a transparent entry.  n = width * height, N = frames * n.
 *   Transparency.  A pixel is TRANSPARENT iff its alpha < alpha_threshold (an integer in [0, 256]), else OPAQUE: the rule of
 *       patolette_amd_rgba.
 *   Palette.  palette / palette_u8 / palette_rows exactly as patolette_amd_remap_u8 takes them (exactly one of the two; trailing
 *       (-1, -1, -1) rows of the f64 one are dropped as there; every remaining row finite).
 *       transparent_index ==  0: row 0 is the transparent entry.  Its colour is never a candidate for any pixel and its quantized
 *                                value is (0, 0, 0, 0), whatever the row holds.
 *       transparent_index == -1: there is no transparent entry; every row is a candidate.
 *       The OPAQUE ROWS are the used rows without the transparent entry; at least one must remain, else -1.  off = 1 when row 0 is
 *       the transparent entry, else 0.
 *   mode 0 (nearest), 2 (ordered; `spread` is read in this mode only).  An opaque pixel's element is off + e, where e is exactly the
 *       element patolette_amd_remap_u8(dither == 0) resp. patolette_amd_remap_ordered_u8(spread) writes for that pixel -- its bytes, at
 *       its place in its own frame -- with the palette made of the opaque rows only.  Both maps are per pixel, so the RGB hidden under
 *       transparent pixels cannot matter.
 *   mode 1 (Riemersma).  Frame by frame the reference's walk over that frame's own width x height curve from an empty error queue, on
 *       the opaque rows, with transparent pixels treated exactly like positions outside the image (no choice, the queue unchanged) --
 *       the rule of patolette_amd_rgba; element off + the walk's choice.  No state passes between frames.  A frame without a
 *       transparent pixel is therefore the walk of patolette_amd_remap_u8(dither != 0) on its RGB; a 1 x 1 frame gets entry off.
 *   Transparent pixels: element 0 and quantized (0, 0, 0, 0).
 *   Opaque pixels: quantized = (pal8[element], 255), pal8 as the remap contract defines it (palette_u8 as given, or
 *       clip(palette * 255, 0, 255) truncated).
 *   A transparent pixel while transparent_index == -1 has no element to take: it is never used as an address, a kernel raises a flag
 *       (modes 0 and 2: the stamp; mode 1: the frames' opaque counts), and the call fails with -1 and a "patolette_amd_remap_rgba:"
 *       text in patolette_amd_last_error; what the outputs then hold is not defined.  The next call works.
 *   Outputs, each optional (NULL): palette_map, N elements of map_elem_bytes (1, 2, 4 or 8; able to hold palette_rows - 1: the
 *       elements are sized by palette_rows, transparent row included), frame after frame; quantized, N x 4 interleaved.  With both
 *       NULL the call still checks the arguments and the flag.
 *   Exit codes: 0; -2 an empty image or frames == 0; -4 more than 2^31 pixels in all in mode 1 (more than 40000^2 otherwise); -1 (with
 *       a "patolette_amd_remap_rgba:" text) for a mode other than 0, 1, 2, an alpha_threshold outside [0, 256], a transparent_index
 *       other than -1 and 0, both or neither palette, no palette row, a bad map_elem_bytes, no pixels, no usable or a non-finite
 *       palette row, no opaque row left, a spread that is negative or not finite in mode 2, or the flag above.  A failed call leaves
 *       the thread's engine usable.
 *   Statistics: the ms_* fields as for a remap; the dither counters summed over the frames in mode 1, else 0.
 *       patolette_amd_last_map_palette: the opaque rows in the map's space.
 * Modes 0 and 2 run the mappers of the RGB remaps unchanged over every pixel; one more kernel for all frames (k_rgba_stamp) reads the
 * alpha byte and the mapper's element and writes the final element and the RGBA word.  Mode 1 goes frame after frame through the
 * RGBA entry's compaction, masked walk and expansion; every frame's opaque count reaches the host with one wait.
 * The *_device flavour takes device pointers for pixels / palette_map / quantized (palette_map and quantized aligned to their element
 * size, as hipMalloc returns them; pixels that are not 4-byte aligned are copied once); both palettes stay host memory. */
void patolette_amd_remap_rgba_u8(size_t frames, size_t width, size_t height, const unsigned char *pixels, int alpha_threshold,
                                 const double *palette, const unsigned char *palette_u8, size_t palette_rows, int transparent_index,
                                 int mode, double spread, void *palette_map, int map_elem_bytes, unsigned char *quantized,
                                 int *exit_code);
void patolette_amd_remap_rgba_u8_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int alpha_threshold,
                                        const double *palette, const unsigned char *palette_u8, size_t palette_rows,
                                        int transparent_index, int mode, double spread, void *d_palette_map, int map_elem_bytes,
                                        unsigned char *d_quantized, int *exit_code);
/* TESTS ONLY: k_rgba_stamp gives a lane four consecutive pixels (16-byte accesses) wherever the stack has at least four pixels and every
 * buffer is aligned for its vector access, otherwise one.  0 takes one everywhere, 1 and -1 restore that rule.  Same results either
 * way.  Process-wide; returns the previous mode. */
int patolette_amd_debug_rgba_stamp_quad(int mode);

/* ---- ColorHistogram: one palette for pixels that arrive in chunks ------------------------------
 * Every palette-making entry above takes all its pixels in one array.  Here an exact histogram of the colours is kept in HBM, filled
 * over as many calls as the caller likes (the frames of a clip a few at a time, the images of a directory), and the palette is made
 * from it at the end.  8-bit input has at most 2^24 distinct colours, so the table has a fixed size, and the quantisers already take
 * per-colour weights.
 *   The table.  The caller owns it as device memory: patolette_amd_malloc(patolette_amd_hist_bytes(weighted)) bytes -- a 64-byte
 *       header plus 2^24 64-bit counts (128 MB), plus 2^24 64-bit unit sums in a weighted table (256 MB) -- made usable by
 *       patolette_amd_hist_clear and passed to every call with the same `weighted` (0 or 1) it was cleared with; a call on memory
 *       that is not a cleared table of that mode fails with -1.  No handle, no registry; one table is used by one thread at a time.
 *   Key.  A pixel's key is R << 16 | G << 8 | B.  A fourth channel does not enter the key.
 *   Skipping by alpha.  With 4-channel pixels and an alpha_threshold in [0, 255], a pixel with alpha < alpha_threshold enters nothing
 *       (opaque means alpha >= threshold, as for patolette_amd_rgba).  alpha_threshold -1: every pixel enters.
 *   Unweighted (weighted == 0).  Per key a 64-bit count of pixels.
 *   Weighted (weighted == 1, fixed when the table is cleared).  Per key also a second 64-bit integer: the sum of the pixels' weights
 *       in units of 2^-32.  Each weight is converted on its own as rint(w * 2^32) -- the scaling is exact, ties go to even -- and then
 *       integers are added.  A weight must be finite and satisfy 0 <= w <= 2^20 (the saliency weights derived here, 1 + sal^2 *
 *       width * height / tile_size^2 with sal in [0, 1], stay far below that for any usual tile size; one beyond it is refused like
 *       a given one).
 *   Exact and order-free.  Both tables hold exact integers: the result of any sequence of adds and merges does not depend on order,
 *       chunking, grid shape or timing.  A clip added whole, frame by frame, row by row or backwards gives the same bits.
 *   Overflow.  Counts cannot overflow.  A weight sum that would pass 2^64 units is detected wherever partial sums are formed and
 *       does not pass silently: the call fails with -1 and a text "<entry>: overflow: ...", the table is marked, and every later call
 *       on it except patolette_amd_hist_clear fails the same way (what the table holds is then not defined).
 *   A refused add leaves the table exactly as it was: bad arguments, a weight out of range or not finite (validated and converted
 *       in a pass of their own before anything is accumulated), a saliency failure (-5, -6, -7; the weights of all frames of the
 *       call are derived first).  Only overflow marks the table.
 *
 * patolette_amd_hist_add_u8: pixels as patolette_amd_frames_u8 takes them (`frames` images of width x height, `channels` 3 or 4).
 *   A weighted table needs `weights` (frames * width * height values in frame order), or tile_size > 0: every frame then gets the
 *   saliency weights patolette_amd_frames_u8 derives for it as an image of its own.  An unweighted table refuses both.  The *_device
 *   flavour takes device pointers for pixels (any alignment) and weights: nothing crosses PCIe.
 * patolette_amd_hist_merge: d_hist += d_other, bin by bin; both of the mode `weighted`; overflow as above (d_hist is marked).
 * patolette_amd_hist_totals: *pixels = the sum of the counts, *colors = the number of keys with count > 0.
 * patolette_amd_hist_export: every key with count > 0, ascending by key, into host buffers of `capacity` rows (at least *colors of
 *   patolette_amd_hist_totals, else -1): colors (M,3) bytes, counts (M) uint64, weights (M) f64 -- equal to the count in an
 *   unweighted table, units / 2^32 in a weighted one, rounded once.  Each may be NULL.
 * patolette_amd_hist_palette: take the exported colours whose weight is > 0; M' of them.  M' == 0: -1.  M' <= palette_size: the
 *   palette is those colours themselves in key order -- palette_u8 their bytes, palette bytes / 255.0, unused rows -1 resp. 0 as
 *   patolette_amd_u8 fills them; no quantiser runs.  M' > palette_size: bit for bit what patolette_amd_u8 returns as palette and
 *   palette_u8 for those M' colours as a 1 x M' image (width M', height 1) with those weights, tile_size 0, `options` with dither
 *   and palette_only off, and neither map nor quantized image wanted (the same internal path, fed from HBM).  palette:
 *   (palette_size,3) column-major f64; palette_u8: palette_size x 3; host memory, each may be NULL.
 * Exit codes: 0; -2 frames == 0 or an empty image; -3 palette_size == 0; -4 more than 40000^2 pixels in one add; -5, -6, -7 from the
 *   saliency stage; -1 with a text in patolette_amd_last_error that begins with the entry's name ("patolette_amd_hist_add:" for both
 *   flavours of the add): no table or pixels, bad channels, an alpha_threshold outside [-1, 255] or one with 3 channels, the weights
 *   rule above, a bad weight, memory that is not a cleared table of this mode, a capacity that is too small, no colour for a
 *   palette, or "... overflow: ...".  The int-returning entries return these codes.  A failed call leaves the thread's engine usable.
 * Statistics (patolette_amd_last_stats): the ms_* fields as for a remap -- ms_upload the pixels and weights of a host add, ms_saliency
 *   the derived weights, ms_map the kernels and their flags (export and palette: the compaction), ms_download the rows on their way
 *   out -- every other field 0.  A palette that runs the quantiser (M' > palette_size) leaves that call's statistics instead, as
 *   patolette_amd_u8_device leaves them, without the compaction ahead of it.
 * Kernels (hist.hip): k_hist_units (weights -> units and their check), k_hist_add (64-bit integer atomics, relaxed, agent scope,
 *   behind a merge of equal keys in registers and in an LDS table), k_hist_merge, k_hist_totals; the export is compact.h over the bins. */
size_t patolette_amd_hist_bytes(int weighted);
int patolette_amd_hist_clear(void *d_hist, int weighted);
void patolette_amd_hist_add_u8(void *d_hist, int weighted, size_t frames, size_t width, size_t height, const unsigned char *pixels,
                               int channels, int alpha_threshold, const double *weights, double tile_size, int *exit_code);
void patolette_amd_hist_add_u8_device(void *d_hist, int weighted, size_t frames, size_t width, size_t height, const unsigned char *d_pixels,
                                      int channels, int alpha_threshold, const double *d_weights, double tile_size, int *exit_code);
int patolette_amd_hist_merge(void *d_hist, const void *d_other, int weighted);
void patolette_amd_hist_totals(const void *d_hist, int weighted, uint64_t *pixels, uint64_t *colors, int *exit_code);
void patolette_amd_hist_export(const void *d_hist, int weighted, size_t capacity, unsigned char *colors, uint64_t *counts, double *weights,
                               int *exit_code);
void patolette_amd_hist_palette(const void *d_hist, int weighted, size_t palette_size, const patolette__QuantizationOptions *options,
                                double *palette, unsigned char *palette_u8, int *exit_code);

/* ---- batch of independent images (SURVEY.md 8(b) "Batch extension") -----------------------
 * count images of identical width x height; data[i] / weights[i] (weights may be NULL or hold
 * NULL entries) / tile_size / palettes[i] / palette_maps[i] / exit_codes[i] as for
 * patolette_amd_quantize(); up to six images are in flight on the current GPU (fewer if the free HBM does not hold their workspaces).  Results are
 * identical to count separate calls. */
void patolette_amd_batch(size_t count, size_t width, size_t height, const double *const *data,
                         const double *const *weights, double tile_size, size_t palette_size,
                         const patolette__QuantizationOptions *options, double *const *palettes,
                         size_t *const *palette_maps, int *exit_codes);

/* the same with every image as (width*height, 3) row-major f64 (see patolette_amd_quantize_rows) */
void patolette_amd_batch_rows(size_t count, size_t width, size_t height, const double *const *rows,
                              const double *const *weights, double tile_size, size_t palette_size,
                              const patolette__QuantizationOptions *options, double *const *palettes,
                              size_t *const *palette_maps, int *exit_codes);

/* the 8-bit entry for a batch: pixels[i] / palettes[i] / palettes_u8[i] / palette_maps[i] / quantized[i] as for
 * patolette_amd_u8() (palettes_u8, palette_maps, quantized or single entries of them may be NULL); 3 bytes per pixel cross
 * PCIe instead of 24, so a host-fed batch is no longer bound by the upload */
void patolette_amd_batch_u8(size_t count, size_t width, size_t height, const unsigned char *const *pixels, int channels,
                            const double *const *weights, double tile_size, size_t palette_size,
                            const patolette__QuantizationOptions *options, double *const *palettes,
                            unsigned char *const *palettes_u8, void *const *palette_maps, int map_elem_bytes,
                            unsigned char *const *quantized, int *exit_codes);

/* Host images in, index maps LEFT IN HBM: the entry behind patolette_amd.dist: each rank quantises its
 * shard of the batch and the maps go to rank 0 over RCCL straight from device memory -- no widening to size_t, no PCIe
 * round trip.  images[i]: pixel_format 0 = planar f64 as patolette() takes it, 1 = (N,3) row-major f64, 3 / 4 = interleaved
 * 8-bit sRGB with that many bytes per pixel.  d_palette_maps (device, may be NULL): count consecutive maps of
 * width*height elements of map_elem_bytes (1 when palette_size <= 256, else 4).  Everything else as patolette_amd_batch(). */
void patolette_amd_batch_dmap(size_t count, size_t width, size_t height, const void *const *images, int pixel_format,
                              const double *const *weights, double tile_size, size_t palette_size,
                              const patolette__QuantizationOptions *options, double *const *palettes, void *d_palette_maps,
                              int map_elem_bytes, int *exit_codes);

/* ---- ONE image over several GPUs (SURVEY.md 8(f)-4, 8(e) last row) ------------------------
 * The reference has no distributed code; this is the path's own sharding.  Every GPU of a group holds a contiguous slice
 * of the image's pixels (image order: slice r+1 follows slice r) and runs the whole path on it; the only data that crosses
 * GPUs are the per-node reductions of patolette.c's stages -- colour bounds and column sums (matrix2D.c:229), projection
 * extrema (sort.c:43-59), 512-bucket moment tables (cells.c:82-112, local.c:118-134), the children's centred moments
 * (cluster.c:111-152) -- and the KMeans subsample (refine.c:127-163, 262 144 x 12 bytes by default).  Those reductions are
 * integers, ordered-key minima / maxima, or sums of addends on fixed grids (DESIGN.md 4.1 "order-independent sums"): exact in
 * any grouping, so every GPU takes the same decisions and the result does not depend on how the pixels are dealt out --
 * the palette is identical on every GPU and bit-identical to what one GPU computes for the whole image with
 * patolette_amd_set_invariant_sums(1); each GPU's index map is its slice of that image's map.
 *
 * The library does not link a communication library: the caller lends it ONE collective, an in-place element-wise SUM over
 * the group (RCCL all-reduce through torch.distributed in patolette_amd.dist; any MPI / RCCL binding will do).  dtype: 0 =
 * f64, 1 = i64, 2 = i32.  `buffer` is device memory unless host_buffers is set (then the library stages through pinned
 * host memory -- for CPU-side transports such as gloo).  The call returns when the reduced values are in `buffer`; non-zero =
 * failure (exit code -1).  Minima, maxima and exclusive prefixes over the ranks are taken from a SUM over a table with one
 * row per rank.  Every rank must make the same call (same palette_size, options, total_pixels). */
typedef int (*patolette_amd_allreduce_sum_fn)(void *ctx, void *buffer, size_t count, int dtype);
typedef struct patolette_amd__Comm {
    int rank, size;
    patolette_amd_allreduce_sum_fn allreduce_sum;
    void *ctx;
    int host_buffers;
} patolette_amd__Comm;
/* slice_data: planar f64 (x | y | z, plane stride slice_pixels) of pixels [slice_begin, slice_begin + slice_pixels) of an
 * image of total_pixels pixels, host memory; slice_weights: NULL or slice_pixels doubles (all ranks alike); palette:
 * palette_size x 3 column-major, the same on every rank; slice_map: slice_pixels entries (NULL with palette_only).
 * Not available per slice: dithering (one curve over the whole image: exit code -1) and derived saliency weights
 * (pass explicit weights).  Exit codes as patolette(); every slice must hold at least one pixel. */
void patolette_amd_slice(size_t total_pixels, size_t slice_begin, size_t slice_pixels, const double *slice_data,
                         const double *slice_weights, size_t palette_size, const patolette__QuantizationOptions *options,
                         const patolette_amd__Comm *comm, double *palette, size_t *slice_map, int *exit_code);
/* the same with the slice (and its weights) resident in HBM and the slice's index map left there (elements of
 * map_elem_bytes: 1 when palette_size <= 256, else 4), as patolette_amd_device() */
void patolette_amd_slice_device(size_t total_pixels, size_t slice_begin, size_t slice_pixels, const double *d_slice_data,
                                const double *d_slice_weights, size_t palette_size, const patolette__QuantizationOptions *options,
                                const patolette_amd__Comm *comm, double *palette, void *d_slice_map, int map_elem_bytes,
                                int *exit_code);
/* 1: the children's moments of every split are summed product by product on the exact grids (tiling-invariant, what the
 * sliced path always does; 190 instead of 157 us per 4096^2 level in the partition kernel, +7 % on the whole step); 0 (default): per-thread partial sums first.  Applies to
 * the calling thread's later calls.  Returns the previous setting. */
int patolette_amd_set_invariant_sums(int on);
/* The centroid update of the KMeans refinement.  0 (default): the reference's, bit for bit -- every centroid is the sequential f32
 * sum of its samples in sample order (faiss Clustering.cpp:135-204), which costs a stable sort of the samples and one dependent
 * chain per centroid in every iteration.  1: order-free -- the sums are taken exactly (64-bit fixed point) and rounded to f32
 * once: deterministic, independent of how the samples spread over the centroids, 4.4x faster per KMeans stage at 67 M samples,
 * but NOT the reference's bits: per iteration the centroids differ by what its f32 chains round away (~1e-6 of the colour range),
 * and a sample on the border of two cells that therefore changes sides moves a centroid of m members by |x - c| / m (1e-4 at the
 * default 1024 members, 1e-6 at 65 536), which over the 32 iterations of the default spreads to most rows: the palette then agrees
 * with the reference's to ~1e-4 of the colour range, not to BASELINE's 1e-5, and ~0.02 % of the index map follows
 * (tests/test_gpu_kmeans_update.py prints the measured figures).  Process-wide; applies to later calls.  Returns
 * the previous setting.  Environment default: PAMD_KMEANS_UPDATE=1. */
int patolette_amd_set_kmeans_update(int mode);

/* Who drives the split loop of the local quantiser (quantize/local.c:318-404).  The device-driven loop enqueues round after round
 * without a host turn: the children's moments, bounds and eigen-solves and the next round's node list are made by two small
 * kernels, the sweep kernels read their sizes from device memory, which candidate nodes to evaluate is decided by a rule that
 * provably never skips a node the greedy loop commits, and the greedy loop of local.c:347-390 is replayed once, on the host, over
 * the evaluated tree; the host synchronises once per image instead of once per round.  Taken for palettes of up to 256 colours
 * on one GPU.  mode 2 (default): for images below 40 Mi pixels (40 x 2^20), where it is at least as fast; 1: wherever it
 * applies; 0: the host-driven loop everywhere (what sliced images, larger palettes and verbose calls always take).  Same
 * decisions and results either way (the children's moments may differ in their last bit: DESIGN.md 4.2).  Process-wide; returns
 * the previous setting.  Environment: PAMD_LQ_DEVICE=0|1|2. */
int patolette_amd_set_split_loop(int mode);
/* Where the decisions of the global quantiser are taken (lib/src/quantize/global.c:189-298: prefix sums of the 512-bucket table,
 * the bias termination test, the dynamic programme's backtrack, the bucket -> base cluster table, the base clusters' records):
 * 1 (default) on the device, in one kernel between the histogram and the partition (no host turn; palettes of more than 12
 * colours on one GPU, not verbose), 0 on the host.  Same arithmetic either way: same cuts, same clusters.  Returns the
 * previous setting. */
int patolette_amd_set_global_quantiser(int on_device);

/* The KMeans subsample list (faiss rand_perm(N, seed 1234), Clustering.cpp:311-319: a pure function of the pixel count) is made
 * on a helper thread that starts at call entry and is joined when the KMeans stage begins.  1 (default): the list stays on the
 * device between calls on images of one size; 0: every call makes it again -- the cost of a FIRST call of a size, call after
 * call (bench.py reports both).  The same switch governs the other size-only table kept between calls: the Riemersma dither's
 * curve order (rank along the Hilbert curve -> pixel number, 4 bytes per pixel, a function of width and height alone).
 * Process-wide.  Returns the previous setting. */
int patolette_amd_set_subsample_cache(int on);

/* ---- single stages, host buffers in / out (for parity tests) ------------------------------ */
/* The KMeans subsample the refinement draws (faiss Clustering.cpp:311-319: the first `take` entries of rand_perm(n, seed 1234),
 * utils/random.cpp:184-194) as the product's host code makes it (host only: needs no device).  0 = ok. */
int patolette_amd_subsample_indices(size_t n, size_t take, int32_t *out);
/* patolette__EIGEN_solve (math/eigen.c:83-140: LAPACK dsyev 'V','L', n = 3) as the split loop's host side solves it:
 * a column-major 3x3 (lower triangle read) -> w ascending, z = eigenvectors as columns; returns LAPACK's info (0 = ok).
 * patolette_amd_principal_axis: covariance as (xx,xy,xz,yy,yz,zz) -> eigenvector of the largest eigenvalue incl. its
 * sign (math/pca.c:122-149 takes column 2); 0 ok.  Pure host code (no device needed). */
int patolette_amd_eigen_sym3(const double a_colmajor[9], double w[3], double z[9]);
int patolette_amd_principal_axis(const double cov6[6], double axis[3]);
/* the same solver as the DEVICE runs it inside the split loop's control kernel (one problem per lane): `count` column-major 3x3
 * matrices in, w (3 per problem), z (9 per problem) and LAPACK's info out; host buffers.  Returns 0, or -1 on a HIP error. */
int patolette_amd_eigen_sym3_device(const double *a_colmajor, size_t count, double *w, double *z, int *info);
/* The global quantiser (global.c:189-377) from a 512-bucket moment table the caller gives, for tests: what it decides, on the
 * route asked for, from the production code itself on scratch buffers.
 *   table        host, the engine's own layout: quantity q, part p, bucket b at (q * 2 + p) * 512 + b; quantities 0..2 sum c,
 *                3 sum |c|^2, 4..9 sum c_r c_s ((r,s) = 00,01,11,02,12,22); when weighted also 10..12 sum w c, 13 sum w
 *   counts       512 pixel counts
 *   palette_size passed straight through (quantize() takes the device route above 12 only; here either route runs at any size)
 *   route        0 the host's turn (the DP kernels, then the host's decisions), 1 the control kernel
 * Out: *kbase base clusters (0 when *error, the eigen-solver's failure), cuts[14] (q_0 = 0 .. q_kbase = 512), bucket_table[512]
 * (bucket -> base cluster), per base cluster begin[12], n[12], sw[12], mean[12][3].  Optional (NULL to skip):
 *   prefix_w0[2][513], prefix[14][513]   the inclusive prefixes, 1-based, as the termination test reads them: row 0 of prefix_w0,
 *                rows 0..9 of prefix (w1[0..2], w2, the six wrs).  Route 0 adds the DP kernels' own chains: row 1 of prefix_w0,
 *                rows 10..13 (w1[0..2], w2); route 1 leaves those zero
 *   cut_table[13][513]   the DP's L[k][n] as the route left it
 * Returns 0, or -1 on bad arguments or a HIP error. */
int patolette_amd_debug_gq_table(const double *table, const uint32_t *counts, int weighted, size_t palette_size, int route, int *kbase, int *error,
                                 int *cuts, unsigned char *bucket_table, uint64_t *begin, uint64_t *n, double *sw, double *mean,
                                 uint64_t *prefix_w0, double *prefix, int *cut_table);
/* out[i] = pow(x[i], y) as the colour conversions evaluate it on the device (x >= 0; <= 0.52 ulp) */
int patolette_amd_pow(const double *x, double y, double *out, size_t n);
/* Tests only: the same with the routine named.  mode 0: the general routine (any x); 1: the branch-free routine of the common domain
 * (x positive, normal and finite, -1200 <= y log2(x) <= 1100: the caller's promise, nothing checks it); 2: what patolette_amd_pow
 * runs -- a vote per wavefront picks 1 when every lane's x allows it and 0 otherwise.  All three return the same bits wherever 1
 * is allowed.  Returns 0, or -1 on an unknown mode or a HIP error. */
int patolette_amd_debug_pow(const double *x, double y, double *out, size_t n, int mode);

enum {
    PAMD_SRGB_TO_ICTCP = 0,     /* patolette__COLOR_sRGB_Matrix_to_ICtCp_Matrix            color/ICtCp.c:120-146 */
    PAMD_SRGB_TO_CIELUV = 1,    /* patolette__COLOR_sRGB_Matrix_to_CIELuv_Matrix           color/CIELuv.c:166-197 */
    PAMD_ICTCP_TO_REC2020 = 2,  /* patolette__COLOR_ICtCp_Matrix_to_Linear_Rec2020_Matrix  color/rec2020.c:128-148 */
    PAMD_CIELUV_TO_REC2020 = 3, /* patolette__COLOR_CIELuv_Matrix_to_Linear_Rec2020_Matrix color/rec2020.c:150-173 */
    PAMD_SRGB_TO_REC2020 = 4,   /* patolette__COLOR_sRGB_Matrix_to_Linear_Rec2020_Matrix   color/rec2020.c:175-195 */
    PAMD_REC2020_TO_SRGB = 5,   /* patolette__COLOR_Linear_Rec2020_Matrix_to_sRGB_Matrix   color/sRGB.c:112-132 */
    PAMD_CIELUV_TO_ICTCP = 6    /* the Luv->Rec2020->sRGB->ICtCp chain of patolette.c:305-314, fused per pixel */
};
/* in place on a planar (n,3) host matrix */
int patolette_amd_convert(int which, double *planar, size_t n);
/* Tests only: one conversion (the ids above, or 100 for the plain copy) of n pixels from a planar (n,3) f64 host matrix or from
 * interleaved 8-bit rows with `channels` (3 or 4) bytes per pixel (exactly one of planar / bytes is non-NULL; bytes / 255 are read
 * as coordinates of the source space whatever it is) into the planar (n,3) host matrix out.  general != 0: every pow through the
 * general routine, whatever the wavefront's vote would say.  Returns 0, or -1 on bad arguments or a HIP error. */
int patolette_amd_debug_convert(int which, const double *planar, const unsigned char *bytes, int channels, double *out, size_t n, int general);

/* patolette__GQ_quantize + patolette__LQ_quantize + patolette__PALETTE_create
 * (quantize/global.c:388-443, quantize/local.c:318-404, palette/create.c:11-33).
 * colors planar (n,3) already in the quantisation space; centers planar (K,3) out (first
 * *n_clusters rows valid, palette order).  Returns 0 or -1. */
int patolette_amd_quantize_clusters(const double *colors, const double *weights, size_t n, size_t K,
                                    double *centers, size_t *n_clusters);

/* patolette__PALETTE_get_refined_palette (palette/refine.c:165-221 -> patched faiss
 * kmeans_clustering).  centers_io planar (k,3) f64.
 *
 * Two DEPARTURES, both where the reference does not return or is undefined; in each the centres come back as they went in
 * (rounded to f32), as they do for n < k and for a NaN / Inf among the colours:
 *
 * 1. Empty clusters without a donor.  split_clusters (Clustering.cpp:216-263) gives an empty cluster half of a donor cj that it
 *    accepts when a draw r in [0, 1) is below (h[cj] - 1) / (n - k), and walks round the clusters until one is accepted.  When
 *    no cluster has a size h > 1 (weighted input whose cluster weight sums are <= 1, or NaN) no candidate can ever be accepted
 *    and the reference spins.  Here, once no cluster with h > 1 is left, the remaining empty clusters of that iteration keep
 *    what the update wrote (centre 0, size 0) and the iterations go on.  An acceptance probability that is small but positive
 *    is the reference's behaviour and stays.  The same walk cannot end when n - k wraps: k > max(max_samples, 65536) makes
 *    the subsample k * (max_samples / k) = 0 samples long.  KMeans is skipped when subsampling leaves fewer than k + 1 samples;
 *    that includes a subsample of exactly k samples (max_samples / 2 < k <= max_samples, n > k), where the reference does
 *    return -- with the first k samples of the image as centres, which refines nothing.
 *
 * 2. The finite domain.  With |x| > ~1.8e19 the f32 norm |x|^2 is +inf, every candidate distance is NaN and the reference's
 *    nearest-centre index is -1, with which it indexes its arrays; the same follows once all centres are NaN, after a sum
 *    overflowed or 1 / h met a subnormal h.  KMeans is skipped unless every f32 intermediate of an iteration is finite by
 *    these bounds, taken from the f32 inputs:  B = max(1, largest |colour value|, largest |initial centre value|), both finite;
 *    m = min(samples used, 2^25);  weights (if any) finite, >= 0 and the smallest positive one, wmin, a normal f32 (>= 2^-126);
 *    Cb bounds every centre of every iteration: 8 B + 8 without weights; with them 4 min(exp(n / 2^23), 4 m wmax / wmin) B + 8
 *    for n samples used (wmax = max(1, largest weight): the first from the rounding of the two chains a centre is the quotient
 *    of, the second from h >= wmin);  required:  16 Cb^2 <= FLT_MAX  and  4 m wmax B <= FLT_MAX.  Without weights that is
 *    B <= 5.7e17; with them, for values up to 255, any weights up to 2.7e8 samples (exp(n / 2^23) B <= 1.1e18), beyond that a
 *    weight ratio of 3.4e7 -- the bound is a proven one, not a sharp one; an image beyond it is not
 *    refined.  Weights without a positive one put no condition on wmin.  The full paths (patolette_amd,
 *    patolette_amd_device, the batch and slice entries) apply the same rule: the pass that takes the largest weight also takes
 *    the smallest positive one and notes a negative or non-finite one, over all GPUs of a sliced image. */
int patolette_amd_kmeans_refine(const double *colors, const double *weights, size_t n,
                                double *centers_io, size_t k, int niter, size_t max_samples);
/* TESTS ONLY: what the last KMeans of the calling thread's engine ran, as a bit mask; 0 = it did not iterate (skipped, n == k, or
 * niter 0).  1 list path (block-local sorts, one block per centroid collects its members) | 2 full scan | 4 the form beyond 4096
 * centroids (counters and cursors in memory) | 8 pruned by the 32^3 table | 16 by the 64^3 table | 32 the 64^3 table read through
 * the four-candidate table in LDS (one byte per assignment) | second half of the stable sort: 64 from int assignments, 128 from
 * bytes, 256 from bytes with paired records, 512 through LDS in batches of 4096 | 1024 the block-parallel chain is on for clusters
 * of PAMD_KM_LONG_MIN (8192) members | 2048 the order-free sums (patolette_amd_set_kmeans_update(1)): no sort, no chain. */
int patolette_amd_debug_km_route(void);

/* patolette__PALETTE_fill_palette_map_nearest (palette/nearest.c:150-209) */
int patolette_amd_nn_map(const double *colors, size_t n, const double *palette, size_t k, size_t *map);
/* TESTS ONLY: which kernels the nearest map takes is decided by the pixel count -- brute force below 16 384 pixels, a 32^3 candidate
 * table from there, a 64^3 table from 2^22 (with up to 256 palette rows: read through a four-candidate table in LDS).  route 1, 2, 3
 * make every nearest map (this stage, the full paths, remap) take the route of the first, second, third size class whatever its
 * size; 0 restores the default.  The limits on the palette stay: outside 8 .. 4096 rows every route is brute force, above 256 rows
 * route 3 reads the 64^3 table directly; and the remap's byte-source kernel (2^22 pixels and more by default) runs under route 3 at
 * any size and never under routes 1 and 2.  Same map for every setting.  Process-wide; returns the previous setting. */
int patolette_amd_debug_nn_route(int route);
/* TESTS ONLY: patolette_amd_nn_map with map elements of map_elem_bytes = 1 (k <= 256; what every image of up to 256 colours takes), 4
 * or 8 bytes in the host buffer `map` (n elements).  misalign = 1 (1-byte elements only) starts the device's output one byte into
 * its allocation: the odd address that image i of a batch with an odd pixel count gets.  0, or -1 (patolette_amd_last_error). */
int patolette_amd_debug_nn_map_elem(const double *colors, size_t n, const double *palette, size_t k, int map_elem_bytes, int misalign,
                                    void *map);

/* patolette__DITHER_riemersma (dither/riemersma.c:437-459); colors/palette in linear Rec2020.  Any double is taken for a PIXEL: one
 * whose distances are all NaN or +Inf (a NaN, an infinite or a huge value in a plane) gets index 0, as do the pixels behind it
 * while its error -- or a sum of errors that overflows -- is in the queue, and the chain goes on from there: the reference's
 * behaviour, under both layouts.  The PALETTE is taken to be finite and below 2^1000 in magnitude: with a larger entry the error
 * sums of the wavefront layout may overflow where no pixel announced it, and the map then differs from the reference's to the end of
 * that run. */
int patolette_amd_dither(const double *colors, size_t width, size_t height, const double *palette,
                         size_t k, size_t *map);

/* Test / tuning knob of the segment-parallel dither (process-wide): `segments` runs (0 = chosen from the image size, 1 = the
 * single serial chain) and `warm` in-image pixels of speculative warm-up per run (< 0 = default; 0 forces every boundary to be
 * repaired).  The map is the reference's chain bit for bit for every setting. */
void patolette_amd_dither_config(int segments, int warm);
/* ... and which layout walks the runs (process-wide, 8 <= palette rows <= 256): -1 (default) = one LANE per run for images of
 * 2^23 pixels and more, one WAVEFRONT per run below; 1 = lanes from 65 536 pixels on; 0 = wavefronts everywhere.  Same map. */
void patolette_amd_dither_layout(int lanes);
/* TESTS ONLY: after `cap` passes taken by one wavefront alone the lane layout gives the image up and the wavefront layout starts
 * over (default 4096, never reached in practice; 0 forces that fall-back at the first stall); < 0 restores the default.  Returns
 * the previous value. */
int patolette_amd_debug_dither_solo_cap(int cap);
/* TESTS ONLY: verification passes without progress (fewer than an eighth of the failing boundaries fixed) after which ONE wavefront
 * walks alone from the lowest failing boundary (default 2; 0 = every repair pass is such a walk); < 0 restores the default.
 * Returns the previous value.  The map is the reference's chain for every setting. */
int patolette_amd_debug_dither_stall_passes(int n);
/* which layout a dither of this image size and palette takes under the current knobs: 1 = one lane per run, 0 = one wavefront per run */
int patolette_amd_dither_layout_in_use(size_t width, size_t height, size_t palette_rows);
/* Where the dither cuts the curve (host-side copy of the kernel's function, runs without a GPU): *d = first curve position of the
 * aligned 64-position block that holds in-image pixel number t (curve order, 0-based), *c = in-image pixels before that block. */
void patolette_amd_debug_dither_locate(size_t width, size_t height, unsigned long long t, unsigned long long *d, unsigned long long *c);
/* TESTS ONLY: what the lane layout's search read in the calling thread's last dither, copied to the host.  geom30: for each of the
 * three grids (over the weighted palette's box +- 1/2 extent, +- 1 1/2 extents, +- 4 extents) ten doubles {lo[3], hi[3], inv[3], G};
 * amb3: the margins of the f32 first pass {amb, amb_p, amb_x}; tables (NULL: geometry only): the 16-byte records, G^3 first records
 * {count, entries 0..14} then G^3 second records {entries 15..29, one byte unused} for each grid in turn, 32 (G0^3 + G1^3 + G2^3) bytes, `capacity`
 * the room there.  0; -1 where that dither did not take the lane layout (or a nearest map has used the workspace since) or the room
 * is too small.  No kernel and no product path reads what this entry keeps. */
int patolette_amd_debug_dither_lane_tables(double *geom30, float *amb3, unsigned char *tables, size_t capacity);

/* ---- statistics of the last full-path call on this thread -------------------------------- */
typedef struct patolette_amd__Stats {
    double ms_total, ms_upload, ms_convert, ms_gq, ms_lq, ms_kmeans, ms_map, ms_download, ms_saliency;
    size_t n_base_clusters;   /* clusters produced by the global quantiser */
    size_t n_clusters;        /* final palette rows */
    size_t split_evals;       /* split_cluster evaluations performed on the GPU */
    size_t split_px;          /* sum of their sizes: D_eff = split_px / (width*height) */
    size_t lq_rounds;         /* host<->device round trips of the split loop */
    size_t kmeans_samples;    /* samples clustered per KMeans iteration */
    size_t dither_segments;   /* runs the Hilbert curve was cut into (walked side by side, one lane or one wavefront each) */
    size_t dither_repairs;    /* runs walked again because their speculative starting state was not the chain's */
    size_t dither_rounds;     /* boundary-verification passes (the last one found nothing to repair) */
    size_t dither_through;    /* stalled verifications (a long flat stretch off the palette) resolved by walking one run through its successors */
    size_t dither_jumps;      /* lane layout: periodic jumps -- a walk over pixels of ONE colour found its period and wrote the pattern to the stretch's end */
    size_t dither_solo;       /* lane layout: passes taken by one wavefront alone after two passes without progress */
} patolette_amd__Stats;
void patolette_amd_last_stats(patolette_amd__Stats *out);
/* The palette exactly as the mapping stage of the last full-path call on this thread used it: linear Rec2020 when dithering
 * (patolette.c:268-299), ICtCp for the nearest-neighbour map (:300-324), before the conversion back to sRGB.  Written
 * column-major with `capacity_rows` rows when they suffice; returns the number of palette rows.  Lets a parity test feed
 * the oracle's dither / NN map the very inputs the device stage saw. */
size_t patolette_amd_last_map_palette(double *out, size_t capacity_rows);

/* ---- what the quantisers of the last call on this thread decided (full path or patolette_amd_quantize_clusters) -----------
 * The global quantiser's axis, covariance and cuts (quantize/global.c:388-443) and, per committed split of the greedy loop
 * (quantize/local.c:347-390) in commit order: which row of `result` was split (`best`, :348-352), where (the bucket of
 * get_optimal_bucket_index, :102-177), along which axis (cluster.c:191-217, with the very matrix the eigen-solver was handed),
 * into how many members, and the distortions behind the benefit (:256-275).  On content whose decisions are ties in exact
 * arithmetic (perfect gradients, a handful of colours) the reference's own choice hinges on the rounding of its sequential
 * sums; tests/tie_prover.py takes this trace and the pixels and checks, in exact integer arithmetic, that every decision
 * recorded here lies within that rounding envelope of the exact optimum.  The CPU oracle exports the same records. */
typedef struct patolette_amd__SplitRecord {
    int32_t row, new_row;     /* row split; row that received the LEFT child (= clusters before the commit, local.c:375-376) */
    int32_t split;            /* bucket index of the cut */
    int32_t degenerate;       /* the projection took sort.c:61-79's round-robin rule */
    uint64_t n, n_left, n_right;
    double sw;                /* sum of the cluster's weights */
    double axis[3];
    double cov6[6];           /* xx, yx, zx, yy, zy, zz as handed to the eigen-solver (pca.c:62-101) */
    double dist, dist_left, dist_right, benefit;
} patolette_amd__SplitRecord;
typedef struct patolette_amd__SplitTrace {
    int32_t n_base, n_clusters, n_records, stopped_early;   /* stopped_early: best benefit < 1e-16 (local.c:365-370) */
    double gq_axis[3];
    uint64_t gq_cuts[14];     /* n_base + 1 entries (global.c:290) */
    double gq_cov6[6];        /* the unweighted covariance of all pixels as handed to the eigen-solver (global.c:407) */
} patolette_amd__SplitTrace;
/* returns the number of records; copies min(capacity, that) of them */
size_t patolette_amd_last_split_trace(patolette_amd__SplitTrace *hdr, patolette_amd__SplitRecord *recs, size_t capacity);
/* PALETTE_create's rows of the last call (palette/create.c:11-33: the clusters' weighted centres in the quantisation space,
 * before any KMeans), column-major with `capacity_rows` rows when they suffice; returns the number of rows */
size_t patolette_amd_last_cluster_centers(double *out, size_t capacity_rows);

/* TESTS ONLY: make the quantisers take a deliberately WRONG decision, to show that tests/tie_prover.py tells a tie from a bug.
 * 0 = none (default); 1 = the cut one occupied bucket past the arg-max of local.c:171; 2 = the greedy step takes the second
 * best cluster (local.c:277-307); 3 = the cut at the LAST maximum of the objective instead of the first (a member of the tie
 * set: differs from the reference only where the objective is exactly tied); 4 = NOT a wrong decision: the device-driven split
 * loop reports its node table full after three rounds, so the call starts over on the host-driven loop (what a candidate tree
 * too large for the table does; the result must not change).  Process-wide; returns the previous setting. */
int patolette_amd_debug_fault(int which);

/* TESTS ONLY: make the workspace's history visible.  A result must not depend on what the engine's buffers held before (another
 * image's state, another engine's freed memory).  Bit 0 (poison): every fresh allocation of f64 / f32 device memory, and of f64
 * pinned host memory, starts as quiet NaN, and so do the floating-point fields of the node table and of the split loop's control
 * state; integer memory (indices, counts, keys) is never touched, so a stray read cannot become an address.  A NaN that reaches a
 * result turns a silent dependence on memory contents into a visible mismatch.  Bit 1: count the workspace growths that free or
 * move an allocation while the calling engine's streams still hold queued work (patolette_amd_debug_late_growths).  A count above
 * zero is a definite hazard; a zero count is only evidence, since queued work may finish before the check.  Bit 2: name each such
 * growth on stderr.  Process-wide; applies to later allocations; returns the previous flags.  Off: one relaxed atomic load per
 * growth.  Environment default: PAMD_DEBUG_WORKSPACE=<flags>, read once when the library loads. */
int patolette_amd_debug_workspace(int flags);
/* late growths counted since the library loaded (bit 1 of patolette_amd_debug_workspace) */
unsigned long long patolette_amd_debug_late_growths(void);

/* ---- per-kernel timing with HIP events on the launch stream ------------------------------
 * The timer is the calling thread's own: these calls switch, select and read the timing of launches made on this thread only. */
void patolette_amd_profile_enable(int on);   /* also resets the accumulated numbers */
/* restrict the timing to the kernel of this name (NULL or "" = every kernel): two event records per launch
 * cost ~7 us, so a throughput measurement times only the kernel it reports the roofline of */
void patolette_amd_profile_only(const char *kernel_name);
/* with a kernel selected by patolette_amd_profile_only: put events on every `period`-th of its launches only (1 = all) */
void patolette_amd_profile_sample(int period);
/* number of distinct kernels seen; entry i: name (<= 63 chars), accumulated ms, launch count and the
 * ALGORITHMIC HBM bytes of those launches (per-unit figures in DESIGN.md) */
int  patolette_amd_profile_count(void);
int  patolette_amd_profile_get(int i, char *name64, double *total_ms, size_t *launches, double *total_bytes);

#ifdef __cplusplus
}
#endif
#endif
