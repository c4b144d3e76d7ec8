// rgba.h -- launchers of the RGBA entry's kernels (rgba.hip).
#pragma once

#include "common.h"

namespace pamd {

// d_rgba: n interleaved RGBA pixels, 4-byte aligned.  Opaque = alpha >= thr.
// Count: d_counts (compact_tiles(n) entries) end as the tiles' offsets, *d_total as the number M of opaque pixels.
void launch_alpha_count(const unsigned char *d_rgba, size_t n, int thr, unsigned *d_counts, unsigned *d_total, hipStream_t s);
// Compaction (with the offsets of launch_alpha_count): d_cpos[i] = pixel i's number among the opaque pixels in row-scan order, or
// -1; d_rgb = their RGB, 3 bytes each; d_wc = their weights when d_w is given.
void launch_alpha_compact(const unsigned char *d_rgba, size_t n, size_t m, int thr, const unsigned *d_offsets, const double *d_w, int *d_cpos,
                          unsigned char *d_rgb, double *d_wc, hipStream_t s);
// Expansion: d_map[i] = off + d_cmap[d_cpos[i]] for an opaque pixel, 0 for a transparent one (d_cpos null: every pixel opaque, compact
// number = pixel number); d_quant[i] = the RGBA word of that palette entry.  cmap_elem 1 or 4; map_elem 1, 2, 4 or 8; either output
// may be null; d_quant and d_map aligned to their element size.
void launch_rgba_expand(const void *d_cmap, int cmap_elem, const int *d_cpos, size_t n, size_t m, unsigned off, const unsigned char *d_pal_rgba,
                        int k, void *d_map, int map_elem, unsigned char *d_quant, hipStream_t s);

// The stamp of the remap with alpha: d_cmap[i] = what a mapper chose for pixel i's RGB among the rows - off opaque rows (elements of
// cmap_elem = 1 or 4 bytes).  d_map[i] = off + d_cmap[i] and d_quant[i] = word d_map[i] of d_pal_rgba (rows RGBA words) where pixel i is
// opaque (alpha >= thr), 0 and (0, 0, 0, 0) where it is not.  A transparent pixel while off == 0 sets bit 0 of *d_flag, which the caller
// has cleared.  map_elem 1, 2, 4 or 8; either output, or both (then d_cmap is not read), may be null.  d_rgba 4-byte aligned, d_map and
// d_quant aligned to their element size; one launch for any n.
void launch_rgba_stamp(const unsigned char *d_rgba, const void *d_cmap, int cmap_elem, size_t n, int thr, unsigned off, const unsigned char *d_pal_rgba,
                       size_t rows, void *d_map, int map_elem, unsigned char *d_quant, unsigned *d_flag, hipStream_t s);
// tests: -1 four pixels per lane wherever the buffers are aligned for it (default), 0 never, 1 the same as -1; returns the previous mode
int rgba_stamp_debug_quad(int mode);

}  // namespace pamd
