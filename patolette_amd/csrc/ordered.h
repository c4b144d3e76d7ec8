// ordered.h -- launcher of the ordered-dither map kernel (ordered.hip).
#pragma once

#include "common.h"

namespace pamd {

// palette rows a block of k_ordered_map holds in LDS at a time, as three planar f64 arrays (24 KB next to the 4 KB of pow tables:
// five blocks of 256 threads fit a CU's 160 KB); a longer palette passes through in chunks of this many rows, ascending
constexpr int kOrderedChunk = 1024;

// The ordered (Bayer 8x8) map of include/patolette_amd.h (patolette_amd_remap_ordered_u8): `frames` images of width x height,
// interleaved 8-bit sRGB with `channels` (3 or 4) bytes per pixel; d_pal: the palette in ICtCp, planar (k,3); elements of 1 or 4
// bytes.  One kernel, no f64 image, no scratch.
void launch_ordered_map(const unsigned char *d_px, int channels, size_t frames, size_t width, size_t height, double spread, const double *d_pal,
                        int k, void *d_out, int elem_bytes, hipStream_t s);

}  // namespace pamd
