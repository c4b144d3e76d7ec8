// measure.h -- launcher of the measure kernels (measure.hip) and the layout of what they leave.
#pragma once

#include "common.h"

namespace pamd {

// cells a block of k_measure accumulates in LDS, and the most palette rows it holds there: per cell a 64-bit sse, a 32-bit count and a
// 32-bit maximum, per row its three bytes packed in a word (20 KB), with the ICtCp part also three planar f64 arrays (24 KB) next to
// the 4 KB of pow tables and the 2 KB companding table: 50 KB.  A shorter palette's rows get several cells each (measure_copies_log2);
// a longer palette is indexed and accumulated in global memory.
constexpr int kMeasureChunk = 1024;
// same-address atomics serialise in L2: the blocks' per-entry cells are spread over up to this many slots, which k_measure_fold sums
constexpr unsigned kMeasureSlots = 32;
// positions of a tile while a frame has at most 2^22 of them; beyond that the tile doubles until a frame has at most kMeasureTiles
constexpr size_t kMeasureTile = 2048, kMeasureTiles = 2048;

// THE PARTITION: a function of the frame's positions and the palette's rows, of nothing else
inline size_t measure_tile(size_t n) { size_t t = kMeasureTile; while (ceil_div(n, t) > kMeasureTiles) t *= 2; return t; }
inline size_t measure_tiles_per_frame(size_t n) { return ceil_div(n, measure_tile(n)); }
// log2 of the copies of a row's LDS cell (1, 2, 4 or 8: what fits the chunk); a lane accumulates into copy lane % copies
inline unsigned measure_copies_log2(size_t rows) { unsigned s = 0; while (s < 3 && (rows << (s + 1)) <= (size_t)kMeasureChunk) s++; return s; }
inline unsigned measure_slots(size_t rows) { unsigned s = kMeasureSlots; while (s > 1 && rows * s > ((size_t)1 << 21)) s >>= 1; return s; }

// what a tile leaves with plain stores: its part of the frame's integers, and of the two ICtCp figures (0 without them)
struct MeasureTile { unsigned long long sse; unsigned count, max_se; double d_sum, d_max; };

// d_words, as unsigned long long words, S = measure_slots(rows):
//   [0, S*rows)            per slot and row the sse
//   [S*rows, 2*S*rows)     per slot and row two unsigned ints: count, max_se
//   [2*S*rows]             low bit: some element was neither the skip index nor below `rows`
//   then 3 words per row   count, sse, max_se            (k_measure_fold)
//   then 5 words per frame count, sse, max_se, d_sum and d_max as the doubles' bits
// launch_measure zeroes the words up to and including the flag; the host reads from the flag on.
inline size_t measure_flag_word(size_t rows) { return 2 * (size_t)measure_slots(rows) * rows; }
inline size_t measure_words(size_t frames, size_t rows) { return measure_flag_word(rows) + 1 + 3 * rows + 5 * frames; }
inline size_t measure_tile_count(size_t frames, size_t n) { return frames * measure_tiles_per_frame(n); }

// The measure of include/patolette_amd.h (patolette_amd_measure): `frames` index maps of n positions with elements of 1 or 4 bytes
// against their frames' interleaved 8-bit pixels.  rows: the palette's used rows (an element must be below it, or equal `skip` while
// skip_on); d_p8: per row its three bytes packed as r | g << 8 | b << 16; d_pal: the rows in ICtCp, planar (rows,3), or null -- then
// no pixel is converted and the tiles' d_sum / d_max are 0.  d_words: measure_words(frames, rows); d_tiles: measure_tile_count.
// k_measure is one launch for all frames; k_measure_fold sums the slots and folds every frame's tiles in a fixed order.
void launch_measure(const void *d_maps, int elem_bytes, size_t frames, size_t n, const unsigned char *d_px, int channels, size_t rows,
                    bool skip_on, unsigned skip, const unsigned *d_p8, const double *d_pal, unsigned long long *d_words,
                    MeasureTile *d_tiles, hipStream_t s);

}  // namespace pamd
