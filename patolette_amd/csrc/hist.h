// hist.h -- launchers of the colour-histogram kernels (hist.hip) and the layout of the table they keep.
#pragma once

#include "common.h"
#include "compact.h"

namespace pamd {

// THE TABLE (include/patolette_amd.h, "ColorHistogram"), as unsigned long long words in memory the caller owns:
//   [0]                          flags: bit 0 = a weight sum passed 2^64 units (the table is void until it is cleared)
//   [1]                          kHistMagic + (weighted ? 1 : 0): written by clear, so that a call can tell a cleared table of its mode
//   [2, kHistHeaderWords)        0
//   then kHistBins words         count of the pixels of key R << 16 | G << 8 | B
//   then, weighted only, kHistBins words: the sum of those pixels' weights in units of 2^-32
constexpr size_t kHistBins = (size_t)1 << 24;
constexpr size_t kHistHeaderWords = 8;
constexpr unsigned long long kHistMagic = 0x70616d6468697300ULL;           // "pamdhis\0"
constexpr double kHistUnit = 4294967296.0;                                 // units per 1.0 of weight: 2^32
constexpr double kHistMaxWeight = 1048576.0;                               // 2^20: a pixel carries at most 2^52 units
inline size_t hist_words(bool weighted) { return kHistHeaderWords + kHistBins * (weighted ? 2 : 1); }
inline unsigned long long *hist_counts(unsigned long long *h) { return h + kHistHeaderWords; }
inline const unsigned long long *hist_counts(const unsigned long long *h) { return h + kHistHeaderWords; }
inline unsigned long long *hist_units(unsigned long long *h) { return h + kHistHeaderWords + kHistBins; }
inline const unsigned long long *hist_units(const unsigned long long *h) { return h + kHistHeaderWords + kHistBins; }

// k_hist_add's partition: a lane takes kHistLanePixels consecutive pixels, a block of 256 lanes a tile, and kHistBlockTiles
// consecutive tiles before it flushes its LDS table.  Any partition gives the same table: the sums are integers.
constexpr int kHistLanePixels = 8;
constexpr size_t kHistTile = (size_t)256 * kHistLanePixels;
constexpr int kHistBlockTiles = 8;
constexpr int kHistSlotsLog2 = 11;                                         // the block's LDS table: 2048 (key, count, units) slots

// f64 weights -> units, each on its own as rint(w * 2^32); *d_flag (zeroed by the caller) gets bit 0 when a weight is not finite
// or outside [0, 2^20] (its unit is then written as 0).  Runs, and is checked by the host, before anything is accumulated.
void launch_hist_units(const double *d_weights, size_t N, unsigned long long *d_units, unsigned *d_flag, hipStream_t s);

// The add: N interleaved 8-bit pixels of `channels` (3 or 4) bytes at d_px (any alignment) into the table.  alpha_thr >= 0 (4 channels
// only): a pixel with alpha < alpha_thr enters nothing.  d_units: N units from launch_hist_units (a weighted table), or null.
// A weight sum that passes 2^64 -- in the block's LDS table or in the table itself; a lane's run is too short to -- sets bit 0 of word 0.
void launch_hist_add(unsigned long long *d_hist, bool weighted, const unsigned char *d_px, int channels, int alpha_thr, size_t N,
                     const unsigned long long *d_units, hipStream_t s);

// d_hist += d_other, bin by bin (both of the mode `weighted`); a unit sum that passes 2^64 sets bit 0 of d_hist's word 0
void launch_hist_merge(unsigned long long *d_hist, const unsigned long long *d_other, bool weighted, hipStream_t s);

// d_out[0] = the sum of the counts, d_out[1] = the number of bins with count > 0 (d_out: two words, zeroed here)
void launch_hist_totals(const unsigned long long *d_hist, unsigned long long *d_out, hipStream_t s);

// Export through compact.h over the bins, ascending by key.  keep: count > 0, and with `positive` also weight > 0 (the palette's
// list).  count: d_tiles (compact_tiles(kHistBins) entries) end as the tiles' offsets, *d_total as the number kept.  write: row r
// of the kept bins gets its key's three bytes at d_rgb + 3 r, its count at d_counts[r] (may be null) and its weight at d_w[r] --
// the count, or units / 2^32, converted to f64 once.
void launch_hist_export_count(const unsigned long long *d_hist, bool weighted, bool positive, unsigned *d_tiles, unsigned *d_total, hipStream_t s);
void launch_hist_export_write(const unsigned long long *d_hist, bool weighted, bool positive, const unsigned *d_tiles, unsigned char *d_rgb,
                              unsigned long long *d_counts, double *d_w, hipStream_t s);

}  // namespace pamd
