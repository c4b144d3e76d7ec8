// lzw.h -- launcher of the GIF LZW kernels (lzw.hip) and the layout of what passes between them.
#pragma once

#include "common.h"

namespace pamd {

// pixels of a segment when the caller passes 0 (include/patolette_amd.h); the most a caller may ask for
constexpr size_t kLzwSegment = 8192, kLzwSegmentMax = (size_t)1 << 24;
// slots of a wavefront's dictionary in LDS: 32 bits each, 20 of key (prefix code << 8 | byte) above 12 of code, 0 = empty (no entered
// code is below 6).  At most 4090 codes are ever entered, so a probe always meets an empty slot; 32 KB, five blocks on a CU's 160 KB.
constexpr unsigned kLzwSlots = 8192;

// a frame's rectangle as the kernels take it, and the number of its first segment; the table has frames + 1 records, the last one's
// seg0 being the number of segments in all
struct LzwFrame { unsigned x0, y0, w, area, seg0; };

// codes a frame of `area` symbols in `nseg` segments emits at the most -- one per symbol, a closing code per segment, a Clear per
// full dictionary (at least 3838 codes apart), the opening Clear -- as include/patolette_amd.h states it, and its bytes at 12 bits
inline size_t lzw_frame_bound(size_t area, size_t nseg) { return (12 * (area + 2 * nseg + area / 3000 + 2) + 7) / 8; }
// 32-bit words of a segment's staging area: 12 bits for each of its at most len symbol codes, len / 3000 Clears, the closing code and
// the opening Clear, and one word more, so that the word after any bit of it can be read
inline size_t lzw_stage_words(size_t len) { return (12 * (len + len / 3000 + 3) + 31) / 32 + 2; }

// d_words: [0] the flag (low bit: an element inside a rectangle was not below 2^m), then offsets[frames + 1] in bytes.
// launch_lzw zeroes word 0; the host reads all of them.
inline size_t lzw_words(size_t frames) { return frames + 2; }

// The LZW of include/patolette_amd.h (patolette_amd_gif_lzw): d_maps frames x n one-byte elements, n = width * height; d_frames the
// frames + 1 records above (S = their last seg0 segments in all); seg_len the segment's pixels, m the minimum code size.
// d_stage: S * lzw_stage_words(min(seg_len, largest area)) words; d_bits: S; d_gbit: S + 1; d_words: lzw_words(frames);
// d_out: out_words 32-bit words, at least the sum of the frames' bounds.  Three launches: k_lzw_segments, k_lzw_offsets, k_lzw_pack.
void launch_lzw(const unsigned char *d_maps, size_t frames, size_t n, size_t width, const LzwFrame *d_frames, size_t S, size_t seg_len,
                size_t stride, int m, unsigned *d_stage, unsigned *d_bits, unsigned long long *d_gbit, unsigned long long *d_words,
                unsigned *d_out, size_t out_words, hipStream_t s);

// What follows a segments kernel, the deflate coder's too (deflate.hip): k_lzw_offsets and k_lzw_pack over S segments whose bit strings
// lie LSB first at d_stage + s * stride with d_bits[s] bits each -- the frames' offsets into d_words[1 ..], the streams into d_out.
// pack_blocks: ceil(out_words / 256).
void lzw_offsets_and_pack(size_t frames, const LzwFrame *d_frames, size_t S, size_t stride, const unsigned *d_stage, const unsigned *d_bits,
                          unsigned long long *d_gbit, unsigned long long *d_words, unsigned *d_out, size_t out_words, size_t pack_blocks,
                          hipStream_t s);

// bytes of the lossy coder's table: 256 rows of 16 -- the count, then up to 15 candidates in order of preference
constexpr size_t kLzwNearBytes = 4096;

// The lossy LZW of include/patolette_amd.h (patolette_amd_gif_lzw_lossy): launch_lzw with k_lzw_lossy_segments in the place of
// k_lzw_segments.  d_near: the table, of which the rows below 2^m are read (the host has checked their counts and candidates);
// 16-byte aligned.  d_coded: null, or frames x n bytes that do not overlap d_maps: the symbol each step coded, inside the rectangles.
void launch_lzw_lossy(const unsigned char *d_maps, size_t frames, size_t n, size_t width, const LzwFrame *d_frames, size_t S, size_t seg_len,
                      size_t stride, int m, const unsigned char *d_near, unsigned char *d_coded, unsigned *d_stage, unsigned *d_bits,
                      unsigned long long *d_gbit, unsigned long long *d_words, unsigned *d_out, size_t out_words, hipStream_t s);

}  // namespace pamd
