// deflate.h -- launcher of the PNG deflate kernels (deflate.hip) and the layout of what passes between them.
#pragma once

#include "common.h"
#include "deflate_codes.h"
#include "lzw.h"

namespace pamd {

// filtered bytes of a segment when the caller passes 0 (include/patolette_amd.h); the most a caller may ask for: the deflate window
constexpr size_t kDeflateSegment = 16384, kDeflateSegmentMax = dc::kWindow;
// slots of a wavefront's hash table in LDS: per 3-byte key the last position of the segment that had it, plus one (0 = none)
constexpr unsigned kDeflateHashSlots = 4096;

// bytes the workspace keeps readable on either side of the filtered streams
constexpr size_t kDeflateStreamPad = 32;

// a frame's filtered stream (PNG filter type 0 at depth 8): h rows of a zero byte and the rectangle's w indices
inline size_t deflate_filtered(size_t w, size_t h) { return h * (w + 1); }
// Bytes that hold a frame's stream of `flen` filtered bytes in `nseg` segments, as include/patolette_amd.h states it: every segment is
// one block of at most dc::block_bound_bits bits, the blocks lie bit to bit and the frame ends on a byte.
inline size_t deflate_frame_bound(size_t flen, size_t nseg) { return (9 * flen + 10 * nseg + 7) / 8; }
// 32-bit words of a segment's staging area, and one word more, so that the word after any bit of it can be read (k_lzw_pack)
inline size_t deflate_stage_words(size_t len) { return (size_t)((dc::block_bound_bits(len) + 31) / 32) + 2; }
// tokens a segment of len bytes has at the most: one a byte and the end of block
inline size_t deflate_token_stride(size_t len) { return len + 1; }

// d_words: [0] unused (zeroed), then offsets[frames + 1] in bytes, as k_lzw_offsets writes them (lzw.h); behind them two words per
// segment: the sum of its bytes and the sum of (len - i) * byte i, from which the host folds a frame's Adler-32.
inline size_t deflate_words(size_t frames, size_t S) { return frames + 2 + 2 * S; }
// A frame's Adler-32 from its segments' sums in order (zlib's adler32_combine, from the sums instead of from two checksums)
struct Adler32 {
    uint64_t a = 1, b = 0;
    void add(uint64_t sum, uint64_t weighted, uint64_t len) {
        b = (b + (len % 65521u) * a + weighted % 65521u) % 65521u;
        a = (a + sum % 65521u) % 65521u;
    }
    uint32_t value() const { return (uint32_t)(b << 16 | a); }
};

// The coder of include/patolette_amd.h (patolette_amd_png_deflate): d_maps frames x n one-byte elements, n = width * height; d_frames
// the frames + 1 records of lzw.h with `area` the FILTERED bytes h * (w + 1) (S = their last seg0 segments in all) and d_base[frames + 1]
// the frames' first bytes in d_stream, which takes d_base[frames] bytes; seg_len the segment's filtered bytes.
// d_stream is 16-byte aligned with kDeflateStreamPad readable bytes before it and after its d_base[frames] bytes: the exploration reads
// the window in aligned 16-byte pieces.
// d_tokens: S * tok_stride words; d_stage: S * stride words; d_bits: S; d_gbit: S + 1; d_words: deflate_words(frames, S);
// d_out: out_words 32-bit words, at least the sum of the frames' bounds.
// Four launches: k_png_filter, k_deflate_segments, k_lzw_offsets, k_lzw_pack.
void launch_deflate(const unsigned char *d_maps, size_t frames, size_t n, size_t width, const LzwFrame *d_frames, const unsigned long long *d_base,
                    size_t stream_bytes, size_t S, size_t seg_len, size_t tok_stride, size_t stride, unsigned char *d_stream, unsigned *d_tokens,
                    unsigned *d_stage, unsigned *d_bits, unsigned long long *d_gbit, unsigned long long *d_words, unsigned *d_out, size_t out_words,
                    hipStream_t s);

}  // namespace pamd
