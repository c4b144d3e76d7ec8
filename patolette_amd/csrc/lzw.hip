// lzw.hip -- the GIF flavour of LZW on gfx950: include/patolette_amd.h, patolette_amd_gif_lzw.
//
// LZW is one serial chain per stream, and a GIF decoder forgets its dictionary at every Clear code: a frame's symbols are cut into
// segments that are compressed on their own, every one ending in a Clear (the last in the end code), and the segments' bit strings
// are then put end to end.  Three kernels, integers only, no atomic but the flag's OR (the lossy coder, patolette_amd_gif_lzw_lossy,
// puts k_lzw_lossy_segments in the first one's place):
// k_lzw_segments: a wavefront (a block of 64) per segment.  The lanes fetch 64 symbols with one load (a rectangle's rows are runs of
//   consecutive bytes) while the chain runs over the 64 before them; the chain itself is wave-uniform -- prefix, key, hash, the slot
//   read back through readfirstlane, the bit accumulator and every branch live in scalar registers.  The dictionary is an open
//   addressing table in LDS (lzw.h).  Codes gather in a 64-bit accumulator; each full 32-bit word goes to lane (word number % 64) of
//   one register, and every 64 words leave with one plain store into the segment's own staging area.  The segment's bit length
//   goes into a table.
// k_lzw_offsets: one block.  Per frame the sum of its segments' bits, rounded up to bytes (frames start on a byte); an exclusive
//   scan of those over the frames -- the offsets the caller gets --; then per frame an exclusive scan of the segments' bits from
//   the frame's first bit: every segment's first bit in the output.
// k_lzw_pack: a thread per 32-bit output word: a binary search for the segment its first bit lies in (or behind), then every
//   segment that reaches into the word is shifted into place from its staging area.
#include "lzw.h"

namespace pamd {

__global__ __launch_bounds__(64) void k_lzw_segments(const unsigned char *__restrict__ maps, size_t n, unsigned width,
                                                     const LzwFrame *__restrict__ fr, unsigned frames, unsigned seg_len, unsigned m,
                                                     size_t stride, unsigned *__restrict__ stage, unsigned *__restrict__ seg_bits,
                                                     unsigned *flag) {
    __shared__ unsigned s_tab[kLzwSlots];
    const unsigned lane = threadIdx.x, sg = blockIdx.x;
    // the frame: the last record whose first segment is not beyond this one
    unsigned lo = 0, hi = frames;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (fr[mid].seg0 <= sg) lo = mid; else hi = mid;
    }
    const LzwFrame F = fr[lo];
    const unsigned k = sg - F.seg0, q0 = k * seg_len;                   // (q0 < area <= 1.6e9)
    const unsigned len = min(seg_len, F.area - q0);
    const bool last = q0 + len == F.area;
    const unsigned char *frame = maps + (size_t)lo * n + (size_t)F.y0 * width + F.x0;
    const unsigned clear = 1u << m, eoi = clear + 1u;
    unsigned *out = stage + (size_t)sg * stride;

    bool bad = false;
    // symbols base + lane of the segment (0 beyond its end); an element that is no symbol raises `bad` and is never a key
    auto fetch = [&](unsigned base) -> unsigned {
        const unsigned i = base + lane;
        if (base >= len || i >= len) return 0u;
        const unsigned q = q0 + i, y = q / F.w, x = q - y * F.w;
        unsigned v = frame[(size_t)y * width + x];
        if (v >= clear) { bad = true; v = 0; }
        return v;
    };
    auto wipe = [&]() {
        for (unsigned j = lane; j < kLzwSlots; j += 64) s_tab[j] = 0;
        __syncthreads();
    };

    unsigned long long acc = 0;
    unsigned nbits = 0, wpos = 0, held = 0;                             // held: this lane's word of the 64 being gathered
    auto push = [&]() {                                                 // the accumulator's low word
        if (lane == (wpos & 63u)) held = (unsigned)acc;
        wpos++;
        if ((wpos & 63u) == 0) out[wpos - 64 + lane] = held;
    };
    auto emit = [&](unsigned code, unsigned w) {
        acc |= (unsigned long long)code << nbits;
        nbits += w;
        if (nbits >= 32) {
            push();
            acc >>= 32;
            nbits -= 32;
        }
    };

    unsigned cur = fetch(0);
    wipe();
    unsigned free_code = eoi + 1u, cw = m + 1u;
    if (k == 0) emit(clear, cw);
    unsigned prefix = (unsigned)__builtin_amdgcn_readlane((int)cur, 0);
    unsigned first = 1;
    for (unsigned base = 0; base < len; base += 64) {
        const unsigned nxt = fetch(base + 64);                          // in flight while the chain runs over `cur`
        const unsigned cnt = min(64u, len - base);
        for (unsigned i = first; i < cnt; i++) {
            const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)cur, (int)i);
            const unsigned key = prefix << 8 | c;
            unsigned h = (key * 2654435761u) >> 19;                     // 13 bits
            unsigned found = 0;
            for (unsigned probe = 0; probe < kLzwSlots; probe++) {      // (bounded by the table: no input can spin)
                const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tab[h]);
                if (e == 0) break;
                if ((e >> 12) == key) { found = e & 4095u; break; }
                h = (h + 1u) & (kLzwSlots - 1u);
            }
            if (found) { prefix = found; continue; }
            emit(prefix, cw);
            if (free_code < 4096u) {
                s_tab[h] = key << 12 | free_code;
                if (free_code == (1u << cw) && cw < 12u) cw++;
                free_code++;
            } else {
                emit(clear, cw);
                wipe();
                free_code = eoi + 1u; cw = m + 1u;
            }
            prefix = c;
        }
        first = 0;
        cur = nxt;
    }
    emit(prefix, cw);
    if (free_code < 4096u && free_code == (1u << cw) && cw < 12u) cw++;   // the decoder makes an entry on that code too
    emit(last ? eoi : clear, cw);
    const unsigned bits = wpos * 32u + nbits;
    if (nbits > 0) push();
    if (lane < (wpos & 63u)) out[(wpos & ~63u) + lane] = held;
    if (lane == 0) seg_bits[sg] = bits;
    if (__ballot(bad) && lane == 0) atomicOr(flag, 1u);
}

// The lossy coder (include/patolette_amd.h, patolette_amd_gif_lzw_lossy): k_lzw_segments with another step.  When the pair (prefix,
// symbol) is not in the dictionary, the symbol's candidates -- its row of `near`, 16 bytes: the count, then up to 15 symbols in order
// of preference -- are tried in its place, and the first that is continues the match.  Lane j < 16 probes for candidate j (lane 0 for
// the symbol itself), all in the same step: every lane probes from its own slot in one uniform loop that runs while any lane is still
// probing (a lane's state moves by selects), a 64-bit ballot of the hits picks the lowest lane, and its code and candidate come
// back by readlane.  No hit: lane 0 stands on the empty slot of the exact pair, and the old miss runs
// wave-uniformly with the TRUE symbol.
// The rows travel with the symbols: the lane that fetches symbol i of a batch loads that symbol's row (one 16-byte load of a 4 KB
// table, a batch ahead of its use), and step i takes the four words by readlane; lane j picks byte j.  No table in LDS.
// The dictionary's write of a step is a store of one value by all 64 lanes in uniform control flow (nothing in the step diverges:
// the ballots, like every cross-lane builtin, stand in uniform code): each lane that reads the slot in a later step has written it
// itself, in program order.  wipe() ends in a barrier as before.
// coded (or null): the symbol each step coded, at the place its symbol came from.  A lane keeps its own symbol and takes the
// substitute when step i == lane replaced it; a batch leaves with one store.
__global__ __launch_bounds__(64) void k_lzw_lossy_segments(const unsigned char *__restrict__ maps, size_t n, unsigned width,
                                                           const LzwFrame *__restrict__ fr, unsigned frames, unsigned seg_len, unsigned m,
                                                           const uint4 *__restrict__ near, unsigned char *__restrict__ coded, size_t stride,
                                                           unsigned *__restrict__ stage, unsigned *__restrict__ seg_bits, unsigned *flag) {
    __shared__ unsigned s_tab[kLzwSlots];
    const unsigned lane = threadIdx.x, sg = blockIdx.x;
    unsigned lo = 0, hi = frames;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (fr[mid].seg0 <= sg) lo = mid; else hi = mid;
    }
    const LzwFrame F = fr[lo];
    const unsigned k = sg - F.seg0, q0 = k * seg_len;
    const unsigned len = min(seg_len, F.area - q0);
    const bool last = q0 + len == F.area;
    const size_t origin = (size_t)lo * n + (size_t)F.y0 * width + F.x0;
    const unsigned char *frame = maps + origin;
    const unsigned clear = 1u << m, eoi = clear + 1u;
    unsigned *out = stage + (size_t)sg * stride;

    bool bad = false;
    // symbol base + lane of the segment with its row and its place in the frame (all 0 beyond the segment's end)
    struct Batch { unsigned sym, at; uint4 row; };
    auto fetch = [&](unsigned base) -> Batch {
        Batch b{0u, 0u, make_uint4(0u, 0u, 0u, 0u)};
        const unsigned i = base + lane;
        if (base >= len || i >= len) return b;
        const unsigned q = q0 + i, y = q / F.w, x = q - y * F.w;
        b.at = y * width + x;                                           // (< n <= 1.6e9)
        unsigned v = frame[b.at];
        if (v >= clear) { bad = true; v = 0; }
        b.sym = v;
        b.row = near[v];                                                // (v < 2^m: a row the host has checked)
        return b;
    };
    auto wipe = [&]() {
        for (unsigned j = lane; j < kLzwSlots; j += 64) s_tab[j] = 0;
        __syncthreads();
    };

    unsigned long long acc = 0;
    unsigned nbits = 0, wpos = 0, held = 0;
    auto push = [&]() {
        if (lane == (wpos & 63u)) held = (unsigned)acc;
        wpos++;
        if ((wpos & 63u) == 0) out[wpos - 64 + lane] = held;
    };
    auto emit = [&](unsigned code, unsigned w) {
        acc |= (unsigned long long)code << nbits;
        nbits += w;
        if (nbits >= 32) {
            push();
            acc >>= 32;
            nbits -= 32;
        }
    };

    // where candidate `lane` lies in a row: which of the four words (its mask is all ones, the others' 0; no word beyond lane 15) and
    // the byte's shift -- a select without a branch
    const unsigned shift_of = (lane & 3u) * 8u;
    const unsigned in0 = (lane >> 2) == 0 ? ~0u : 0u, in1 = (lane >> 2) == 1 ? ~0u : 0u, in2 = (lane >> 2) == 2 ? ~0u : 0u, in3 = (lane >> 2) == 3 ? ~0u : 0u;
    Batch cur = fetch(0);
    wipe();
    unsigned free_code = eoi + 1u, cw = m + 1u;
    if (k == 0) emit(clear, cw);
    unsigned prefix = (unsigned)__builtin_amdgcn_readlane((int)cur.sym, 0);
    unsigned first = 1;
    for (unsigned base = 0; base < len; base += 64) {
        const Batch nxt = fetch(base + 64);                             // in flight while the chain runs over `cur`
        const unsigned cnt = min(64u, len - base);
        unsigned mine = cur.sym;                                        // what the step of this lane's symbol codes
        for (unsigned i = first; i < cnt; i++) {
            const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)cur.sym, (int)i);
            const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)cur.row.x, (int)i);
            const unsigned r1 = (unsigned)__builtin_amdgcn_readlane((int)cur.row.y, (int)i);
            const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)cur.row.z, (int)i);
            const unsigned r3 = (unsigned)__builtin_amdgcn_readlane((int)cur.row.w, (int)i);
            const unsigned count = r0 & 255u;                           // (<= 15: the host has checked it)
            const unsigned rw = (r0 & in0) | (r1 & in1) | (r2 & in2) | (r3 & in3);
            const unsigned cand = lane == 0 ? c : (rw >> shift_of) & 255u;
            const unsigned key = prefix << 8 | cand;
            // The probes of all candidates at once: the loop is uniform and runs while any lane is still probing; a lane's state moves
            // by selects, not by branches.  A lane that takes no part reads slot `lane` (its own bank) and nothing comes of it.
            bool live = lane <= count && lane < 16u;
            unsigned h = live ? (key * 2654435761u) >> 19 : lane;       // 13 bits
            unsigned found = 0;
            for (unsigned probe = 0; probe < kLzwSlots && __ballot(live) != 0; probe++) {   // (bounded by the table: no input can spin)
                const unsigned e = s_tab[h];
                const bool hit = live && e != 0 && (e >> 12) == key;
                found = hit ? e & 4095u : found;
                live = live && e != 0 && !hit;                          // an empty slot ends a lane's probe where it stands
                h = live ? (h + 1u) & (kLzwSlots - 1u) : h;
            }
            const unsigned long long hits = __ballot(found != 0);
            if (hits) {
                const int win = __builtin_ctzll(hits);                  // the symbol itself first, then the row's order
                prefix = (unsigned)__builtin_amdgcn_readlane((int)found, win);
                if (win != 0) {
                    const unsigned sub = (unsigned)__builtin_amdgcn_readlane((int)cand, win);
                    if (lane == i) mine = sub;
                }
                continue;
            }
            const unsigned slot = (unsigned)__builtin_amdgcn_readlane((int)h, 0);   // the empty slot of the exact pair
            emit(prefix, cw);
            if (free_code < 4096u) {
                s_tab[slot] = (prefix << 8 | c) << 12 | free_code;
                if (free_code == (1u << cw) && cw < 12u) cw++;
                free_code++;
            } else {
                emit(clear, cw);
                wipe();
                free_code = eoi + 1u; cw = m + 1u;
            }
            prefix = c;
        }
        if (coded && lane < cnt) coded[origin + cur.at] = (unsigned char)mine;
        first = 0;
        cur = nxt;
    }
    emit(prefix, cw);
    if (free_code < 4096u && free_code == (1u << cw) && cw < 12u) cw++;   // the decoder makes an entry on that code too
    emit(last ? eoi : clear, cw);
    const unsigned bits = wpos * 32u + nbits;
    if (nbits > 0) push();
    if (lane < (wpos & 63u)) out[(wpos & ~63u) + lane] = held;
    if (lane == 0) seg_bits[sg] = bits;
    if (__ballot(bad) && lane == 0) atomicOr(flag, 1u);
}

__device__ inline unsigned long long wave_inclusive_scan(unsigned long long v, unsigned lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(v, o);
        if (lane >= (unsigned)o) v += up;
    }
    return v;
}

// One block of 1024 (sixteen wavefronts), frames in chunks of 1024.  A wavefront takes frames w, w + 16, ... of the chunk.
__global__ __launch_bounds__(1024) void k_lzw_offsets(const LzwFrame *__restrict__ fr, unsigned frames, const unsigned *__restrict__ seg_bits,
                                                      unsigned long long *__restrict__ gbit, unsigned long long *__restrict__ words) {
    __shared__ unsigned long long s_val[1024], s_wave[16], s_carry;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid == 0) s_carry = 0;
    for (unsigned c0 = 0; c0 < frames; c0 += 1024) {
        const unsigned cn = min(1024u, frames - c0);
        __syncthreads();
        for (unsigned i = wv; i < cn; i += 16) {                        // a frame's bytes
            const unsigned s0 = fr[c0 + i].seg0, s1 = fr[c0 + i + 1].seg0;
            unsigned long long b = 0;
            for (unsigned s = s0 + lane; s < s1; s += 64) b += seg_bits[s];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o);
            if (lane == 0) s_val[i] = (b + 7) >> 3;
        }
        __syncthreads();
        const unsigned long long v = tid < cn ? s_val[tid] : 0;         // the frames' first bytes: an exclusive scan
        const unsigned long long inc = wave_inclusive_scan(v, lane);
        if (lane == 63) s_wave[wv] = inc;
        __syncthreads();
        unsigned long long before = s_carry;
        for (unsigned j = 0; j < wv; j++) before += s_wave[j];
        const unsigned long long excl = before + inc - v;
        __syncthreads();
        if (tid < cn) { s_val[tid] = excl; words[1 + c0 + tid] = excl; }
        if (tid == 1023) s_carry = excl + v;
        __syncthreads();
        for (unsigned i = wv; i < cn; i += 16) {                        // every segment's first bit in the output
            const unsigned s0 = fr[c0 + i].seg0, s1 = fr[c0 + i + 1].seg0;
            unsigned long long run = s_val[i] * 8;
            for (unsigned sb = s0; sb < s1; sb += 64) {
                const unsigned s = sb + lane;
                const unsigned long long b = s < s1 ? seg_bits[s] : 0;
                const unsigned long long in = wave_inclusive_scan(b, lane);
                if (s < s1) gbit[s] = run + in - b;
                run += __shfl(in, 63);
            }
        }
    }
    __syncthreads();
    if (tid == 0) { words[1 + frames] = s_carry; gbit[fr[frames].seg0] = s_carry * 8; }
}

__global__ __launch_bounds__(256) void k_lzw_pack(const unsigned *__restrict__ stage, size_t stride, const unsigned *__restrict__ seg_bits,
                                                  const unsigned long long *__restrict__ gbit, unsigned S, unsigned *__restrict__ out,
                                                  size_t out_words) {
    const size_t W = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long B = (unsigned long long)W * 32;
    if (W >= out_words || B >= gbit[S]) return;
    unsigned lo = 0, hi = S;                                            // the last segment that starts at or before bit B
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (gbit[mid] <= B) lo = mid; else hi = mid;
    }
    unsigned word = 0;
    for (unsigned s = lo; s < S; s++) {
        const unsigned long long g = gbit[s];
        if (g >= B + 32) break;
        const unsigned long long a = g > B ? g : B, e = g + seg_bits[s] < B + 32 ? g + seg_bits[s] : B + 32;
        if (a >= e) continue;                                           // (the padding behind a frame's last segment)
        const unsigned p = (unsigned)(a - g), cnt = (unsigned)(e - a);
        const unsigned *st = stage + (size_t)s * stride + (p >> 5);     // (lzw_stage_words: the word behind any bit exists)
        const unsigned long long win = (unsigned long long)st[0] | (unsigned long long)st[1] << 32;
        unsigned v = (unsigned)(win >> (p & 31u));
        if (cnt < 32) v &= (1u << cnt) - 1u;
        word |= v << (unsigned)(a - B);
    }
    out[W] = word;
}

// What both coders check before their first launch, and the blocks of k_lzw_pack
static size_t lzw_launch_check(const void *d_maps, size_t frames, size_t width, const LzwFrame *d_frames, size_t S, size_t seg_len, int m,
                               unsigned *d_stage, unsigned *d_bits, unsigned long long *d_gbit, unsigned long long *d_words, unsigned *d_out,
                               size_t out_words) {
    if (!d_maps || !d_frames || !d_stage || !d_bits || !d_gbit || !d_words || !d_out) throw HipError("patolette_amd: gif_lzw needs maps and its workspace");
    if (m < 2 || m > 8 || seg_len < 1 || seg_len > kLzwSegmentMax) throw HipError("patolette_amd: gif_lzw: min_code_size or segment out of range");
    const size_t pack_blocks = ceil_div(out_words, 256);
    if (frames >> 31 || S >> 31 || pack_blocks >> 31 || width >> 32) throw HipError("patolette_amd: gif_lzw: a size does not fit the kernels' 32-bit fields");
    return pack_blocks;
}

// The segments' and frames' places, then the streams: what follows either coder's segments kernel, and the deflate coder's (lzw.h)
void lzw_offsets_and_pack(size_t frames, const LzwFrame *d_frames, size_t S, size_t stride, const unsigned *d_stage, const unsigned *d_bits,
                                 unsigned long long *d_gbit, unsigned long long *d_words, unsigned *d_out, size_t out_words, size_t pack_blocks,
                                 hipStream_t s) {
    {
        KTIME("k_lzw_offsets", s, 16.0 * S + 8.0 * frames);
        hipLaunchKernelGGL(k_lzw_offsets, 1, 1024, 0, s, d_frames, (unsigned)frames, d_bits, d_gbit, d_words);
        HIP_CHECK(hipGetLastError());
    }
    {
        KTIME("k_lzw_pack", s, 8.0 * out_words);
        hipLaunchKernelGGL(k_lzw_pack, (unsigned)pack_blocks, 256, 0, s, d_stage, stride, d_bits, d_gbit, (unsigned)S, d_out, out_words);
        HIP_CHECK(hipGetLastError());
    }
}

void launch_lzw(const unsigned char *d_maps, size_t frames, size_t n, size_t width, const LzwFrame *d_frames, size_t S, size_t seg_len,
                size_t stride, int m, unsigned *d_stage, unsigned *d_bits, unsigned long long *d_gbit, unsigned long long *d_words,
                unsigned *d_out, size_t out_words, hipStream_t s) {
    if (frames == 0 || S == 0) return;
    const size_t pack_blocks = lzw_launch_check(d_maps, frames, width, d_frames, S, seg_len, m, d_stage, d_bits, d_gbit, d_words, d_out, out_words);
    HIP_CHECK(hipMemsetAsync(d_words, 0, sizeof(unsigned long long), s));
    {
        KTIME("k_lzw_segments", s, 1.0 * frames * n);
        hipLaunchKernelGGL(k_lzw_segments, (unsigned)S, 64, 0, s, d_maps, n, (unsigned)width, d_frames, (unsigned)frames, (unsigned)seg_len, (unsigned)m,
                           stride, d_stage, d_bits, reinterpret_cast<unsigned *>(d_words));
        HIP_CHECK(hipGetLastError());
    }
    lzw_offsets_and_pack(frames, d_frames, S, stride, d_stage, d_bits, d_gbit, d_words, d_out, out_words, pack_blocks, s);
}

void launch_lzw_lossy(const unsigned char *d_maps, size_t frames, size_t n, size_t width, const LzwFrame *d_frames, size_t S, size_t seg_len,
                      size_t stride, int m, const unsigned char *d_near, unsigned char *d_coded, unsigned *d_stage, unsigned *d_bits,
                      unsigned long long *d_gbit, unsigned long long *d_words, unsigned *d_out, size_t out_words, hipStream_t s) {
    if (frames == 0 || S == 0) return;
    const size_t pack_blocks = lzw_launch_check(d_maps, frames, width, d_frames, S, seg_len, m, d_stage, d_bits, d_gbit, d_words, d_out, out_words);
    if (!d_near || ((uintptr_t)d_near & 15u)) throw HipError("patolette_amd: gif_lzw_lossy needs its table, 16-byte aligned");
    HIP_CHECK(hipMemsetAsync(d_words, 0, sizeof(unsigned long long), s));
    {
        KTIME("k_lzw_lossy_segments", s, (d_coded ? 2.0 : 1.0) * frames * n);
        hipLaunchKernelGGL(k_lzw_lossy_segments, (unsigned)S, 64, 0, s, d_maps, n, (unsigned)width, d_frames, (unsigned)frames, (unsigned)seg_len,
                           (unsigned)m, reinterpret_cast<const uint4 *>(d_near), d_coded, stride, d_stage, d_bits, reinterpret_cast<unsigned *>(d_words));
        HIP_CHECK(hipGetLastError());
    }
    lzw_offsets_and_pack(frames, d_frames, S, stride, d_stage, d_bits, d_gbit, d_words, d_out, out_words, pack_blocks, s);
}

}  // namespace pamd
