// deflate.hip -- indexed PNG image data on gfx950: include/patolette_amd.h, patolette_amd_png_deflate.
//
// A frame's rectangle becomes PNG's scanline stream at depth 8 with filter type 0 -- every row a zero byte and its indices, the
// "filtered stream" -- and that stream one raw deflate stream (RFC 1951).  Deflate's dictionary is the decoded input itself, so the
// filtered stream is cut into segments that are parsed on their own, get their own code tables and still point back into the bytes
// before their start; the segments' blocks are put end to end bit by bit.  Four kernels, integers only; the only atomics are LDS
// integer adds (histograms), maxima (the hash table: the LAST position wins, whichever lane arrives first) and ORs (bits into words):
// k_png_filter: a thread per filtered byte: the streams of all frames, back to back, into the workspace.
// k_deflate_segments: a wavefront (a block of 64) per segment, in three parts.
//   Parse: 64 positions a step, a lane each.  A lane tries the image's own distances -- 1, 2, 4, 8, then the pixel above and its
//     neighbours (R - 1, R, R + 1 with R = w + 1 the row's bytes) and 2, 4, 8 rows up, the period of an 8 x 8 ordered dither -- and the
//     last earlier position of the segment with the same three bytes (a hash table in LDS, read before the step's own positions enter
//     it), and the up to four distances its explorations have found (below); every candidate within the frame and the 32 KB window
//     counts, also before the segment's start.  Each lane extends its
//     candidates four bytes at a time and keeps the longest (the first among equals in the order tried -- the order above, the
//     remembered distances and the hashed one last --, which is not the nearest: 8 comes before R - 1).  The serial part is a wave-uniform walk over
//     the 64 lengths: take the match at p unless the one at p + 1 is longer (one step of lazy evaluation), then jump.  It leaves two
//     64-bit masks (token starts, matches); the lanes at the starts then write their tokens side by side (a popcount gives the
//     place) and count them into the two histograms.
//   Tables: deflate_codes.h -- length-limited code lengths for literals/lengths and distances, their run-length coding, the
//     code-length code; the dynamic block's cost against the fixed block's, the cheaper wins (ties: fixed).
//   Emit: 64 tokens a step.  A lane looks up its token's bits (at most 48), a wave prefix scan of the bit counts gives every lane its
//     place, the bits are ORed into a small buffer in LDS, and the buffer's full words leave with one store into the segment's
//     staging area.  The header's fields and the coded lengths go the same way.
// k_lzw_offsets, k_lzw_pack (lzw.hip), as they are: the frames' offsets, every segment's first bit, and the bits shifted together.
#include "deflate.h"

namespace pamd {

__global__ __launch_bounds__(256) void k_png_filter(const unsigned char *__restrict__ maps, size_t n, unsigned width, const LzwFrame *__restrict__ fr,
                                                    const unsigned long long *__restrict__ base, unsigned frames, unsigned long long total,
                                                    unsigned char *__restrict__ stream) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    unsigned lo = 0, hi = frames;                                       // the last frame that starts at or before byte g
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (base[mid] <= g) lo = mid; else hi = mid;
    }
    const LzwFrame F = fr[lo];
    const unsigned q = (unsigned)(g - base[lo]), R = F.w + 1u, y = q / R, c = q - y * R;
    stream[g] = c == 0 ? (unsigned char)0 : maps[(size_t)lo * n + (size_t)(F.y0 + y) * width + F.x0 + (c - 1u)];
}

// bytes of a and b that agree from their start, at most maxlen (both readable over maxlen bytes)
__device__ inline unsigned match_length(const unsigned char *a, const unsigned char *b, unsigned maxlen) {
    unsigned k = 0;
    while (k + 4u <= maxlen) {
        unsigned va, vb;
        __builtin_memcpy(&va, a + k, 4);
        __builtin_memcpy(&vb, b + k, 4);
        const unsigned x = va ^ vb;
        if (x) return k + ((unsigned)__builtin_ctz(x) >> 3);
        k += 4u;
    }
    while (k < maxlen && a[k] == b[k]) k++;
    return k;
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The exploration: when a step has left more than kExploreTokens tokens, the next one first tries EVERY distance of the window at its
// first free position -- the window read in aligned 16-byte pieces, the four bytes at every place against the four here, then the
// length of those that agree and can beat the lane's best -- and a match of kExploreMin bytes and more puts its distance in front of the four
// remembered ones, which every lane then tries at every position.  An image repeats at few distances (a dither's tile, a row, a
// sprite's step), and the hash table, which keeps one position per key, cannot find the far ones.  An exploration that finds nothing
// makes the next ones wait 1, 3, 7, 15, then always 15 steps; one that finds something ends the waiting.
constexpr unsigned kExploreTokens = 2, kExploreMin = 8, kExplorePieces = 8;
constexpr unsigned kEmitWords = 104;                                    // 31 bits carried + 64 x 48, and the two words a lane's bits may reach into

__global__ __launch_bounds__(64) void k_deflate_segments(const unsigned char *__restrict__ stream, const unsigned long long *__restrict__ base,
                                                         const LzwFrame *__restrict__ fr, unsigned frames, unsigned seg_len, size_t tok_stride,
                                                         unsigned *__restrict__ tokens, size_t stride, unsigned *__restrict__ stage,
                                                         unsigned *__restrict__ seg_bits, unsigned long long *__restrict__ sums) {
    __shared__ unsigned s_hash[kDeflateHashSlots];
    __shared__ uint32_t s_lit_freq[dc::kLitTable], s_dist_freq[dc::kDistTable], s_cl_freq[dc::kClSyms + 1], s_cl_sent[dc::kClSyms + 1];
    __shared__ uint16_t s_lit_codes[dc::kLitTable], s_dist_codes[dc::kDistTable], s_cl_codes[dc::kClSyms + 1], s_rle[dc::kLitTable + dc::kDistTable];
    __shared__ uint8_t s_lit_lens[dc::kLitTable], s_dist_lens[dc::kDistTable], s_cl_lens[dc::kClSyms + 1];
    __shared__ dc::Work s_work;
    __shared__ unsigned s_buf[kEmitWords];
    __shared__ unsigned s_head[4];                                      // the coded lengths' count, HLIT, HDIST
    const unsigned lane = threadIdx.x, sg = blockIdx.x;
    unsigned lo = 0, hi = frames;                                       // the frame: the last record whose first segment is not beyond this one
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (fr[mid].seg0 <= sg) lo = mid; else hi = mid;
    }
    const LzwFrame F = fr[lo];
    const unsigned q0 = (sg - F.seg0) * seg_len;                        // (q0 < area < 2^32)
    const unsigned len = min(seg_len, F.area - q0);
    const bool last = q0 + len == F.area;
    const unsigned char *seg = stream + base[lo] + q0;                  // bytes [-q0, len) of it lie in the frame's stream
    unsigned *tok = tokens + (size_t)sg * tok_stride;
    unsigned *out = stage + (size_t)sg * stride;
    const unsigned R = F.w + 1u;
    auto sync = []() { __syncthreads(); };

    for (unsigned j = lane; j < kDeflateHashSlots; j += 64) s_hash[j] = 0;
    for (unsigned j = lane; j < dc::kLitTable; j += 64) s_lit_freq[j] = 0;
    if (lane < dc::kDistTable) s_dist_freq[lane] = 0;
    __syncthreads();

    // ---- parse ----
    unsigned long long sum = 0, weighted = 0;
    unsigned ntok = 0, skip = 0;                                        // skip: positions of the next step that a match has covered
    unsigned rep0 = 0, rep1 = 0, rep2 = 0, rep3 = 0;                    // the distances the explorations found, the latest first
    unsigned prev_tokens = 64, wait = 0, fails = 0;                     // tokens of the step before; steps until the next exploration
    for (unsigned b0 = 0; b0 < len; b0 += 64) {
        const unsigned cnt = min(64u, len - b0), i = b0 + lane;
        const bool in = lane < cnt;
        const unsigned char *cur = seg + i;
        const unsigned byte = in ? cur[0] : 0u;
        sum += byte;
        weighted += (unsigned long long)(in ? len - i : 0u) * byte;
        if (skip >= cnt) { skip -= cnt; continue; }                     // (uniform; only a full step can be covered and leave more)
        // the exploration (uniform): every distance of the window at one position, the step's first free one
        bool explore = false;
        if (prev_tokens > kExploreTokens) { if (wait == 0) explore = true; else wait--; }
        if (explore) {
            const unsigned ai = b0 + skip;
            const unsigned char *a = seg + ai;
            const unsigned amax = min(dc::kMaxMatch, len - ai), areach = min(q0 + ai, dc::kWindow);
            unsigned wl = 0, wd = 0;
            if (amax >= 4u) {
                unsigned a32;
                __builtin_memcpy(&a32, a, 4);
                // The window in aligned 16-byte pieces, piece k the one that ends 16 * k bytes below the end of the anchor's own: lane l
                // takes pieces l, l + 64, ... (the nearest first), kExplorePieces of them in flight at a time, each with the word behind
                // it, and finds in registers which of its 16 places start with the anchor's four bytes.
                const uintptr_t at = (uintptr_t)a, top = at & ~(uintptr_t)15;
                const unsigned off = (unsigned)(at - top);
                const unsigned pieces = (areach + 15u - off) / 16u + 1u;   // (the last one starts at most 15 bytes before the window)
                for (unsigned k0 = 0; k0 < pieces; k0 += 64u * kExplorePieces) {
                    uint4 q[kExplorePieces];
                    unsigned e[kExplorePieces];
#pragma unroll
                    for (unsigned u = 0; u < kExplorePieces; u++) {     // the loads first: nothing here waits for the lengths
                        const unsigned k = k0 + 64u * u + lane;
                        q[u] = make_uint4(0u, 0u, 0u, 0u);
                        e[u] = 0u;
                        if (k < pieces) {
                            const uint4 *piece = reinterpret_cast<const uint4 *>(top - 16u * (uintptr_t)k);
                            q[u] = piece[0];
                            e[u] = *reinterpret_cast<const unsigned *>(piece + 1);
                        }
                    }
#pragma unroll
                    for (unsigned u = 0; u < kExplorePieces; u++) {
                        const unsigned k = k0 + 64u * u + lane;
                        if (k >= pieces || wl >= amax) continue;
                        const unsigned w[5] = {q[u].x, q[u].y, q[u].z, q[u].w, e[u]};
                        unsigned mask = 0;
#pragma unroll
                        for (unsigned j = 0; j < 16u; j++) {
                            const unsigned sh = 8u * (j & 3u);
                            const unsigned v = sh ? (w[j >> 2] >> sh) | (w[(j >> 2) + 1u] << (32u - sh)) : w[j >> 2];
                            mask |= (v == a32 ? 1u : 0u) << j;
                        }
                        while (mask) {                                  // the nearest first: the highest place
                            const unsigned j = 31u - (unsigned)__builtin_clz(mask);
                            mask &= ~(1u << j);
                            const int d = (int)(off + 16u * k) - (int)j;
                            if (d < 1 || (unsigned)d > areach || wl >= amax) continue;
                            const unsigned char *c = a - d;
                            if (c[wl] != a[wl]) continue;               // cannot be longer than the lane's best
                            const unsigned l = match_length(a, c, amax);
                            if (l > wl) { wl = l; wd = (unsigned)d; }   // (ascending distances: the nearest among equals)
                        }
                    }
                }
            }
            unsigned key = wl << 16 | (dc::kWindow - wd);               // the longest, the nearest among equals
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor(key, o));
            wl = key >> 16; wd = dc::kWindow - (key & 65535u);
            if (wl >= kExploreMin) {                                    // to the front of the remembered distances
                fails = 0;
                if (wd == rep0) {} else if (wd == rep1) { rep1 = rep0; } else if (wd == rep2) { rep2 = rep1; rep1 = rep0; }
                else { rep3 = rep2; rep2 = rep1; rep1 = rep0; }
                rep0 = wd;
            } else {
                fails++;
                wait = min(1u << min(fails, 5u), 16u) - 1u;
            }
        }
        const unsigned maxlen = in ? min(dc::kMaxMatch, len - i) : 0u;
        const unsigned reach = min(q0 + i, dc::kWindow);                // how far back a match may start
        unsigned best = 0, best_dist = 0;
        const bool hashed = maxlen >= dc::kMinMatch;
        unsigned slot = 0, seen = 0;
        if (hashed) {
            slot = ((byte | (unsigned)cur[1] << 8 | (unsigned)cur[2] << 16) * 2654435761u) >> 20;      // 12 bits
            seen = s_hash[slot];
        }
        if (hashed && lane >= skip) {
            auto candidate = [&](unsigned d) {
                if (d == 0 || d > reach || best >= maxlen) return;
                const unsigned char *c = cur - d;
                if (c[best] != cur[best]) return;                       // (best < maxlen) cannot be longer than the best so far
                const unsigned l = match_length(cur, c, maxlen);
                if (l > best) { best = l; best_dist = d; }
            };
            candidate(1u); candidate(2u); candidate(4u); candidate(8u);
            candidate(R - 1u); candidate(R); candidate(R + 1u);
            candidate(2u * R); candidate(4u * R); candidate(8u * R);
            candidate(rep0); candidate(rep1); candidate(rep2); candidate(rep3);
            if (seen) candidate(i + 1u - seen);
            if (best < dc::kMinMatch || (best == dc::kMinMatch && best_dist > dc::kShortMatchFar)) best = 0;
        }
        __syncthreads();                                                // every lane has read the table
        if (hashed) atomicMax(&s_hash[slot], i + 1u);
        __syncthreads();
        // the walk: wave-uniform
        unsigned long long starts = 0, matches = 0;
        unsigned p = skip;
        while (p < cnt) {
            p = (unsigned)__builtin_amdgcn_readfirstlane((int)p);
            unsigned L = (unsigned)__builtin_amdgcn_readlane((int)best, (int)p);
            if (L && p + 1u < cnt && (unsigned)__builtin_amdgcn_readlane((int)best, (int)(p + 1u)) > L) L = 0;
            starts |= 1ull << p;
            if (L) { matches |= 1ull << p; p += L; } else p++;
        }
        skip = p - cnt;
        if ((starts >> lane) & 1ull) {
            const bool is_match = (matches >> lane) & 1ull;
            const unsigned at = ntok + (unsigned)__popcll(starts & ((1ull << lane) - 1ull));
            tok[at] = is_match ? dc::tok_match(best, best_dist) : byte;   // (at <= b0 + lane: below tok_stride - 1)
            if (is_match) {
                atomicAdd(&s_lit_freq[dc::length_symbol(best).sym], 1u);
                atomicAdd(&s_dist_freq[dc::dist_symbol(best_dist).sym], 1u);
            } else {
                atomicAdd(&s_lit_freq[byte], 1u);
            }
        }
        prev_tokens = (unsigned)__popcll(starts);
        ntok += prev_tokens;
    }
    if (lane == 0) { tok[ntok] = dc::kEob; s_lit_freq[dc::kEob] = 1; }
    ntok++;
    sum = wave_sum(sum);
    weighted = wave_sum(weighted);
    if (lane == 0) { sums[2 * (size_t)sg] = sum; sums[2 * (size_t)sg + 1] = weighted; }
    __syncthreads();

    // ---- tables ----
    dc::code_lengths(s_lit_freq, dc::kLitSyms, dc::kLitLimit, s_lit_lens, s_work, lane, 64u, sync);
    dc::code_lengths(s_dist_freq, dc::kDistSyms, dc::kLitLimit, s_dist_lens, s_work, lane, 64u, sync);
    if (lane == 0) {
        unsigned hlit = dc::kLitSyms, hdist = dc::kDistSyms;
        while (hlit > 257u && s_lit_lens[hlit - 1u] == 0) hlit--;
        while (hdist > 1u && s_dist_lens[hdist - 1u] == 0) hdist--;
        s_head[0] = dc::rle_lengths(s_lit_lens, hlit, s_dist_lens, hdist, s_rle, s_cl_freq);
        s_head[1] = hlit; s_head[2] = hdist;
        for (unsigned s = 0; s < dc::kClSyms; s++) s_cl_sent[s] = s_cl_freq[s];
        dc::cl_complete(s_cl_freq);
    }
    __syncthreads();
    dc::code_lengths(s_cl_freq, dc::kClSyms, dc::kClLimit, s_cl_lens, s_work, lane, 64u, sync);
    const unsigned long long dyn = 3u + dc::header_bits(s_cl_sent, s_cl_lens)
                                   + wave_sum(dc::body_bits_dynamic(s_lit_freq, s_lit_lens, s_dist_freq, s_dist_lens, lane, 64u));
    const unsigned long long fix = 3u + wave_sum(dc::body_bits_fixed(s_lit_freq, s_dist_freq, lane, 64u));
    const bool dynamic = dyn < fix;                                     // (uniform)
    const unsigned nrle = s_head[0], hlit = s_head[1], hdist = s_head[2];
    __syncthreads();
    if (dynamic) {
        dc::canonical_codes(s_cl_lens, dc::kClSyms, s_cl_codes, s_work, lane, 64u, sync);
    } else {
        for (unsigned s = lane; s < dc::kLitTable; s += 64) s_lit_lens[s] = (uint8_t)dc::fixed_lit_len(s);
        if (lane < dc::kDistTable) s_dist_lens[lane] = (uint8_t)dc::kFixedDistLen;
        __syncthreads();
    }
    dc::canonical_codes(s_lit_lens, dynamic ? dc::kLitSyms : dc::kLitTable, s_lit_codes, s_work, lane, 64u, sync);
    dc::canonical_codes(s_dist_lens, dynamic ? dc::kDistSyms : dc::kDistTable, s_dist_codes, s_work, lane, 64u, sync);

    // ---- emit ----
    for (unsigned j = lane; j < kEmitWords; j += 64) s_buf[j] = 0;
    __syncthreads();
    unsigned wpos = 0, carried = 0;                                     // words that have left; bits (< 32) waiting in s_buf[0]
    auto emit = [&](unsigned long long v, unsigned nb) {                // every lane's bits, in lane order
        unsigned incl = nb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(incl, o);
            if (lane >= (unsigned)o) incl += up;
        }
        const unsigned total = carried + __shfl(incl, 63), at = carried + incl - nb;
        if (nb) {
            const unsigned w = at >> 5, sh = at & 31u;
            const unsigned long long low = v << sh;
            const unsigned high = sh ? (unsigned)(v >> (64u - sh)) : 0u;
            if ((unsigned)low) atomicOr(&s_buf[w], (unsigned)low);
            if ((unsigned)(low >> 32)) atomicOr(&s_buf[w + 1u], (unsigned)(low >> 32));
            if (high) atomicOr(&s_buf[w + 2u], high);
        }
        __syncthreads();
        const unsigned full = total >> 5;                               // (<= 96)
        for (unsigned j = lane; j < full; j += 64) out[wpos + j] = s_buf[j];
        const unsigned rest = s_buf[full];
        __syncthreads();
        for (unsigned j = lane; j < full + 3u; j += 64) s_buf[j] = 0;   // (full + 2 <= 98)
        __syncthreads();
        if (lane == 0) s_buf[0] = rest;
        __syncthreads();
        wpos += full;
        carried = total & 31u;
    };
    if (dynamic) {
        const unsigned hclen = dc::header_hclen(s_cl_lens);
        unsigned long long v = 0;
        unsigned nb = 0;
        if (lane == 0) { v = (last ? 1u : 0u) | 2u << 1 | (hlit - 257u) << 3 | (hdist - 1u) << 8 | (hclen - 4u) << 13; nb = 17; }
        else if (lane <= hclen) { v = s_cl_lens[dc::cl_order(lane - 1u)]; nb = 3; }
        emit(v, nb);
        for (unsigned b0 = 0; b0 < nrle; b0 += 64) {
            v = 0; nb = 0;
            if (b0 + lane < nrle) {
                const unsigned e = s_rle[b0 + lane], s = e & 31u;
                v = s_cl_codes[s] | (unsigned long long)(e >> 5) << s_cl_lens[s];
                nb = s_cl_lens[s] + dc::cl_extra_bits(s);
            }
            emit(v, nb);
        }
    } else {
        emit(lane == 0 ? ((last ? 1u : 0u) | 1u << 1) : 0u, lane == 0 ? 3u : 0u);
    }
    for (unsigned b0 = 0; b0 < ntok; b0 += 64) {
        dc::TokBits t{0, 0};
        if (b0 + lane < ntok) t = dc::token_bits(tok[b0 + lane], s_lit_codes, s_lit_lens, s_dist_codes, s_dist_lens);
        emit(t.bits, t.nbits);
    }
    if (lane == 0) {
        if (carried) out[wpos] = s_buf[0];
        seg_bits[sg] = wpos * 32u + carried;
    }
}

void launch_deflate(const unsigned char *d_maps, size_t frames, size_t n, size_t width, const LzwFrame *d_frames, const unsigned long long *d_base,
                    size_t stream_bytes, size_t S, size_t seg_len, size_t tok_stride, size_t stride, unsigned char *d_stream, unsigned *d_tokens,
                    unsigned *d_stage, unsigned *d_bits, unsigned long long *d_gbit, unsigned long long *d_words, unsigned *d_out, size_t out_words,
                    hipStream_t s) {
    if (frames == 0 || S == 0) return;
    if (!d_maps || !d_frames || !d_base || !d_stream || !d_tokens || !d_stage || !d_bits || !d_gbit || !d_words || !d_out)
        throw HipError("patolette_amd: png_deflate needs maps and its workspace");
    if (seg_len < 1 || seg_len > kDeflateSegmentMax) throw HipError("patolette_amd: png_deflate: segment out of range");
    if ((uintptr_t)d_stream & 15u) throw HipError("patolette_amd: png_deflate needs its filtered streams 16-byte aligned");
    const size_t filter_blocks = ceil_div(stream_bytes, 256), pack_blocks = ceil_div(out_words, 256);
    if (frames >> 31 || S >> 31 || pack_blocks >> 31 || filter_blocks >> 31 || width >> 32)
        throw HipError("patolette_amd: png_deflate: a size does not fit the kernels' 32-bit fields");
    HIP_CHECK(hipMemsetAsync(d_words, 0, sizeof(unsigned long long), s));
    {
        KTIME("k_png_filter", s, 2.0 * stream_bytes);
        hipLaunchKernelGGL(k_png_filter, (unsigned)filter_blocks, 256, 0, s, d_maps, n, (unsigned)width, d_frames, d_base, (unsigned)frames,
                           (unsigned long long)stream_bytes, d_stream);
        HIP_CHECK(hipGetLastError());
    }
    {
        KTIME("k_deflate_segments", s, 1.0 * stream_bytes);
        hipLaunchKernelGGL(k_deflate_segments, (unsigned)S, 64, 0, s, d_stream, d_base, d_frames, (unsigned)frames, (unsigned)seg_len, tok_stride,
                           d_tokens, stride, d_stage, d_bits, d_words + (frames + 2));
        HIP_CHECK(hipGetLastError());
    }
    lzw_offsets_and_pack(frames, d_frames, S, stride, d_stage, d_bits, d_gbit, d_words, d_out, out_words, pack_blocks, s);
}

}  // namespace pamd
