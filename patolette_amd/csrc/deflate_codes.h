// deflate_codes.h -- the code tables of a deflate block (RFC 1951): plain C++ for the host and the device.
//
// What deflate.hip's kernel and the host share: a token's symbols and extra bits, length-limited prefix code lengths from a histogram,
// canonical codes, the run-length coding of the code lengths (symbols 16, 17, 18), the header's cost -- and, for the host alone,
// write_block, which writes one complete block for a token list through exactly these routines (tests/deflate_codes_check.cpp).
//
// The routines that take (lane, lanes, sync) spread their independent work over `lanes` callers that all call them with the same
// arguments and meet at sync(); the host passes (0, 1) and a sync that does nothing.  The serial parts run in lane 0.
// Every choice is made by value and position (histogram ties go by symbol number), so the tables are a function of the histogram alone.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define DC_HD __host__ __device__
#else
#define DC_HD
#endif

namespace pamd {
namespace dc {

constexpr unsigned kLitSyms = 286, kLitTable = 288, kDistSyms = 30, kDistTable = 32, kClSyms = 19;
constexpr unsigned kLitLimit = 15, kClLimit = 7, kEob = 256;
constexpr unsigned kMinMatch = 3, kMaxMatch = 258, kWindow = 32768;
// a match of three bytes further back than this costs more than its literals do in most tables (zlib's TOO_FAR)
constexpr unsigned kShortMatchFar = 4096;

// A token: a literal or the end of block (its symbol, 0 .. 256), or a match: kTokMatch | (length - 3) << 16 | (distance - 1)
constexpr uint32_t kTokMatch = 0x80000000u;
DC_HD inline uint32_t tok_match(unsigned len, unsigned dist) { return kTokMatch | (len - 3u) << 16 | (dist - 1u); }
DC_HD inline bool tok_is_match(uint32_t t) { return (t & kTokMatch) != 0; }
DC_HD inline unsigned tok_len(uint32_t t) { return ((t >> 16) & 255u) + 3u; }
DC_HD inline unsigned tok_dist(uint32_t t) { return (t & 32767u) + 1u; }

DC_HD inline unsigned floor_log2(unsigned v) {                          // v >= 1
    unsigned r = 0;
    while (v >>= 1) r++;
    return r;
}

// A length's symbol (257 .. 285), the count of its extra bits and their value; l = length - 3
struct SymBits { unsigned sym, nbits, bits; };
DC_HD inline SymBits length_symbol(unsigned len) {
    const unsigned l = len - 3u;
    if (l < 8u) return SymBits{257u + l, 0u, 0u};
    if (l == 255u) return SymBits{285u, 0u, 0u};
    const unsigned eb = floor_log2(l) - 2u;
    return SymBits{261u + 4u * eb + ((l >> eb) & 3u), eb, l & ((1u << eb) - 1u)};
}
// A distance's symbol (0 .. 29)
DC_HD inline SymBits dist_symbol(unsigned dist) {
    const unsigned d = dist - 1u;
    if (d < 4u) return SymBits{d, 0u, 0u};
    const unsigned eb = floor_log2(d) - 1u;
    return SymBits{2u * eb + 2u + ((d >> eb) & 1u), eb, d & ((1u << eb) - 1u)};
}
// extra bits of a literal/length symbol and of a distance symbol
DC_HD inline unsigned lit_extra_bits(unsigned sym) { return sym < 265u || sym >= 285u ? 0u : (sym - 261u) >> 2; }
DC_HD inline unsigned dist_extra_bits(unsigned sym) { return sym < 4u ? 0u : (sym - 2u) >> 1; }
// the fixed code's lengths (RFC 1951, 3.2.6); its codes are the canonical ones of these lengths
DC_HD inline unsigned fixed_lit_len(unsigned sym) { return sym < 144u ? 8u : sym < 256u ? 9u : sym < 280u ? 7u : 8u; }
constexpr unsigned kFixedDistLen = 5;

DC_HD inline unsigned reverse_bits(unsigned code, unsigned len) {      // a code as it goes into an LSB-first stream
    unsigned r = 0;
    for (unsigned i = 0; i < len; i++) r |= ((code >> i) & 1u) << (len - 1u - i);
    return r;
}

// Scratch of code_lengths and canonical_codes (the device keeps one in LDS)
struct Work {
    uint32_t a[kLitTable];                                              // the weights in ascending order, then parents, then depths
    uint16_t order[kLitTable];                                          // the used symbols, ascending by (weight, symbol)
    uint32_t count[16], next[16];                                       // symbols per length; the first code of a length
    uint32_t used;
};

struct NoSync { DC_HD void operator()() const {} };

// Code lengths of a prefix code for the histogram freq[0 .. n), none above `limit` (n <= 288 with limit 15, n <= 19 with limit 7; the
// weights' sum below 2^32): lens[s] = 0 for an unused symbol.  Two and more used symbols: a complete code (Kraft sum exactly 1), the
// Huffman code whenever that is no deeper than the limit.  One used symbol: length 1.  None: all 0.
// The tree: Moffat and Katajainen's in-place algorithm over the sorted weights.  Too deep: every length above the limit becomes the
// limit, and, while the Kraft sum is above 1, a code at the limit goes and the deepest code above it is split in two one level down;
// the lengths then go to the symbols in order of weight.
template <class Sync>
DC_HD inline void code_lengths(const uint32_t *freq, unsigned n, unsigned limit, uint8_t *lens, Work &w, unsigned lane, unsigned lanes, Sync sync) {
    for (unsigned s = lane; s < n; s += lanes) {                        // a symbol's place: the used symbols before it in the order
        lens[s] = 0;
        const uint32_t f = freq[s];
        if (f == 0) continue;
        unsigned rank = 0;
        for (unsigned t = 0; t < n; t++) {
            const uint32_t g = freq[t];
            rank += (g != 0 && (g < f || (g == f && t < s))) ? 1u : 0u;
        }
        w.order[rank] = (uint16_t)s;
    }
    sync();
    if (lane == 0) {
        unsigned m = 0;
        for (unsigned s = 0; s < n; s++) m += freq[s] != 0 ? 1u : 0u;
        w.used = m;
        if (m == 1) lens[w.order[0]] = 1;
        if (m >= 2) {
            uint32_t *A = w.a;
            for (unsigned i = 0; i < m; i++) A[i] = freq[w.order[i]];
            // phase 1: internal nodes' weights, then parents
            A[0] += A[1];
            unsigned root = 0, leaf = 2;
            for (unsigned next = 1; next + 1 < m; next++) {
                if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
                if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
            }
            // phase 2: internal nodes' depths
            A[m - 2] = 0;
            for (int next = (int)m - 3; next >= 0; next--) A[next] = A[A[next]] + 1u;
            // phase 3: leaves' depths, A[0] the deepest
            int avbl = 1, used = 0, dpth = 0, rt = (int)m - 2, nx = (int)m - 1;
            while (avbl > 0) {
                while (rt >= 0 && (int)A[rt] == dpth) { used++; rt--; }
                while (avbl > used) { A[nx--] = (uint32_t)dpth; avbl--; }
                avbl = 2 * used; dpth++; used = 0;
            }
            for (unsigned l = 0; l < 16; l++) w.count[l] = 0;
            for (unsigned i = 0; i < m; i++) w.count[A[i] < limit ? A[i] : limit]++;
            uint32_t total = 0;                                         // the Kraft sum in units of 2^-limit
            for (unsigned l = 1; l <= limit; l++) total += w.count[l] << (limit - l);
            while (total > (1u << limit)) {
                w.count[limit]--;
                for (unsigned l = limit - 1; l > 0; l--)
                    if (w.count[l]) { w.count[l]--; w.count[l + 1] += 2; break; }
                total--;
            }
            unsigned i = 0;                                             // the lightest symbols get the longest codes
            for (unsigned l = limit; l > 0; l--)
                for (uint32_t c = 0; c < w.count[l]; c++) lens[w.order[i++]] = (uint8_t)l;
        }
    }
    sync();
}

// The canonical codes of lens[0 .. n), bit-reversed for the LSB-first stream (0 for an unused symbol)
template <class Sync>
DC_HD inline void canonical_codes(const uint8_t *lens, unsigned n, uint16_t *codes, Work &w, unsigned lane, unsigned lanes, Sync sync) {
    if (lane == 0) {
        for (unsigned l = 0; l < 16; l++) w.count[l] = 0;
        for (unsigned s = 0; s < n; s++) w.count[lens[s]]++;
        w.count[0] = 0;
        uint32_t code = 0;
        for (unsigned l = 1; l < 16; l++) { code = (code + w.count[l - 1]) << 1; w.next[l] = code; }
        for (unsigned s = 0; s < n; s++) w.a[s] = lens[s] ? w.next[lens[s]]++ : 0u;
    }
    sync();
    for (unsigned s = lane; s < n; s += lanes) codes[s] = (uint16_t)reverse_bits(w.a[s], lens[s]);
    sync();
}

// The order in which the header lists the lengths of the code-length code
DC_HD inline unsigned cl_order(unsigned i) {
    const uint8_t o[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}

// The run-length coding of the hlit literal/length lengths followed by the hdist distance lengths: rle[i] = symbol | extra value << 5,
// at most hlit + hdist of them; cl_freq[19] counts the symbols.  Returns their number.  Serial: one caller.
// A run of zeros: 18 for every 11 .. 138 of it, then 17 for 3 .. 10, else zeros; a run of another length: the length once, 16 for every
// 3 .. 6 repeats, else the length again.
DC_HD inline unsigned rle_lengths(const uint8_t *lit_lens, unsigned hlit, const uint8_t *dist_lens, unsigned hdist, uint16_t *rle, uint32_t *cl_freq) {
    for (unsigned s = 0; s < kClSyms; s++) cl_freq[s] = 0;
    const unsigned total = hlit + hdist;
    unsigned out = 0, i = 0;
    while (i < total) {
        const unsigned v = i < hlit ? lit_lens[i] : dist_lens[i - hlit];
        unsigned run = 1;
        while (i + run < total && (i + run < hlit ? lit_lens[i + run] : dist_lens[i + run - hlit]) == v) run++;
        i += run;
        if (v == 0) {
            while (run >= 11) { const unsigned r = run < 138u ? run : 138u; rle[out++] = (uint16_t)(18u | (r - 11u) << 5); cl_freq[18]++; run -= r; }
            if (run >= 3) { rle[out++] = (uint16_t)(17u | (run - 3u) << 5); cl_freq[17]++; run = 0; }
        } else {
            rle[out++] = (uint16_t)v; cl_freq[v]++; run--;
            while (run >= 3) { const unsigned r = run < 6u ? run : 6u; rle[out++] = (uint16_t)(16u | (r - 3u) << 5); cl_freq[16]++; run -= r; }
        }
        for (; run > 0; run--) { rle[out++] = (uint16_t)v; cl_freq[v]++; }
    }
    return out;
}
DC_HD inline unsigned cl_extra_bits(unsigned sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }

// The code-length code must be complete even with one used symbol: a second one is counted in (its code is never sent)
DC_HD inline void cl_complete(uint32_t *cl_freq) {
    unsigned used = 0;
    for (unsigned s = 0; s < kClSyms; s++) used += cl_freq[s] != 0 ? 1u : 0u;
    if (used == 1) cl_freq[cl_freq[0] ? 1 : 0] = 1;
}
// how many of the code-length code's lengths the header lists (4 .. 19)
DC_HD inline unsigned header_hclen(const uint8_t *cl_lens) {
    unsigned h = kClSyms;
    while (h > 4 && cl_lens[cl_order(h - 1)] == 0) h--;
    return h;
}
// bits of a dynamic block's header behind the three of BFINAL and BTYPE; cl_sent: the counts of the symbols that are sent
DC_HD inline uint32_t header_bits(const uint32_t *cl_sent, const uint8_t *cl_lens) {
    uint32_t bits = 5 + 5 + 4 + 3 * header_hclen(cl_lens);
    for (unsigned s = 0; s < kClSyms; s++) bits += cl_sent[s] * (cl_lens[s] + cl_extra_bits(s));
    return bits;
}
// bits of the tokens counted in the two histograms under the given lengths (extra bits included); symbols lane, lane + lanes, ...
DC_HD inline uint64_t body_bits_dynamic(const uint32_t *lit_freq, const uint8_t *lit_lens, const uint32_t *dist_freq, const uint8_t *dist_lens,
                                        unsigned lane, unsigned lanes) {
    uint64_t bits = 0;
    for (unsigned s = lane; s < kLitSyms; s += lanes) bits += (uint64_t)lit_freq[s] * (lit_lens[s] + lit_extra_bits(s));
    for (unsigned s = lane; s < kDistSyms; s += lanes) bits += (uint64_t)dist_freq[s] * (dist_lens[s] + dist_extra_bits(s));
    return bits;
}
DC_HD inline uint64_t body_bits_fixed(const uint32_t *lit_freq, const uint32_t *dist_freq, unsigned lane, unsigned lanes) {
    uint64_t bits = 0;
    for (unsigned s = lane; s < kLitSyms; s += lanes) bits += (uint64_t)lit_freq[s] * (fixed_lit_len(s) + lit_extra_bits(s));
    for (unsigned s = lane; s < kDistSyms; s += lanes) bits += (uint64_t)dist_freq[s] * (kFixedDistLen + dist_extra_bits(s));
    return bits;
}
// Bits that hold any block of `len` bytes coded with the fixed code: three of header, at most 9 a byte -- a literal's 8 or 9; a match of
// 3 .. 10 bytes 7 + 5 + 13 = 25 <= 27; a longer one at most 8 + 5 + 5 + 13 = 31 -- and the end of block's 7.  The coder takes
// the cheaper of the dynamic and the fixed block, so this holds whatever the content.
DC_HD inline uint64_t block_bound_bits(uint64_t len) { return 9 * len + 10; }

// A token's bits in the stream's order (LSB first) and their count (at most 48): the codes and lengths are the block's tables
struct TokBits { uint64_t bits; unsigned nbits; };
DC_HD inline TokBits token_bits(uint32_t tok, const uint16_t *lit_codes, const uint8_t *lit_lens, const uint16_t *dist_codes, const uint8_t *dist_lens) {
    if (!tok_is_match(tok)) return TokBits{lit_codes[tok], lit_lens[tok]};
    const SymBits L = length_symbol(tok_len(tok)), D = dist_symbol(tok_dist(tok));
    uint64_t v = lit_codes[L.sym];
    unsigned nb = lit_lens[L.sym];
    v |= (uint64_t)L.bits << nb; nb += L.nbits;
    v |= (uint64_t)dist_codes[D.sym] << nb; nb += dist_lens[D.sym];
    v |= (uint64_t)D.bits << nb; nb += D.nbits;
    return TokBits{v, nb};
}

}  // namespace dc
}  // namespace pamd

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace pamd {
namespace dc {

// An LSB-first bit string on the host
struct BitWriter {
    std::vector<uint8_t> bytes;
    uint64_t nbits = 0;
    void put(uint64_t v, unsigned n) {                                  // n <= 48
        for (unsigned i = 0; i < n; i++, nbits++) {
            if ((nbits & 7u) == 0) bytes.push_back(0);
            bytes.back() |= (uint8_t)(((v >> i) & 1u) << (nbits & 7u));
        }
    }
};

// One complete block for tokens[0 .. count) -- the end of block is appended here --: the dynamic block, or the fixed one where that
// is no larger, by the routines above, as the device's coder decides and writes it.  Returns the block's bits.
inline uint64_t write_block(const uint32_t *tokens, size_t count, bool final_block, BitWriter &bw) {
    uint32_t lit_freq[kLitTable] = {0}, dist_freq[kDistTable] = {0}, cl_freq[kClSyms], cl_sent[kClSyms];
    uint8_t lit_lens[kLitTable] = {0}, dist_lens[kDistTable] = {0}, cl_lens[kClSyms] = {0};
    uint16_t lit_codes[kLitTable] = {0}, dist_codes[kDistTable] = {0}, cl_codes[kClSyms] = {0}, rle[kLitTable + kDistTable];
    Work w;
    const NoSync sync;
    for (size_t i = 0; i < count; i++) {
        if (tok_is_match(tokens[i])) { lit_freq[length_symbol(tok_len(tokens[i])).sym]++; dist_freq[dist_symbol(tok_dist(tokens[i])).sym]++; }
        else lit_freq[tokens[i]]++;
    }
    lit_freq[kEob]++;
    code_lengths(lit_freq, kLitSyms, kLitLimit, lit_lens, w, 0, 1, sync);
    code_lengths(dist_freq, kDistSyms, kLitLimit, dist_lens, w, 0, 1, sync);
    unsigned hlit = kLitSyms, hdist = kDistSyms;
    while (hlit > 257 && lit_lens[hlit - 1] == 0) hlit--;
    while (hdist > 1 && dist_lens[hdist - 1] == 0) hdist--;
    const unsigned nrle = rle_lengths(lit_lens, hlit, dist_lens, hdist, rle, cl_freq);
    for (unsigned s = 0; s < kClSyms; s++) cl_sent[s] = cl_freq[s];
    cl_complete(cl_freq);
    code_lengths(cl_freq, kClSyms, kClLimit, cl_lens, w, 0, 1, sync);
    const uint64_t dyn = 3 + header_bits(cl_sent, cl_lens) + body_bits_dynamic(lit_freq, lit_lens, dist_freq, dist_lens, 0, 1);
    const uint64_t fix = 3 + body_bits_fixed(lit_freq, dist_freq, 0, 1);
    const uint64_t before = bw.nbits;
    const bool dynamic = dyn < fix;
    bw.put(final_block ? 1 : 0, 1);
    bw.put(dynamic ? 2 : 1, 2);
    if (dynamic) {
        canonical_codes(cl_lens, kClSyms, cl_codes, w, 0, 1, sync);
        const unsigned hclen = header_hclen(cl_lens);
        bw.put(hlit - 257, 5); bw.put(hdist - 1, 5); bw.put(hclen - 4, 4);
        for (unsigned i = 0; i < hclen; i++) bw.put(cl_lens[cl_order(i)], 3);
        for (unsigned i = 0; i < nrle; i++) {
            const unsigned s = rle[i] & 31u;
            bw.put(cl_codes[s], cl_lens[s]);
            bw.put(rle[i] >> 5, cl_extra_bits(s));
        }
    } else {
        for (unsigned s = 0; s < kLitTable; s++) lit_lens[s] = (uint8_t)fixed_lit_len(s);
        for (unsigned s = 0; s < kDistTable; s++) dist_lens[s] = (uint8_t)kFixedDistLen;
    }
    canonical_codes(lit_lens, dynamic ? kLitSyms : kLitTable, lit_codes, w, 0, 1, sync);
    canonical_codes(dist_lens, dynamic ? kDistSyms : kDistTable, dist_codes, w, 0, 1, sync);
    for (size_t i = 0; i <= count; i++) {
        const TokBits t = token_bits(i < count ? tokens[i] : kEob, lit_codes, lit_lens, dist_codes, dist_lens);
        bw.put(t.bits, t.nbits);
    }
    (void)before;
    return bw.nbits - before;
}

}  // namespace dc
}  // namespace pamd
#endif
