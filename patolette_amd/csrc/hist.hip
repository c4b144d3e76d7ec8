// hist.hip -- an exact colour histogram of 8-bit pixels kept in HBM and filled over many calls, on gfx950: include/patolette_amd.h,
// "ColorHistogram"; the table's layout is in hist.h.
//
// Everything accumulated is an integer: a 64-bit count per key and, in a weighted table, a 64-bit sum of weight units (2^-32).
// Integer adds commute, so the table is a function of the multiset of (key, units) pairs that entered it: no partition, merge
// scheme, grid shape or timing can change a bit of it.  That leaves the scheme free to be chosen for speed:
//   k_hist_units   f64 weights -> units, with the flag for a weight that is not finite or outside [0, 2^20].  A pass of its own,
//                  checked by the host before k_hist_add is enqueued: a refused add has touched nothing.
//   k_hist_add     a lane reads kHistLanePixels consecutive pixels (words where the pointer allows, bytes otherwise), merges runs
//                  of equal keys in registers and hands each run to the block's LDS table (one probe: a slot that holds another
//                  key sends the run to the global table at once).  After kHistBlockTiles tiles the block flushes its slots with
//                  one set of global atomics each: 64-bit integer adds, relaxed, agent scope.
//   k_hist_merge, k_hist_totals: one streaming pass over the bins each.  Export: compact.h over the bins.
// Overflow of a unit sum is looked for wherever a sum of unit values can wrap: in the LDS slot (the returning ds atomic), in the
// global bin (the returning global atomic), in the merge.  A lane's run cannot wrap: it spans at most kHistLanePixels *
// kHistBlockTiles = 64 pixels of at most 2^52 units (a static_assert in k_hist_add holds the constants to that).  A partial sum
// never exceeds the key's true sum, and a true sum of 2^64 or more wraps at one of the checked adds at least: the flag is raised
// exactly when a key's sum passes 2^64.
#include "hist.h"

namespace pamd {

using ull = unsigned long long;

__global__ __launch_bounds__(256) void k_hist_units(const double *__restrict__ w, size_t N, ull *__restrict__ units, unsigned *flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const double v = w[i];
        const bool ok = v >= 0.0 && v <= kHistMaxWeight;                 // (NaN fails both)
        bad |= !ok;
        units[i] = ok ? (ull)rint(v * kHistUnit) : 0ull;                 // the scaling is exact; ties to even
    }
    if (__ballot(bad) && (threadIdx.x & 63u) == 0) atomicOr(flag, 1u);
}

template <bool W>
__device__ __forceinline__ bool hist_global_add(ull *counts, ull *units, unsigned key, ull c, ull u) {
    __hip_atomic_fetch_add(counts + key, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (W) {
        if (u) {
            const ull old = __hip_atomic_fetch_add(units + key, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return old + u < old;
        }
    }
    return false;
}

// CH: bytes per pixel.  WORDS: px is 4-byte aligned, a lane's full stretch is read as 32-bit words.  W: a weighted table.
// thr: -1, or (CH == 4) the alpha below which a pixel enters nothing.  bt: tiles per block.
template <int CH, bool WORDS, bool W>
__global__ __launch_bounds__(256) void k_hist_add(ull *__restrict__ counts, ull *__restrict__ units, unsigned *flags,
                                                  const unsigned char *__restrict__ px, size_t N, int thr, const ull *__restrict__ pu,
                                                  unsigned bt) {
    constexpr int P = kHistLanePixels;
    // a lane's run holds at most P * kHistBlockTiles pixels of at most 2^52 units each: below 2^64 while that product is below 4096
    static_assert((unsigned long long)kHistLanePixels * kHistBlockTiles < 4096, "a lane's run of weight units could wrap");
    constexpr unsigned S = 1u << kHistSlotsLog2, EMPTY = 0xFFFFFFFFu;
    __shared__ unsigned s_key[S], s_cnt[S];
    __shared__ ull s_units[W ? S : 1];
    const unsigned tid = threadIdx.x;
    for (unsigned j = tid; j < S; j += 256) { s_key[j] = EMPTY; s_cnt[j] = 0; if (W) s_units[j] = 0; }
    __syncthreads();
    bool ovf = false;
    // a run of equal keys into the block's table; a slot taken by another key: straight to the global table
    auto emit = [&](unsigned key, unsigned c, ull u) {
        const unsigned h = (key * 2654435761u) >> (32 - kHistSlotsLog2);
        const unsigned was = atomicCAS(&s_key[h], EMPTY, key);
        if (was == EMPTY || was == key) {
            atomicAdd(&s_cnt[h], c);
            if constexpr (W) {
                if (u) { const ull old = atomicAdd(&s_units[h], u); ovf |= old + u < old; }
            }
        } else ovf |= hist_global_add<W>(counts, units, key, c, u);
    };
    unsigned rkey = EMPTY, rcnt = 0;                                     // the lane's run; it lives across the block's tiles
    ull ru = 0;
    for (unsigned t = 0; t < bt; t++) {
        const size_t p0 = ((size_t)blockIdx.x * bt + t) * kHistTile + (size_t)tid * P;
        if (p0 >= N) break;
        unsigned v[P];                                                   // the key, or EMPTY for a pixel that enters nothing
        if (WORDS && p0 + P <= N) {
            const unsigned *q = reinterpret_cast<const unsigned *>(px + p0 * CH);      // (p0 is a multiple of 8: a whole word)
            unsigned wd[P * CH / 4];
#pragma unroll
            for (int j = 0; j < P * CH / 4; j++) wd[j] = q[j];
#pragma unroll
            for (int j = 0; j < P; j++) {
                auto byte = [&](int k) { return (wd[k >> 2] >> (8 * (k & 3))) & 255u; };
                v[j] = byte(CH * j) << 16 | byte(CH * j + 1) << 8 | byte(CH * j + 2);
                if constexpr (CH == 4) { if ((int)byte(CH * j + 3) < thr) v[j] = EMPTY; }
            }
        } else {
#pragma unroll
            for (int j = 0; j < P; j++) {
                v[j] = EMPTY;
                if (p0 + j < N) {
                    const unsigned char *q = px + (p0 + j) * CH;
                    v[j] = (unsigned)q[0] << 16 | (unsigned)q[1] << 8 | (unsigned)q[2];
                    if (CH == 4 && (int)q[CH - 1] < thr) v[j] = EMPTY;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < P; j++) {
            if (v[j] == EMPTY) continue;
            ull u = 0;
            if constexpr (W) u = pu[p0 + j];
            if (v[j] == rkey) {
                rcnt++;
                if constexpr (W) ru += u;                                // (cannot wrap: the static_assert above)
            } else {
                if (rcnt) emit(rkey, rcnt, ru);
                rkey = v[j]; rcnt = 1; ru = u;
            }
        }
    }
    if (rcnt) emit(rkey, rcnt, ru);
    __syncthreads();
    for (unsigned j = tid; j < S; j += 256)
        if (s_key[j] != EMPTY) ovf |= hist_global_add<W>(counts, units, s_key[j], (ull)s_cnt[j], W ? s_units[j] : 0ull);
    if (__ballot(ovf) && (tid & 63u) == 0) atomicOr(flags, 1u);
}

__global__ __launch_bounds__(256) void k_hist_merge(ull *__restrict__ dc, const ull *__restrict__ sc, ull *__restrict__ du,
                                                    const ull *__restrict__ su, unsigned *flags) {
    bool ovf = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < kHistBins; i += (size_t)gridDim.x * 256) {
        const ull c = sc[i];
        if (c == 0) continue;                                            // (no units without a count)
        dc[i] += c;
        if (du) {
            const ull b = su[i];
            if (b) { const ull a = du[i], s = a + b; ovf |= s < a; du[i] = s; }
        }
    }
    if (__ballot(ovf) && (threadIdx.x & 63u) == 0) atomicOr(flags, 1u);
}

__global__ __launch_bounds__(256) void k_hist_totals(const ull *__restrict__ counts, ull *out) {
    ull px = 0, colors = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < kHistBins; i += (size_t)gridDim.x * 256) {
        const ull c = counts[i];
        px += c; colors += c != 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { px += __shfl_xor(px, o); colors += __shfl_xor(colors, o); }
    if ((threadIdx.x & 63u) == 0 && colors) { atomicAdd(out, px); atomicAdd(out + 1, colors); }
}

// compact.h's operation over the bins.  W: a weighted table.  POS: keep only bins whose weight is > 0 as well (the palette's list)
template <bool W, bool POS>
struct HistExportOp {
    struct V { ull c, u; };
    const ull *counts, *units;
    unsigned char *rgb;
    ull *out_c;
    double *out_w;
    __device__ V load(size_t i) const { V v; v.c = counts[i]; v.u = (W && v.c) ? units[i] : 0ull; return v; }
    __device__ bool keep(V v) const { return v.c > 0 && (!(W && POS) || v.u > 0); }
    __device__ void put(size_t i, V v, bool k, unsigned r) const {
        if (!k) return;
        unsigned char *o = rgb + 3 * (size_t)r;
        o[0] = (unsigned char)(i >> 16); o[1] = (unsigned char)(i >> 8); o[2] = (unsigned char)i;
        if (out_c) out_c[r] = v.c;
        out_w[r] = W ? (double)v.u * (1.0 / kHistUnit) : (double)v.c;    // one rounding (u64 -> f64); the scaling is exact
    }
};

void launch_hist_units(const double *d_weights, size_t N, ull *d_units, unsigned *d_flag, hipStream_t s) {
    if (N == 0) return;
    const unsigned blocks = (unsigned)std::min<size_t>(ceil_div(N, 256), (size_t)num_cus() * 16);
    KTIME("k_hist_units", s, 16.0 * N);
    hipLaunchKernelGGL(k_hist_units, blocks, 256, 0, s, d_weights, N, d_units, d_flag);
    HIP_CHECK(hipGetLastError());
}

template <int CH, bool WORDS>
static void hist_add_typed(ull *d_hist, bool weighted, unsigned blocks, const unsigned char *d_px, size_t N, int thr, const ull *d_units,
                           unsigned bt, hipStream_t s) {
    unsigned *flags = reinterpret_cast<unsigned *>(d_hist);
    if (weighted)
        hipLaunchKernelGGL((k_hist_add<CH, WORDS, true>), blocks, 256, 0, s, hist_counts(d_hist), hist_units(d_hist), flags, d_px, N, thr, d_units, bt);
    else
        hipLaunchKernelGGL((k_hist_add<CH, WORDS, false>), blocks, 256, 0, s, hist_counts(d_hist), (ull *)nullptr, flags, d_px, N, thr, d_units, bt);
}

void launch_hist_add(ull *d_hist, bool weighted, const unsigned char *d_px, int channels, int alpha_thr, size_t N, const ull *d_units,
                     hipStream_t s) {
    if (N == 0) return;
    if (!d_hist || !d_px || (channels != 3 && channels != 4) || (alpha_thr >= 0 && channels != 4) || alpha_thr > 255 || weighted != (d_units != nullptr))
        throw HipError("patolette_amd: the histogram add needs a table, pixels of 3 or 4 channels and units exactly for a weighted table");
    const size_t tiles = ceil_div(N, kHistTile);
    // tiles per block: as many as leave every CU four blocks, at most kHistBlockTiles (fewer flushes, longer lane runs)
    const unsigned bt = (unsigned)std::max<size_t>(1, std::min<size_t>(kHistBlockTiles, tiles / ((size_t)num_cus() * 4)));
    const size_t blocks = ceil_div(tiles, bt);
    if (blocks >> 31) throw HipError("patolette_amd: the histogram add: too many pixels for one launch");
    const bool words = ((uintptr_t)d_px & 3u) == 0;
    const int thr = alpha_thr < 0 ? 0 : alpha_thr;                       // (no alpha is below 0)
    KTIME("k_hist_add", s, ((double)channels + (weighted ? 8.0 : 0.0)) * N);
    if (channels == 3) {
        if (words) hist_add_typed<3, true>(d_hist, weighted, (unsigned)blocks, d_px, N, thr, d_units, bt, s);
        else hist_add_typed<3, false>(d_hist, weighted, (unsigned)blocks, d_px, N, thr, d_units, bt, s);
    } else {
        if (words) hist_add_typed<4, true>(d_hist, weighted, (unsigned)blocks, d_px, N, thr, d_units, bt, s);
        else hist_add_typed<4, false>(d_hist, weighted, (unsigned)blocks, d_px, N, thr, d_units, bt, s);
    }
    HIP_CHECK(hipGetLastError());
}

void launch_hist_merge(ull *d_hist, const ull *d_other, bool weighted, hipStream_t s) {
    KTIME("k_hist_merge", s, (weighted ? 48.0 : 24.0) * kHistBins);
    hipLaunchKernelGGL(k_hist_merge, (unsigned)num_cus() * 16, 256, 0, s, hist_counts(d_hist), hist_counts(d_other),
                       weighted ? hist_units(d_hist) : (ull *)nullptr, weighted ? hist_units(d_other) : (const ull *)nullptr,
                       reinterpret_cast<unsigned *>(d_hist));
    HIP_CHECK(hipGetLastError());
}

void launch_hist_totals(const ull *d_hist, ull *d_out, hipStream_t s) {
    HIP_CHECK(hipMemsetAsync(d_out, 0, 2 * sizeof(ull), s));
    KTIME("k_hist_totals", s, 8.0 * kHistBins);
    hipLaunchKernelGGL(k_hist_totals, (unsigned)num_cus() * 16, 256, 0, s, hist_counts(d_hist), d_out);
    HIP_CHECK(hipGetLastError());
}

template <class F>
static void hist_export_op(const ull *d_hist, bool weighted, bool positive, unsigned char *d_rgb, ull *d_counts, double *d_w, F &&go) {
    const ull *c = hist_counts(d_hist), *u = weighted ? hist_units(d_hist) : nullptr;
    if (weighted && positive) go(HistExportOp<true, true>{c, u, d_rgb, d_counts, d_w});
    else if (weighted) go(HistExportOp<true, false>{c, u, d_rgb, d_counts, d_w});
    else go(HistExportOp<false, false>{c, u, d_rgb, d_counts, d_w});    // (a count is a weight > 0 already)
}

void launch_hist_export_count(const ull *d_hist, bool weighted, bool positive, unsigned *d_tiles, unsigned *d_total, hipStream_t s) {
    hist_export_op(d_hist, weighted, positive, nullptr, nullptr, nullptr, [&](auto op) {
        launch_compact_count(op, kHistBins, d_tiles, d_total, s, "k_hist_export_count", (weighted ? 16.0 : 8.0) * kHistBins);
    });
}

void launch_hist_export_write(const ull *d_hist, bool weighted, bool positive, const unsigned *d_tiles, unsigned char *d_rgb, ull *d_counts,
                              double *d_w, hipStream_t s) {
    hist_export_op(d_hist, weighted, positive, d_rgb, d_counts, d_w, [&](auto op) {
        launch_compact_write(op, kHistBins, d_tiles, s, "k_hist_export_write", (weighted ? 16.0 : 8.0) * kHistBins);
    });
}

}  // namespace pamd
