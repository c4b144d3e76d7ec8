// compact.h -- order-preserving stream compaction on gfx950: which items of [0, n) pass a test, numbered in ascending order.
//
// Three launches: k_compact_count (one count per tile of 4096 items: a __ballot + __popcll per wave and item), k_compact_scan (the
// tile counts into exclusive offsets, one block), k_compact_write (each item's rank = its tile's offset + the items before it in
// the tile: per-wave ballots, a 64-entry scan in LDS).  The item order inside a tile is item j of thread t = j * 256 + t, so the
// loads of one step are consecutive and the ranks follow the item index.  Used by the RGBA entry (rgba.hip: opaque pixels), by
// the masked dither (map.hip: opaque pixels in curve order) and by the colour histogram's export (hist.hip: the bins with a count;
// its V is two 64-bit words, sixteen of which a thread of k_compact_write holds: 73 VGPRs unweighted, 105 weighted).
//
// An operation OP supplies:  using V = ...;  V load(size_t i);  bool keep(V);  void put(size_t i, V, bool keep, unsigned rank).
// put is called for every item of [0, n) (rank is only meaningful when keep).
#pragma once

#include "common.h"

#include <algorithm>

namespace pamd {

constexpr int kCompactItems = 16;                                    // items per thread; 256 threads per block
constexpr size_t kCompactTile = (size_t)256 * kCompactItems;
inline size_t compact_tiles(size_t n) { return ceil_div(n, kCompactTile); }

template <class OP>
__global__ __launch_bounds__(256) void k_compact_count(OP op, size_t n, unsigned *__restrict__ counts) {
    __shared__ unsigned part[4];
    const size_t base = (size_t)blockIdx.x * kCompactTile;
    unsigned c = 0;                                                  // wave-uniform
#pragma unroll
    for (int j = 0; j < kCompactItems; j++) {
        const size_t i = base + (size_t)j * 256 + threadIdx.x;
        const bool k = i < n && op.keep(op.load(i));
        c += (unsigned)__popcll(__ballot(k));
    }
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// counts[0 .. nt) -> exclusive offsets in place; *total = their sum.  One block of 1024 threads, each a contiguous stretch.
// (a template so that every translation unit that launches it has its own instance)
template <int = 0>
__global__ __launch_bounds__(1024) void k_compact_scan(unsigned *__restrict__ counts, size_t nt, unsigned *__restrict__ total) {
    __shared__ unsigned s[1024];
    const unsigned t = threadIdx.x;
    const size_t per = (nt + 1023) / 1024, a = std::min(nt, (size_t)t * per), b = std::min(nt, a + per);
    unsigned sum = 0;
    for (size_t i = a; i < b; i++) sum += counts[i];
    s[t] = sum;
    __syncthreads();
    for (unsigned o = 1; o < 1024; o <<= 1) {                        // inclusive scan over the 1024 stretch sums
        const unsigned y = t >= o ? s[t - o] : 0u;
        __syncthreads();
        s[t] += y;
        __syncthreads();
    }
    unsigned run = s[t] - sum;
    for (size_t i = a; i < b; i++) { const unsigned c = counts[i]; counts[i] = run; run += c; }
    if (t == 1023) *total = s[1023];
}

template <class OP>
__global__ __launch_bounds__(256) void k_compact_write(OP op, size_t n, const unsigned *__restrict__ offs) {
    __shared__ unsigned wc[kCompactItems * 4];                       // [item][wave] counts, then their exclusive prefix
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    const size_t base = (size_t)blockIdx.x * kCompactTile;
    typename OP::V v[kCompactItems];
    bool k[kCompactItems];
    unsigned before[kCompactItems];
#pragma unroll
    for (int j = 0; j < kCompactItems; j++) {
        const size_t i = base + (size_t)j * 256 + threadIdx.x;
        k[j] = false;
        if (i < n) { v[j] = op.load(i); k[j] = op.keep(v[j]); }
        const unsigned long long m = __ballot(k[j]);
        before[j] = (unsigned)__popcll(m & lt);
        if (lane == 0) wc[j * 4 + wv] = (unsigned)__popcll(m);
    }
    __syncthreads();
    if (wv == 0) {                                                   // 64 entries = one wavefront: inclusive scan, then exclusive
        const unsigned x = wc[lane];
        unsigned s = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned y = __shfl_up(s, o, 64); if (lane >= (unsigned)o) s += y; }
        wc[lane] = s - x;
    }
    __syncthreads();
    const unsigned o = offs[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kCompactItems; j++) {
        const size_t i = base + (size_t)j * 256 + threadIdx.x;
        if (i < n) op.put(i, v[j], k[j], o + wc[j * 4 + wv] + before[j]);
    }
}

// count + scan: counts (compact_tiles(n) entries) end as the tiles' offsets, *d_total (device memory) as the number kept.
// n < 2^32 (ranks are 32-bit).
template <class OP>
void launch_compact_count(const OP &op, size_t n, unsigned *counts, unsigned *d_total, hipStream_t s, const char *name, double bytes) {
    if (n >> 32) throw HipError("patolette_amd: the compaction numbers items with 32 bits");
    const size_t nt = compact_tiles(n);
    if (nt == 0) { HIP_CHECK(hipMemsetAsync(d_total, 0, sizeof(unsigned), s)); return; }
    {
        KTIME(name, s, bytes);
        hipLaunchKernelGGL(k_compact_count<OP>, (unsigned)nt, 256, 0, s, op, n, counts);
    }
    hipLaunchKernelGGL(k_compact_scan<0>, 1, 1024, 0, s, counts, nt, d_total);
    HIP_CHECK(hipGetLastError());
}
// ... then the write, with the offsets launch_compact_count left in counts
template <class OP>
void launch_compact_write(const OP &op, size_t n, const unsigned *counts, hipStream_t s, const char *name, double bytes) {
    const size_t nt = compact_tiles(n);
    if (nt == 0) return;
    KTIME(name, s, bytes);
    hipLaunchKernelGGL(k_compact_write<OP>, (unsigned)nt, 256, 0, s, op, n, counts);
    HIP_CHECK(hipGetLastError());
}

}  // namespace pamd
