// rgba.hip -- the kernels of the RGBA entry (patolette_amd_rgba): alpha compaction and map expansion (gfx950).
//
// A pixel is transparent iff its alpha byte is below the threshold.  The compaction (compact.h: count, scan, write) hands the
// pipeline the opaque pixels in row-scan order -- the image the reference would be given as an (M, 3) list -- and every pixel's
// compact number (-1 for a transparent one) for the masked dither and the expansion.  The expansion writes the full index map
// (0 = the transparent entry, 1 + the compact choice otherwise) and the RGBA image in one pass.  All three move bytes only.
// The remap with alpha (patolette_amd_remap_rgba_u8) adds k_rgba_stamp, at the end of this file: the same two outputs from a map that
// the nearest or the ordered mapper made of every pixel's RGB.
#include "rgba.h"

#include "compact.h"

namespace pamd {

namespace {
struct AlphaCountOp {                    // pass 1: which pixels are opaque
    const unsigned *px;                  // RGBA, one 32-bit word per pixel (R in the low byte)
    unsigned thr;
    using V = unsigned;
    __device__ V load(size_t i) const { return px[i]; }
    __device__ bool keep(V v) const { return (v >> 24) >= thr; }
    __device__ void put(size_t, V, bool, unsigned) const {}
};
struct AlphaWriteOp : AlphaCountOp {     // pass 2: compact number of every pixel, the opaque ones' RGB and weights
    int *cpos;
    unsigned char *rgb;                  // 3 bytes per opaque pixel
    const double *w;                     // nullptr: unweighted
    double *wc;
    __device__ void put(size_t i, V v, bool k, unsigned r) const {
        cpos[i] = k ? (int)r : -1;
        if (k) {
            unsigned char *o = rgb + 3 * (size_t)r;
            o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16);
            if (w) wc[r] = w[i];
        }
    }
};
}  // namespace

void launch_alpha_count(const unsigned char *d_rgba, size_t n, int thr, unsigned *d_counts, unsigned *d_total, hipStream_t s) {
    const AlphaCountOp op{(const unsigned *)d_rgba, (unsigned)thr};
    launch_compact_count(op, n, d_counts, d_total, s, "k_alpha_count", 4.0 * n);
}

void launch_alpha_compact(const unsigned char *d_rgba, size_t n, size_t m, int thr, const unsigned *d_offsets, const double *d_w, int *d_cpos,
                          unsigned char *d_rgb, double *d_wc, hipStream_t s) {
    AlphaWriteOp op{};
    op.px = (const unsigned *)d_rgba; op.thr = (unsigned)thr;
    op.cpos = d_cpos; op.rgb = d_rgb; op.w = d_w; op.wc = d_wc;
    launch_compact_write(op, n, d_offsets, s, "k_alpha_compact", 8.0 * n + 3.0 * m + (d_w ? 16.0 * m : 0.0));
}

// map[i] = off + cmap[cpos[i]] (0 where cpos[i] < 0; cpos null: the identity), quant[i] = pal[map[i]]; a grid-stride loop, the
// palette (one RGBA word per entry) in LDS when it fits
template <typename InT, typename OutT, bool LDS>
__global__ __launch_bounds__(256) void k_rgba_expand(const InT *__restrict__ cmap, const int *__restrict__ cpos, size_t n, unsigned off,
                                                     const unsigned *__restrict__ pal, int k, OutT *__restrict__ map, unsigned *__restrict__ quant) {
    extern __shared__ unsigned spal[];
    if constexpr (LDS) {
        for (int j = threadIdx.x; j < k; j += blockDim.x) spal[j] = pal[j];
        __syncthreads();
    }
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        unsigned v;
        if (cpos) { const int c = cpos[i]; v = c < 0 ? 0u : off + (unsigned)cmap[c]; }
        else v = off + (unsigned)cmap[i];
        if (map) map[i] = (OutT)v;
        if (quant) {
            if constexpr (LDS) quant[i] = spal[v];
            else quant[i] = pal[v];
        }
    }
}

template <typename InT, typename OutT>
static void expand_t(const void *cmap, const int *cpos, size_t n, unsigned off, const unsigned *pal, int k, void *map, unsigned *quant,
                     hipStream_t s) {
    size_t b = ceil_div(n, 256);
    if (b > 256 * 16) b = 256 * 16;                                  // 256 CUs x 16 blocks, grid-stride the rest
    if (b < 1) b = 1;
    if (k <= 4096) hipLaunchKernelGGL((k_rgba_expand<InT, OutT, true>), (unsigned)b, 256, (size_t)k * 4, s, (const InT *)cmap, cpos, n, off, pal, k, (OutT *)map, quant);
    else hipLaunchKernelGGL((k_rgba_expand<InT, OutT, false>), (unsigned)b, 256, 0, s, (const InT *)cmap, cpos, n, off, pal, k, (OutT *)map, quant);
}

void launch_rgba_expand(const void *d_cmap, int cmap_elem, const int *d_cpos, size_t n, size_t m, unsigned off, const unsigned char *d_pal_rgba,
                        int k, void *d_map, int map_elem, unsigned char *d_quant, hipStream_t s) {
    KTIME("k_rgba_expand", s, (d_cpos ? 4.0 * n : 0.0) + (double)cmap_elem * m + (d_map ? (double)map_elem * n : 0.0) + (d_quant ? 4.0 * n : 0.0));
    const unsigned *pal = (const unsigned *)d_pal_rgba;
    unsigned *q = (unsigned *)d_quant;
    const int me = d_map ? map_elem : 1;
#define PAMD_EXPAND(IN)                                                                                         \
    do {                                                                                                        \
        if (me == 1) expand_t<IN, unsigned char>(d_cmap, d_cpos, n, off, pal, k, d_map, q, s);                  \
        else if (me == 2) expand_t<IN, unsigned short>(d_cmap, d_cpos, n, off, pal, k, d_map, q, s);            \
        else if (me == 4) expand_t<IN, unsigned int>(d_cmap, d_cpos, n, off, pal, k, d_map, q, s);              \
        else expand_t<IN, unsigned long long>(d_cmap, d_cpos, n, off, pal, k, d_map, q, s);                     \
    } while (0)
    if (cmap_elem == 1) PAMD_EXPAND(unsigned char);
    else PAMD_EXPAND(unsigned int);
#undef PAMD_EXPAND
    HIP_CHECK(hipGetLastError());
}

// --------------------------------------------------------------------------------------------
// remap with alpha (patolette_amd_remap_rgba_u8): the stamp behind the nearest and the ordered map
// --------------------------------------------------------------------------------------------
// TESTS ONLY (patolette_amd_debug_rgba_stamp_quad): -1 the rule of launch_rgba_stamp, 0 one pixel per lane, 1 four wherever they can be
static std::atomic<int> g_stamp_quad{-1};
int rgba_stamp_debug_quad(int mode) { return g_stamp_quad.exchange(mode < 0 ? -1 : (mode ? 1 : 0)); }

namespace {
// four consecutive elements as one access
template <typename T> struct Quad;
template <> struct Quad<unsigned char> { using type = uchar4; };
template <> struct Quad<unsigned short> { using type = ushort4; };
template <> struct Quad<unsigned int> { using type = uint4; };
template <> struct Quad<unsigned long long> { using type = ulonglong4; };
}  // namespace

// The mappers ran over every pixel of the stack with the opaque rows alone (cmap[i] = their element for pixel i, RGB bytes only);
// this pass reads the alpha byte and that element and writes what the caller sees: map[i] = off + cmap[i] and quant[i] = that row's
// RGBA word for an opaque pixel, 0 and (0, 0, 0, 0) for a transparent one.  A transparent pixel with off == 0 (no transparent entry)
// raises *flag; its element is not used as an address.  pal: rows words (row 0 the transparent entry's when off == 1), in LDS up to
// kStampRows rows.  V == 4: lane t < N / 4 owns pixels 4t .. 4t + 3 -- one 16-byte pixel load, one 16-byte quantized store, one vector
// access per map -- and the N % 4 pixels behind them go one each to the next lanes.  V == 1: a pixel per lane.  cmap is read only
// where an output wants it; map and quant may be null.
constexpr unsigned kStampRows = 1024;
template <typename InT, typename OutT, int V, bool LDS>
__global__ __launch_bounds__(256) void k_rgba_stamp(const unsigned *__restrict__ px, const InT *__restrict__ cmap, size_t N, unsigned thr,
                                                    unsigned off, const unsigned *__restrict__ pal, unsigned rows, OutT *__restrict__ map,
                                                    unsigned *__restrict__ quant, unsigned *flag) {
    __shared__ unsigned s_pal[LDS ? kStampRows : 1];
    if constexpr (LDS) {
        for (unsigned j = threadIdx.x; j < rows; j += 256) s_pal[j] = pal[j];
        __syncthreads();
    }
    const bool want = map || quant;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t quads = V == 4 ? N / 4 : 0;
    bool bad = false;
    // element and word of one pixel (a: its RGBA word, e: the mapper's element)
    auto one = [&](unsigned a, unsigned e, unsigned &v, unsigned &w) {
        const bool opaque = (a >> 24) >= thr;
        bad |= !opaque && off == 0;
        v = opaque ? off + e : 0u;
        w = 0u;
        if (opaque && quant && v < rows) {                                 // (v < rows always: the mappers choose among rows - off)
            if constexpr (LDS) w = s_pal[v]; else w = pal[v];
        }
    };
    if (V == 4 && t < quads) {
        const uint4 p = reinterpret_cast<const uint4 *>(px)[t];
        const unsigned a[4] = {p.x, p.y, p.z, p.w};
        unsigned e[4] = {0, 0, 0, 0}, v[4], w[4];
        if (want) { const typename Quad<InT>::type q = reinterpret_cast<const typename Quad<InT>::type *>(cmap)[t]; e[0] = q.x; e[1] = q.y; e[2] = q.z; e[3] = q.w; }
#pragma unroll
        for (int j = 0; j < 4; j++) one(a[j], e[j], v[j], w[j]);
        if (map) {
            typename Quad<OutT>::type q;
            q.x = (OutT)v[0]; q.y = (OutT)v[1]; q.z = (OutT)v[2]; q.w = (OutT)v[3];
            reinterpret_cast<typename Quad<OutT>::type *>(map)[t] = q;
        }
        if (quant) reinterpret_cast<uint4 *>(quant)[t] = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        const size_t i = V == 4 ? 4 * quads + (t - quads) : t;
        if (i < N) {
            unsigned v, w;
            one(px[i], want ? (unsigned)cmap[i] : 0u, v, w);
            if (map) map[i] = (OutT)v;
            if (quant) quant[i] = w;
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63u) == 0) atomicOr(flag, 1u);
}

template <typename InT, typename OutT>
static void stamp_t(const unsigned char *px, const void *cmap, size_t N, int thr, unsigned off, const unsigned *pal, size_t rows, void *map,
                    unsigned char *quant, unsigned *flag, bool quad, hipStream_t s) {
    const size_t lanes = quad ? N / 4 + N % 4 : N;
    const size_t blocks = ceil_div(lanes, 256);
    if (blocks >> 31 || rows >> 32) throw HipError("patolette_amd: remap_rgba: a size does not fit the stamp's 32-bit fields");
    const bool lds = rows <= kStampRows;
#define PAMD_STAMP(V, L)                                                                                                               \
    hipLaunchKernelGGL((k_rgba_stamp<InT, OutT, V, L>), (unsigned)blocks, 256, 0, s, (const unsigned *)px, (const InT *)cmap, N, (unsigned)thr, \
                       off, pal, (unsigned)rows, (OutT *)map, (unsigned *)quant, flag)
    if (quad) { if (lds) PAMD_STAMP(4, true); else PAMD_STAMP(4, false); }
    else { if (lds) PAMD_STAMP(1, true); else PAMD_STAMP(1, false); }
#undef PAMD_STAMP
}

void launch_rgba_stamp(const unsigned char *d_rgba, const void *d_cmap, int cmap_elem, size_t n, int thr, unsigned off, const unsigned char *d_pal_rgba,
                       size_t rows, void *d_map, int map_elem, unsigned char *d_quant, unsigned *d_flag, hipStream_t s) {
    if (n == 0) return;
    if (cmap_elem != 1 && cmap_elem != 4) throw HipError("patolette_amd: the stamp reads elements of 1 or 4 bytes");
    const int me = d_map ? map_elem : 1;
    const bool want = d_map || d_quant;
    KTIME("k_rgba_stamp", s, (4.0 + (want ? cmap_elem : 0) + (d_map ? me : 0) + (d_quant ? 4.0 : 0.0)) * n);
    // four pixels per lane wherever every buffer is aligned for its vector access (no size rule: both forms were measured)
    const int mode = g_stamp_quad.load(std::memory_order_relaxed);
    auto fits = [](const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
    const bool can = n >= 4 && fits(d_rgba, 16) && fits(d_cmap, 4 * (size_t)cmap_elem) && fits(d_map, 4 * (size_t)me) && fits(d_quant, 16);
    const bool quad = can && mode != 0;
    const unsigned *pal = (const unsigned *)d_pal_rgba;
#define PAMD_STAMP_OUT(IN)                                                                                                   \
    do {                                                                                                                     \
        if (me == 1) stamp_t<IN, unsigned char>(d_rgba, d_cmap, n, thr, off, pal, rows, d_map, d_quant, d_flag, quad, s);     \
        else if (me == 2) stamp_t<IN, unsigned short>(d_rgba, d_cmap, n, thr, off, pal, rows, d_map, d_quant, d_flag, quad, s); \
        else if (me == 4) stamp_t<IN, unsigned int>(d_rgba, d_cmap, n, thr, off, pal, rows, d_map, d_quant, d_flag, quad, s);  \
        else stamp_t<IN, unsigned long long>(d_rgba, d_cmap, n, thr, off, pal, rows, d_map, d_quant, d_flag, quad, s);        \
    } while (0)
    if (cmap_elem == 1) PAMD_STAMP_OUT(unsigned char);
    else PAMD_STAMP_OUT(unsigned int);
#undef PAMD_STAMP_OUT
    HIP_CHECK(hipGetLastError());
}

}  // namespace pamd
