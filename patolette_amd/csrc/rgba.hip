// rgba.hip -- the kernels of the RGBA entry (patolette_amd_rgba): alpha compaction and map expansion (gfx950).
//
// A pixel is transparent iff its alpha byte is below the threshold.  The compaction (compact.h: count, scan, write) hands the
// pipeline the opaque pixels in row-scan order -- the image the reference would be given as an (M, 3) list -- and every pixel's
// compact number (-1 for a transparent one) for the masked dither and the expansion.  The expansion writes the full index map
// (0 = the transparent entry, 1 + the compact choice otherwise) and the RGBA image in one pass.  All three move bytes only.
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

}  // namespace pamd
