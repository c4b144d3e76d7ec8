// ordered.hip -- the ordered (Bayer 8x8) dither map on gfx950: include/patolette_amd.h, patolette_amd_remap_ordered_u8.
//
// One kernel, one pass: a lane takes a pixel's bytes, shifts the three of them by the same position-keyed amount (spread * t, t from
// the 8x8 Bayer index of the pixel's place in its own frame), converts the shifted value sRGB -> ICtCp in registers with the functions
// k_convert uses (the device pow with its tables in LDS), and searches the palette for the nearest row: f64, ((d0^2)+d1^2)+d2^2,
// ascending rows, strict '<' -- k_nn_map's loop.  No f64 image is written and nothing passes from one pixel to another.
//
// The palette sits in LDS as three planar arrays and every lane of a wavefront reads the same row (a broadcast); more than
// kOrderedChunk rows pass through LDS chunk by chunk in ascending order with the running best carried along, which keeps the
// lowest-index rule.  The grid cells and candidate tables of k_nn_map_lut / k_nn_map_mid are not used: they take a pixel's cell
// without a clamp, inside a box that is proven for the 2^24 byte colours only, and a shifted value is not one of them.
// Bound: f64 VALU (k rows x 8 flops + nine pow per pixel); the traffic is channels + sizeof(OutT) bytes per pixel.
#include "ordered.h"

#include <algorithm>

#define PAMD_POW_TABLES_IN_LDS
#include "color_device.h"

namespace pamd {

// the 8x8 Bayer index of (x, y): bit-reversed interleave of x ^ y and y; a permutation of 0..63 over a tile
__device__ __forceinline__ unsigned bayer8(const unsigned x, const unsigned y) {
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) v = (v << 2) | ((((x >> i) ^ (y >> i)) & 1u) << 1) | ((y >> i) & 1u);
    return v;
}

// pixels a lane searches for side by side: every palette row read from LDS serves both (measured at 4096^2 x 256 rows: 2.42 ms
// against 2.59 with one pixel; four: 2.36 at 103 registers, and slower on short palettes)
constexpr int kOrderedPixels = 2;

template <typename OutT>
__global__ __launch_bounds__(256) void k_ordered_map(const unsigned char *__restrict__ px, int ch, size_t N, size_t n, size_t width, double spread,
                                                     const double *__restrict__ pal /* planar (k,3), ICtCp */, int k, OutT *__restrict__ out) {
    constexpr int P = kOrderedPixels;
    __shared__ double sp[3][kOrderedChunk];
    // rows [base, base + m) of the palette into LDS
    auto stage = [&](const int base, const int m) {
        for (int j = threadIdx.x; j < m; j += blockDim.x) {
            sp[0][j] = pal[base + j]; sp[1][j] = pal[(size_t)k + base + j]; sp[2][j] = pal[2 * (size_t)k + base + j];
        }
    };
    pow_tables_to_lds();
    const bool resident = k <= kOrderedChunk;                // the whole palette is staged once
    if (resident) stage(0, k);
    __syncthreads();
    const bool small = !(N >> 32);                           // pixel numbers (and so n and width) fit 32 bits: no 64-bit division
    const size_t stride = (size_t)gridDim.x * blockDim.x;    // a lane's P pixels of a round lie `stride` apart: coalesced either way
    const size_t rounds = (N + P * stride - 1) / (P * stride);   // the same for every lane of the block: the chunk loop holds barriers
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t r = 0; r < rounds; r++, i += P * stride) {
        double c[P][3];
#pragma unroll
        for (int p = 0; p < P; p++) {
            const size_t ip = i + p * stride;
            c[p][0] = c[p][1] = c[p][2] = 0.0;
            if (ip < N) {
                unsigned x, y;                               // the pixel's place in its own frame (only the low three bits matter)
                if (small) { const unsigned f = (unsigned)ip % (unsigned)n; x = f % (unsigned)width; y = f / (unsigned)width; }
                else { const size_t f = ip % n; x = (unsigned)((f % width) & 7); y = (unsigned)((f / width) & 7); }
                const double t = ((double)bayer8(x & 7u, y & 7u) + 0.5) / 64.0 - 0.5;
                const double shift = spread * t;
                const unsigned char *q = px + ip * (size_t)ch;
#pragma unroll
                for (int a = 0; a < 3; a++) c[p][a] = dc::gamma_decode(fmin(fmax((double)q[a] / 255.0 + shift, 0.0), 1.0));
                dev_convert_linear<PAMD_SRGB_TO_ICTCP>(c[p]);
            }
        }
        double bd[P];
        int best[P];
#pragma unroll
        for (int p = 0; p < P; p++) { bd[p] = INFINITY; best[p] = 0; }
        for (int base = 0; base < k; base += kOrderedChunk) {
            const int m = k - base < kOrderedChunk ? k - base : kOrderedChunk;
            if (!resident) { __syncthreads(); stage(base, m); __syncthreads(); }
            if (i < N) {                                     // (a lane's later pixels may lie past the end: searched, not stored)
#pragma unroll 4
                for (int j = 0; j < m; j++) {
                    const double p0 = sp[0][j], p1 = sp[1][j], p2 = sp[2][j];
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        const double d0 = c[p][0] - p0, d1 = c[p][1] - p1, d2 = c[p][2] - p2;
                        const double d = (d0 * d0 + d1 * d1) + d2 * d2;
                        if (d < bd[p]) { bd[p] = d; best[p] = base + j; }
                    }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < P; p++)
            if (i + p * stride < N) out[i + p * stride] = (OutT)best[p];
    }
}

void launch_ordered_map(const unsigned char *d_px, int channels, size_t frames, size_t width, size_t height, double spread, const double *d_pal,
                        int k, void *d_out, int elem_bytes, hipStream_t s) {
    const size_t n = width * height, N = frames * n;
    if (N == 0 || k < 1) return;
    if (elem_bytes != 1 && elem_bytes != 4) throw HipError("patolette_amd: the ordered map writes elements of 1 or 4 bytes");
    // 28 KB of LDS per block: four blocks of four wavefronts per CU are resident together, and each takes the same number of rounds
    const int blocks = (int)std::min<size_t>((size_t)num_cus() * 4, ceil_div(N, 256));
    KTIME("k_ordered_map", s, ((double)channels + elem_bytes) * N);
    if (elem_bytes == 1) hipLaunchKernelGGL(k_ordered_map<unsigned char>, blocks, 256, 0, s, d_px, channels, N, n, width, spread, d_pal, k, (unsigned char *)d_out);
    else hipLaunchKernelGGL(k_ordered_map<unsigned int>, blocks, 256, 0, s, d_px, channels, N, n, width, spread, d_pal, k, (unsigned int *)d_out);
    HIP_CHECK(hipGetLastError());
}

}  // namespace pamd
