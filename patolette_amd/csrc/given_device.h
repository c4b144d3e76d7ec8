// given_device.h -- device-side rules shared by the kernels over maps the caller gives (delta.hip, measure.hip): each rule once.
//   LossyLds   a source pixel's squared ICtCp distance to a palette row, and the LDS state it needs
//   fold_box   a lane's box maxima and count into the block's five LDS cells
//   publish_box   the block's cells into a frame's slot in global memory
// Boxes are kept as maxima over zeroed memory (width - x0, height - y0, x1 + 1, y1 + 1): the union of two boxes is the element-wise
// maximum, an empty one is all zero.  Integers only, so no box or count depends on the order of the atomics.
// The including translation unit defines PAMD_POW_TABLES_IN_LDS first (color_device.h).
#pragma once

#include "color_device.h"

#ifndef PAMD_POW_TABLES_IN_LDS
#error "given_device.h: define PAMD_POW_TABLES_IN_LDS before the first include of color_device.h"
#endif

namespace pamd {

// The lossy compare of the frame deltas and the ICtCp part of measure.  The route is the byte route of the nearest maps: the
// companding (sRGB.c:70-89) of every byte value from a 256-entry table in LDS, as k_nn_map_u8 holds it, then dev_convert_linear with
// the pow tables in LDS; the palette (ICtCp, planar (rows,3) f64 at `pal`) is read by index -- a lookup, not a search -- from LDS
// while it has at most Chunk rows (8 Chunk bytes a plane), from global memory beyond.
// On and off: a kernel instantiation that calls neither function (behind `if constexpr`) holds neither array.
// The arrays are two LDS variables, not two members of one __shared__ object: the compiler places a kernel's LDS variables by size,
// the pow tables among them, and the one object (another place for the companding table, or the arrays reached through `this`) took
// k_frame_deltas<unsigned, lossy, 4> from 128 VGPRs to 129 .. 131 and so from four wavefronts per SIMD to three.
template <int Chunk>
struct LossyLds {
    static __device__ __forceinline__ double (&pal3())[3][Chunk] { __shared__ double s_pal[3][Chunk]; return s_pal; }
    static __device__ __forceinline__ double (&glut())[256] { __shared__ double s_glut[256]; return s_glut; }

    // By all 256 threads of the block.  One barrier inside (the pow tables, which the companding table is made with) and NONE at the
    // end: the kernel's next __syncthreads() publishes the two arrays.
    static __device__ __forceinline__ void fill(const double *pal, unsigned rows) {
        const unsigned tid = threadIdx.x;
        pow_tables_to_lds();
        __syncthreads();
        glut()[tid] = dc::gamma_decode((double)tid / 255.0);
        if (rows <= (unsigned)Chunk)
            for (unsigned j = tid; j < rows; j += 256) { pal3()[0][j] = pal[j]; pal3()[1][j] = pal[(size_t)rows + j]; pal3()[2][j] = pal[2 * (size_t)rows + j]; }
    }
    // |ICtCp(b[0], b[1], b[2]) - row `row`|^2, row < rows, associated as (d0*d0 + d1*d1) + d2*d2 (-ffp-contract=off: the bits follow).
    // b: the pixel's bytes where they lie (each is read next to its table look-up) or three values already in registers.  The row
    // is read through one pointer per plane, chosen before the read.  Both are what the kernels compiled to before they shared this
    // function; with the bytes read ahead of the call and a load in either branch k_frame_deltas<unsigned char, lossy, 1> measured
    // 1.5 % slower on 64 frames of 640 x 360 (0.389 against 0.385 ms, three alternating runs each).
    template <typename Bytes>
    static __device__ __forceinline__ double dist2(unsigned row, const Bytes &b, const double *pal, unsigned rows) {
        double v[3] = {glut()[b[0]], glut()[b[1]], glut()[b[2]]};
        dev_convert_linear<PAMD_SRGB_TO_ICTCP>(v);
        const double *r0, *r1, *r2;
        if (rows <= (unsigned)Chunk) { r0 = &pal3()[0][row]; r1 = &pal3()[1][row]; r2 = &pal3()[2][row]; }
        else { r0 = pal + row; r1 = pal + (size_t)rows + row; r2 = pal + 2 * (size_t)rows + row; }
        const double d0 = v[0] - *r0, d1 = v[1] - *r1, d2 = v[2] - *r2;
        return (d0 * d0 + d1 * d1) + d2 * d2;
    }
};

// A lane's maxima v and count into the block's s_acc[5] (zeroed, and a barrier since): shuffles, then one set of LDS atomics per
// wavefront that has something.  `some`: this lane has.
__device__ __forceinline__ void fold_box(unsigned (&v)[4], unsigned cnt, bool some, unsigned *s_acc) {
    if (!__ballot(some)) return;                                 // (wavefront-uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = max(v[j], (unsigned)__shfl_xor((int)v[j], o));
        cnt += (unsigned)__shfl_xor((int)cnt, o);
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) atomicMax(&s_acc[j], v[j]);
        atomicAdd(&s_acc[4], cnt);
    }
}

// Thread 0 publishes the block's s_acc (fold_box by every wavefront, and a barrier since) into cell `cell` of `words`: the box with
// four integer maxima at 16 bytes a cell, the count added to words[count_base + cell] -- kNoCount: the box alone.  A block that
// counted nothing touches no global memory.
constexpr size_t kNoCount = ~(size_t)0;
__device__ __forceinline__ void publish_box(unsigned long long *words, size_t cell, size_t count_base, const unsigned *s_acc) {
    if (threadIdx.x != 0 || s_acc[4] == 0) return;
    unsigned *box = reinterpret_cast<unsigned *>(words) + cell * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) atomicMax(box + j, s_acc[j]);
    if (count_base != kNoCount) atomicAdd(words + count_base + cell, (unsigned long long)s_acc[4]);
}

}  // namespace pamd
