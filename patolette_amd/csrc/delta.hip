// delta.hip -- frame deltas of an animation's index maps on gfx950: include/patolette_amd.h, patolette_amd_frame_deltas, its RGBA
// flavour (further down) and the one with a colour table per frame (k_frame_deltas_local, between the two).
//
// The step is a chain over frames and independent per position, so a lane owns one position, walks all frames and keeps the canvas
// entry in a register: one launch, no canvas buffer, element bytes x (1 + outputs) of traffic per pixel-frame.  The loads of a
// position's elements do not depend on the decisions: while one group of kDeltaAhead frames is decided the next group's elements are
// already on their way (a small clip gives a CU few wavefronts to hide the latency with).  Where every frame starts on a vector boundary a lane owns four
// consecutive positions and moves them as one 4- or 16-byte access.  delta may be the input buffer: a lane stores a frame's
// elements only after it has loaded them, and no other lane touches those positions.
// Lossy: a lane whose element differs from its canvas entry compares the frame's source pixel with the canvas entry's palette row
// (given_device.h, LossyLds: the conversion, the palette in LDS up to kDeltaChunk rows, the distance).  Lanes that see no
// difference convert nothing; whole frames are not converted ahead.
// Rectangle and count in two stages, integers only (order-free).  The walk leaves one ballot per wavefront and frame -- which of its
// 64 consecutive positions changed: one bit per pixel-frame, a plain vector store by one lane, no barrier and no atomic inside the
// walk.  k_delta_boxes then reads the ballots: a count is a popcount, rows come from the first and the last set bit (positions
// ascend), columns likewise while the 64 positions lie in one row and bit by bit where they wrap; blocks reduce in LDS and reach
// global memory with one set of integer atomics per block, none for a block that saw no change (given_device.h: fold_box, publish_box).
// (First form, measured and replaced: the walk itself reduced every frame -- shuffles, LDS atomics between two barriers per
// kDeltaAhead frames, one set of global atomics per block and frame over kDeltaSlots slots.  64 frames of 640 x 360: 0.091 ms;
// 2 frames of 4096 x 4096: 0.662 ms, where 65 536 blocks met on 160 addresses.  DESIGN.md 4.11 has both.)
#include "delta.h"

#define PAMD_POW_TABLES_IN_LDS
#include "given_device.h"

namespace pamd {

// TESTS ONLY (patolette_amd_debug_delta_quad): -1 the rule of launch_frame_deltas, 0 one position per lane, 1 four wherever they can be
static std::atomic<int> g_delta_quad{-1};
int delta_debug_quad(int mode) { return g_delta_quad.exchange(mode < 0 ? -1 : (mode ? 1 : 0)); }

using DeltaLossy = LossyLds<kDeltaChunk>;   // the lossy compare (given_device.h)
constexpr int kDeltaAhead = 4;       // frames per group: a group's elements are loaded while the group before it is decided

// V consecutive elements as one access (V = 4: a 4- or 16-byte vector)
template <typename ElemT> struct Quad;
template <> struct Quad<unsigned char> { using type = uchar4; };
template <> struct Quad<unsigned int> { using type = uint4; };
template <typename ElemT, int V>
__device__ __forceinline__ void load_elems(const ElemT *at, unsigned (&out)[V]) {
    if constexpr (V == 1) out[0] = at[0];
    else { const typename Quad<ElemT>::type q = *reinterpret_cast<const typename Quad<ElemT>::type *>(at); out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w; }
}
template <typename ElemT, int V>
__device__ __forceinline__ void store_elems(ElemT *at, const unsigned (&in)[V]) {
    if constexpr (V == 1) at[0] = (ElemT)in[0];
    else {
        typename Quad<ElemT>::type q;
        q.x = (ElemT)in[0]; q.y = (ElemT)in[1]; q.z = (ElemT)in[2]; q.w = (ElemT)in[3];
        *reinterpret_cast<typename Quad<ElemT>::type *>(at) = q;
    }
}

// A frame's ballots, by every lane of the wavefront: bit i of word w of `frame_masks` = position 64 w + i changed.  changes: bit j says
// that this lane's position p + j did.
template <int V>
__device__ __forceinline__ void store_ballot(unsigned changes, unsigned lane, size_t p, size_t nw, unsigned long long *frame_masks) {
    if constexpr (V == 1) {
        const unsigned long long moved = __ballot(changes != 0);
        if (lane == 0 && (p >> 6) < nw) frame_masks[p >> 6] = moved;
    } else {                                                     // sixteen lanes hold a word's 64 positions, four bits each
        unsigned long long w = (unsigned long long)changes << (4 * (lane & 15u));
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) w |= __shfl_xor(w, o);
        if ((lane & 15u) == 0 && (p >> 6) < nw) frame_masks[p >> 6] = w;
    }
}

// V: positions a lane owns, consecutive ones.  4 needs n to be a multiple of 4 and buffers aligned for the vector accesses (every
// frame then starts on a vector boundary, and a lane's positions lie all inside the frame or all past its end); launch_frame_deltas
// takes it for large frames only.
template <typename ElemT, bool Lossy, int V>
__global__ __launch_bounds__(256) void k_frame_deltas(const ElemT *maps, size_t F, size_t n, size_t nw, unsigned rows, ElemT T,
                                                      const unsigned char *__restrict__ px, int ch,
                                                      const double *__restrict__ pal /* planar (rows,3), ICtCp */, double tol2,
                                                      ElemT *delta, ElemT *shown, unsigned long long *masks, unsigned *flag) {
    constexpr int A = kDeltaAhead;
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    if constexpr (Lossy) {
        DeltaLossy::fill(pal, rows);
        __syncthreads();
    }
    const size_t p = ((size_t)blockIdx.x * 256 + tid) * V;       // the first of this lane's V positions
    const bool active = p < n;                                   // (a lane past the end stays for the ballots)
    unsigned c[V];                                               // the canvas entries
    bool bad = false;
#pragma unroll
    for (int j = 0; j < V; j++) c[j] = 0;
    if (active) {
        load_elems<ElemT, V>(maps + p, c);
#pragma unroll
        for (int j = 0; j < V; j++) bad |= c[j] >= rows;
        if (delta) store_elems<ElemT, V>(delta + p, c);
        if (shown) store_elems<ElemT, V>(shown + p, c);
    }
    unsigned a[A][V], b[A][V];
#pragma unroll
    for (int u = 0; u < A; u++) {
#pragma unroll
        for (int j = 0; j < V; j++) a[u][j] = 0;
        if (active && 1 + u < F) load_elems<ElemT, V>(maps + (1 + u) * n + p, a[u]);
    }
    for (size_t f = 1; f < F; f += A) {
#pragma unroll
        for (int u = 0; u < A; u++) {
#pragma unroll
            for (int j = 0; j < V; j++) b[u][j] = 0;
            if (active && f + A + u < F) load_elems<ElemT, V>(maps + (f + A + u) * n + p, b[u]);
        }
#pragma unroll
        for (int u = 0; u < A; u++) {
            if (f + u >= F) break;                               // (the same for every lane)
            const size_t at = (f + u) * n + p;
            unsigned out[V], changes = 0;                        // bit j: this lane's position p + j changed
#pragma unroll
            for (int j = 0; j < V; j++) {
                bool change = active && a[u][j] != c[j];
                bad |= active && a[u][j] >= rows;
                if constexpr (Lossy) {
                    if (change && c[j] < rows) {                 // (an element that is no row is never an address: `bad` fails the call)
                        const unsigned char *q = px + (at + j) * (size_t)ch;
                        if (DeltaLossy::dist2(c[j], q, pal, rows) <= tol2) change = false;   // the canvas entry still serves
                    }
                }
                if (change) { c[j] = a[u][j]; changes |= 1u << j; }
                out[j] = change ? a[u][j] : (unsigned)T;
            }
            if (active) {
                if (delta) store_elems<ElemT, V>(delta + at, out);
                if (shown) store_elems<ElemT, V>(shown + at, c);
            }
            store_ballot<V>(changes, lane, p, nw, masks + (f + u) * nw);
        }
#pragma unroll
        for (int u = 0; u < A; u++)
#pragma unroll
            for (int j = 0; j < V; j++) a[u][j] = b[u][j];
    }
    if (__ballot(bad) && lane == 0) atomicOr(flag, 1u);
}

// The ballots of frames 1 .. F-1 (k_frame_deltas: word w of a frame = positions 64 w .. 64 w + 63) into every frame's box and count.
// A block takes 256 words of one frame; `words` as delta.h lays it out.
__global__ __launch_bounds__(256) void k_delta_boxes(const unsigned long long *__restrict__ masks, size_t F, size_t n, size_t nw, unsigned width,
                                                     unsigned height, size_t blocks_per_frame, unsigned long long *words) {
    __shared__ unsigned s_acc[5];
    const unsigned tid = threadIdx.x;
    if (tid < 5) s_acc[tid] = 0;
    __syncthreads();
    const size_t f = 1 + blockIdx.x / blocks_per_frame, chunk = blockIdx.x % blocks_per_frame;
    const size_t wi = chunk * 256 + tid;
    const unsigned long long m = wi < nw ? masks[f * nw + wi] : 0ull;
    // as maxima over zero: width - x0, height - y0, x1 + 1, y1 + 1
    unsigned v[4] = {0, 0, 0, 0}, cnt = 0;
    if (m) {
        const size_t p0 = wi * 64;
        const int first = __ffsll((long long)m) - 1, last = 63 - __clzll((long long)m);
        unsigned y0, y1, x0, x1;
        if (!(n >> 32)) {                                        // positions fit 32 bits: no 64-bit division
            const unsigned q0 = (unsigned)p0 + first, q1 = (unsigned)p0 + last;
            y0 = q0 / width; y1 = q1 / width; x0 = q0 - y0 * width; x1 = q1 - y1 * width;
        } else {
            y0 = (unsigned)((p0 + first) / width); y1 = (unsigned)((p0 + last) / width);
            x0 = (unsigned)((p0 + first) % width); x1 = (unsigned)((p0 + last) % width);
        }
        if (y0 != y1) {                                          // the 64 positions wrap: columns bit by bit, stepping along the rows
            unsigned x = x0, lo = x0, hi = x0;
            for (int bit = first + 1; bit <= last; bit++) {
                if (++x == width) x = 0;
                if ((m >> bit) & 1ull) { lo = min(lo, x); hi = max(hi, x); }
            }
            x0 = lo; x1 = hi;
        }
        v[0] = width - x0; v[1] = height - y0; v[2] = x1 + 1u; v[3] = y1 + 1u;
        cnt = (unsigned)__popcll(m);
    }
    fold_box(v, cnt, m != 0, s_acc);
    __syncthreads();
    publish_box(words, f * (size_t)kDeltaSlots + chunk % (unsigned)kDeltaSlots, F * (size_t)kDeltaSlots * 2, s_acc);
}

// Four positions per lane (V = 4) where every frame starts on a vector boundary (`all`: the buffers' addresses or-ed) -- and where that
// still leaves every SIMD its eight wavefronts: a quarter of the wavefronts moves 4096 x 4096 in 0.036 ms instead of 0.085, but
// 640 x 360 (225 blocks, fewer than CUs) in 0.056 instead of 0.027.  Both flavours' launchers ask here.
static bool delta_quad(size_t n, uintptr_t all, int elem_bytes) {
    const int mode = g_delta_quad.load(std::memory_order_relaxed);
    return n % 4 == 0 && all % (4 * (uintptr_t)elem_bytes) == 0 && (mode < 0 ? n >= (size_t)num_cus() * 32 * 256 : mode == 1);
}

// The kernels' instantiation for elements of 1 or 4 bytes, one or four positions per lane, exact or lossy: f(ElemT(), V, Lossy), the last
// two as std::integral_constant
template <typename F>
static void delta_dispatch(int elem_bytes, bool quad, bool lossy, F f) {
    auto by_v = [&](auto elem, auto is_lossy) {
        if (quad) f(elem, std::integral_constant<int, 4>{}, is_lossy); else f(elem, std::integral_constant<int, 1>{}, is_lossy);
    };
    auto by_lossy = [&](auto elem) { if (lossy) by_v(elem, std::true_type{}); else by_v(elem, std::false_type{}); };
    if (elem_bytes == 1) by_lossy((unsigned char)0); else by_lossy(0u);
}

void launch_frame_deltas(const void *d_maps, int elem_bytes, size_t frames, size_t width, size_t height, size_t rows, size_t T, bool lossy,
                         const unsigned char *d_px, int channels, const double *d_pal, double tol2, void *d_delta, void *d_shown,
                         unsigned long long *d_masks, unsigned long long *d_words, hipStream_t s) {
    const size_t n = width * height, N = frames * n, nw = ceil_div(n, 64);
    if (N == 0) return;
    if (elem_bytes != 1 && elem_bytes != 4) throw HipError("patolette_amd: the frame deltas take elements of 1 or 4 bytes");
    const size_t box_blocks = ceil_div(nw, 256);
    if (width >> 31 || height >> 31 || rows >> 32 || T >> (8 * elem_bytes) || ceil_div(n, 256) >> 31 || (box_blocks * (frames - 1)) >> 31)
        throw HipError("patolette_amd: frame deltas: a size does not fit the kernels' 32-bit fields");
    if (lossy && (!d_px || !d_pal || rows < 1)) throw HipError("patolette_amd: the lossy frame deltas need pixels and a palette");
    HIP_CHECK(hipMemsetAsync(d_words, 0, frame_deltas_words(frames) * sizeof(unsigned long long), s));
    unsigned *d_flag = reinterpret_cast<unsigned *>(d_words + frames * (size_t)kDeltaSlots * 3);
    {
        const int outs = (d_delta ? 1 : 0) + (d_shown ? 1 : 0);
        KTIME("k_frame_deltas", s, ((double)elem_bytes * (1 + outs) + (lossy ? channels : 0) + 0.125) * N);
        const bool quad = delta_quad(n, (uintptr_t)d_maps | (uintptr_t)d_delta | (uintptr_t)d_shown, elem_bytes);
        delta_dispatch(elem_bytes, quad, lossy, [&](auto elem, auto v, auto is_lossy) {
            using ElemT = decltype(elem);
            constexpr int V = decltype(v)::value;
            hipLaunchKernelGGL((k_frame_deltas<ElemT, decltype(is_lossy)::value, V>), (unsigned)ceil_div(n, (size_t)256 * V), 256, 0, s,
                               (const ElemT *)d_maps, frames, n, nw, (unsigned)rows, (ElemT)T, d_px, channels, d_pal, tol2, (ElemT *)d_delta,
                               (ElemT *)d_shown, d_masks, d_flag);
        });
        HIP_CHECK(hipGetLastError());
    }
    if (frames > 1) {
        KTIME("k_delta_boxes", s, 8.0 * nw * (frames - 1));
        hipLaunchKernelGGL(k_delta_boxes, (unsigned)(box_blocks * (frames - 1)), 256, 0, s, d_masks, frames, n, nw, (unsigned)width, (unsigned)height,
                           box_blocks, d_words);
        HIP_CHECK(hipGetLastError());
    }
}

// --------------------------------------------------------------------------------------------
// Per-frame palettes (include/patolette_amd.h, patolette_amd_frame_deltas_local): frame f's elements index table pof[f] of P tables of
// K rows, so the canvas a lane keeps is a colour -- the row's packed RGB word -- and, for the lossy compare, the number g K + a of the
// row it was drawn from.  k_frame_deltas' walk otherwise: one launch, the next group's elements loaded ahead, one ballot word per
// wavefront and frame, k_delta_boxes behind it.  Every step looks a row's word up: the P K words lie in LDS where launch_frame_deltas_local
// finds that worth a block's fill (Lds), in global memory otherwise -- they are L2-resident, a frame's table mostly L1-resident.
// --------------------------------------------------------------------------------------------
// TESTS ONLY (patolette_amd_debug_delta_local_tables): -1 the rule of launch_frame_deltas_local, 0 global memory, 1 LDS wherever they fit
static std::atomic<int> g_local_tables{-1}, g_local_route{-1};
int delta_debug_local_tables(int mode) { return g_local_tables.exchange(mode < 0 ? -1 : (mode ? 1 : 0)); }
int delta_local_route() { return g_local_route.load(std::memory_order_relaxed); }

// V positions' colour words (r in the low byte) as 3 V interleaved bytes; V == 4: `at` is 4-byte aligned (12 bytes, three words)
template <int V>
__device__ __forceinline__ void store_rgb(unsigned char *at, const unsigned (&c)[V]) {
    if constexpr (V == 1) { at[0] = (unsigned char)c[0]; at[1] = (unsigned char)(c[0] >> 8); at[2] = (unsigned char)(c[0] >> 16); }
    else {
        unsigned *q = reinterpret_cast<unsigned *>(at);
        q[0] = c[0] | c[1] << 24; q[1] = c[1] >> 8 | c[2] << 16; q[2] = c[2] >> 16 | c[3] << 8;
    }
}

// maps, delta: one-byte elements (delta may be maps).  palw: the P K rows' words (given.h, given_row_words), PK = P K of them; pof: the
// frames' tables, each below P (the host has checked them); pal: the P K rows in ICtCp, planar (PK,3).  shown: 3 bytes a position.
// An element that is not below K is never an address: row 0 of its frame's table stands in, and the flag fails the call.
// Lds: PK * 4 bytes of dynamic LDS hold palw.
template <bool Lossy, int V, bool Lds>
__global__ __launch_bounds__(256) void k_frame_deltas_local(const unsigned char *maps, size_t F, size_t n, size_t nw, unsigned K, unsigned PK, unsigned T,
                                                            const int *__restrict__ pof, const unsigned *__restrict__ palw,
                                                            const unsigned char *__restrict__ px, int ch,
                                                            const double *__restrict__ pal /* planar (PK,3), ICtCp */, double tol2,
                                                            unsigned char *delta, unsigned char *shown, unsigned long long *masks, unsigned *flag) {
    extern __shared__ unsigned s_words[];
    constexpr int A = kDeltaAhead;
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    if constexpr (Lds) for (unsigned j = tid; j < PK; j += 256) s_words[j] = palw[j];
    if constexpr (Lossy) DeltaLossy::fill(pal, PK);
    if constexpr (Lds || Lossy) __syncthreads();
    auto row_word = [&](unsigned row) -> unsigned { if constexpr (Lds) return s_words[row]; else return palw[row]; };
    const size_t p = ((size_t)blockIdx.x * 256 + tid) * V;       // the first of this lane's V positions
    const bool active = p < n;                                   // (a lane past the end stays for the ballots)
    unsigned c[V], cr[V];                                        // the canvas: the colour's word, and the row it was drawn from
    bool bad = false;
#pragma unroll
    for (int j = 0; j < V; j++) { c[j] = 0; cr[j] = 0; }
    if (active) {
        unsigned e[V];
        load_elems<unsigned char, V>(maps + p, e);
        const unsigned base = (unsigned)pof[0] * K;
#pragma unroll
        for (int j = 0; j < V; j++) {
            const bool ok = e[j] < K;
            bad |= !ok;
            cr[j] = base + (ok ? e[j] : 0u);
            c[j] = row_word(cr[j]);
        }
        if (delta) store_elems<unsigned char, V>(delta + p, e);
        if (shown) store_rgb<V>(shown + 3 * p, c);
    }
    unsigned a[A][V], b[A][V];
#pragma unroll
    for (int u = 0; u < A; u++) {
#pragma unroll
        for (int j = 0; j < V; j++) a[u][j] = 0;
        if (active && 1 + u < F) load_elems<unsigned char, V>(maps + (1 + u) * n + p, a[u]);
    }
    for (size_t f = 1; f < F; f += A) {
#pragma unroll
        for (int u = 0; u < A; u++) {
#pragma unroll
            for (int j = 0; j < V; j++) b[u][j] = 0;
            if (active && f + A + u < F) load_elems<unsigned char, V>(maps + (f + A + u) * n + p, b[u]);
        }
#pragma unroll
        for (int u = 0; u < A; u++) {
            if (f + u >= F) break;                               // (the same for every lane)
            const size_t at = (f + u) * n + p;
            const unsigned base = (unsigned)pof[f + u] * K;      // (uniform: a scalar load)
            unsigned out[V], changes = 0;                        // bit j: this lane's position p + j changed
#pragma unroll
            for (int j = 0; j < V; j++) {
                const unsigned e = a[u][j];
                const bool ok = e < K;
                bad |= active && !ok;
                const unsigned r = base + (ok ? e : 0u);         // (a lane past the end: row 0 of the table, a valid address)
                const unsigned w = row_word(r);
                bool change = active && w != c[j];
                if constexpr (Lossy) {
                    if (change) {
                        const unsigned char *q = px + (at + j) * (size_t)ch;
                        if (DeltaLossy::dist2(cr[j], q, pal, PK) <= tol2) change = false;    // the canvas colour still serves
                    }
                }
                if (change) { c[j] = w; cr[j] = r; changes |= 1u << j; }
                out[j] = change ? e : T;
            }
            if (active) {
                if (delta) store_elems<unsigned char, V>(delta + at, out);
                if (shown) store_rgb<V>(shown + 3 * at, c);
            }
            store_ballot<V>(changes, lane, p, nw, masks + (f + u) * nw);
        }
#pragma unroll
        for (int u = 0; u < A; u++)
#pragma unroll
            for (int j = 0; j < V; j++) a[u][j] = b[u][j];
    }
    if (__ballot(bad) && lane == 0) atomicOr(flag, 1u);
}

void launch_frame_deltas_local(const unsigned char *d_maps, size_t frames, size_t width, size_t height, size_t K, size_t P, size_t T, bool lossy,
                               const int *d_pof, const unsigned *d_rows, const unsigned char *d_px, int channels, const double *d_pal, double tol2,
                               unsigned char *d_delta, unsigned char *d_shown, unsigned long long *d_masks, unsigned long long *d_words, hipStream_t s) {
    const size_t n = width * height, N = frames * n, nw = ceil_div(n, 64), PK = P * K;
    if (N == 0) return;
    const size_t box_blocks = ceil_div(nw, 256);
    if (width >> 31 || height >> 31 || ceil_div(n, 256) >> 31 || (box_blocks * (frames - 1)) >> 31)
        throw HipError("patolette_amd: frame deltas: a size does not fit the kernels' 32-bit fields");
    if (K < 1 || K > 255 || T < K || T > 255 || P < 1 || P > 65536 || !d_pof || !d_rows)
        throw HipError("patolette_amd: the local frame deltas need 1 .. 65536 tables of 1 .. 255 rows and a free index up to 255");
    if (lossy && (!d_px || !d_pal)) throw HipError("patolette_amd: the lossy frame deltas need pixels and a palette");
    HIP_CHECK(hipMemsetAsync(d_words, 0, frame_deltas_words(frames) * sizeof(unsigned long long), s));
    unsigned *d_flag = reinterpret_cast<unsigned *>(d_words + frames * (size_t)kDeltaSlots * 3);
    {
        // The words in LDS: every block fills all P K of them, so only where that is no more than its lanes load elements anyway
        // (256 a frame) and the block's LDS stays small enough for the SIMDs' eight wavefronts.
        const int mode = g_local_tables.load(std::memory_order_relaxed);
        const bool fits = PK <= (size_t)kLocalLdsRows;
        const bool in_lds = fits && (mode < 0 ? PK <= 256 * frames : mode == 1);
        g_local_route.store(in_lds ? 1 : 0, std::memory_order_relaxed);
        KTIME("k_frame_deltas_local", s, (1.0 + (d_delta ? 1 : 0) + (d_shown ? 3 : 0) + (lossy ? channels : 0) + 0.125) * N);
        const bool quad = delta_quad(n, (uintptr_t)d_maps | (uintptr_t)d_delta | (uintptr_t)d_shown, 1);
        delta_dispatch(1, quad, lossy, [&](auto, auto v, auto is_lossy) {
            constexpr int V = decltype(v)::value;
            auto go = [&](auto lds) {
                constexpr bool Lds = decltype(lds)::value;
                hipLaunchKernelGGL((k_frame_deltas_local<decltype(is_lossy)::value, V, Lds>), (unsigned)ceil_div(n, (size_t)256 * V), 256,
                                   Lds ? PK * sizeof(unsigned) : 0, s, d_maps, frames, n, nw, (unsigned)K, (unsigned)PK, (unsigned)T, d_pof, d_rows, d_px,
                                   channels, d_pal, tol2, d_delta, d_shown, d_masks, d_flag);
            };
            if (in_lds) go(std::true_type{}); else go(std::false_type{});
        });
        HIP_CHECK(hipGetLastError());
    }
    if (frames > 1) {
        KTIME("k_delta_boxes", s, 8.0 * nw * (frames - 1));
        hipLaunchKernelGGL(k_delta_boxes, (unsigned)(box_blocks * (frames - 1)), 256, 0, s, d_masks, frames, n, nw, (unsigned)width, (unsigned)height,
                           box_blocks, d_words);
        HIP_CHECK(hipGetLastError());
    }
}

// --------------------------------------------------------------------------------------------
// RGBA maps (include/patolette_amd.h, patolette_amd_frame_deltas_rgba): index 0 is the transparent entry, 0 in a delta means "leave the
// canvas", and a frame whose successor makes a pixel transparent is disposed to background over a rectangle that covers the pixel.
// That rectangle is a grid-wide result the next frame's decisions need, so the frames are a chain of launches: k_rgba_vanish once for
// every frame's V box (from the maps alone), then k_frame_delta_rgba frame after frame on one stream, each reading the slots its
// predecessor filled.  No host turn in between; the host folds the slots once at the end.
// Boxes as given_device.h keeps them: no result depends on the order of the atomics.
// --------------------------------------------------------------------------------------------
constexpr int kRgbaBlocksPerCu = 8;     // 256 threads each: the 32 wavefronts a CU holds

// column and row of a lane's j-th position, from those of its first one (x0 < width; at most j steps)
__device__ __forceinline__ void step_xy(unsigned x0, unsigned y0, unsigned j, unsigned width, unsigned &x, unsigned &y) {
    x = x0 + j; y = y0;
    while (x >= width) { x -= width; y++; }
}

// Every frame's V: the box of the positions that are opaque in frame f and transparent in its successor (frame 0 after the last one
// with `loop`, none otherwise).  Block b takes 256 * V positions of frame b / blocks_per_frame; every element is also tested against
// `rows` here, once (the flag).  `words` as delta.h lays it out.
template <typename ElemT, int V>
__global__ __launch_bounds__(256) void k_rgba_vanish(const ElemT *__restrict__ maps, size_t F, size_t n, unsigned rows, unsigned width, unsigned height,
                                                     int loop, size_t blocks_per_frame, unsigned long long *words) {
    __shared__ unsigned s_acc[5];
    const unsigned tid = threadIdx.x;
    if (tid < 5) s_acc[tid] = 0;
    __syncthreads();
    const size_t f = blockIdx.x / blocks_per_frame, chunk = blockIdx.x % blocks_per_frame;
    const size_t p = (chunk * 256 + tid) * V;
    const bool has_next = f + 1 < F || loop != 0;
    const size_t g = f + 1 < F ? f + 1 : 0;
    unsigned a[V], b[V], gone = 0;                               // bit j: position p + j vanishes
    bool bad = false;
    if (p < n) {
        load_elems<ElemT, V>(maps + f * n + p, a);
#pragma unroll
        for (int j = 0; j < V; j++) bad |= a[j] >= rows;
        if (has_next) {
            load_elems<ElemT, V>(maps + g * n + p, b);
#pragma unroll
            for (int j = 0; j < V; j++) gone |= (a[j] != 0 && b[j] == 0) ? 1u << j : 0u;
        }
    }
    unsigned v[4] = {0, 0, 0, 0};
    if (gone) {
        const unsigned y0 = (unsigned)p / width, x0 = (unsigned)p - y0 * width;      // (n < 2^32: launch_frame_deltas_rgba)
#pragma unroll
        for (int j = 0; j < V; j++) {
            if (!(gone >> j & 1u)) continue;
            unsigned x, y;
            step_xy(x0, y0, j, width, x, y);
            v[0] = max(v[0], width - x); v[1] = max(v[1], height - y); v[2] = max(v[2], x + 1u); v[3] = max(v[3], y + 1u);
        }
    }
    fold_box(v, gone ? 1u : 0u, gone != 0, s_acc);
    __syncthreads();
    publish_box(words, (F + f) * (size_t)kDeltaSlots + chunk % (unsigned)kDeltaSlots, kNoCount, s_acc);
    if (__ballot(bad) && (tid & 63u) == 0) atomicOr(reinterpret_cast<unsigned *>(words + F * (size_t)kDeltaSlots * 5), 1u);
}

// Frame f of the chain.  m, delta, px: frame f's; canvas_in: what the canvas showed after frame f - 1, before that frame's disposal
// (shown[f - 1], or the one-frame workspace; null for f == 0, where the canvas is empty); canvas_out: shown[f] or the workspace again
// (a lane reads and writes its own positions only).  The predecessor's rectangle and disposal come from its slots and its V slots,
// folded once per block by the first wavefront.
template <typename ElemT, bool Lossy, int V>
__global__ __launch_bounds__(256) void k_frame_delta_rgba(const ElemT *m, const ElemT *canvas_in, ElemT *canvas_out, ElemT *delta, size_t F, size_t f,
                                                          size_t n, size_t tiles, unsigned rows, unsigned width, unsigned height,
                                                          const unsigned char *__restrict__ px, int ch,
                                                          const double *__restrict__ pal /* planar (rows,3), ICtCp */, double tol2,
                                                          unsigned long long *words) {
    __shared__ unsigned s_acc[5], s_prev[5];                     // s_prev: x0, y0, x1, y1 (exclusive) of what frame f - 1 cleared; whether it did
    const unsigned tid = threadIdx.x;
    if (tid < 5) s_acc[tid] = 0;
    if (tid < 64) {
        unsigned r[4] = {0, 0, 0, 0}, vanish = 0;
        if (f > 0) {                                             // lanes 0 .. 31: the slots of C[f - 1]; 32 .. 63: those of V[f - 1]
            const uint4 q = reinterpret_cast<const uint4 *>(words)[((tid < 32 ? 0 : F) + (f - 1)) * (size_t)kDeltaSlots + (tid & 31u)];
            r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w;
            vanish = tid < 32 ? 0u : q.z;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int j = 0; j < 4; j++) r[j] = max(r[j], (unsigned)__shfl_xor((int)r[j], o));
            vanish = max(vanish, (unsigned)__shfl_xor((int)vanish, o));
        }
        if (tid == 0) { s_prev[0] = width - r[0]; s_prev[1] = height - r[1]; s_prev[2] = r[2]; s_prev[3] = r[3]; s_prev[4] = vanish != 0; }
    }
    if constexpr (Lossy) DeltaLossy::fill(pal, rows);
    __syncthreads();                                             // (s_acc, s_prev and what fill left)
    unsigned cnt = 0;
    unsigned v[4] = {0, 0, 0, 0};
    const bool cleared = s_prev[4] != 0;
    const unsigned cx0 = s_prev[0], cy0 = s_prev[1], cx1 = s_prev[2], cy1 = s_prev[3];
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {            // (no barrier inside: lanes past the end just pass)
        const size_t p = (tile * 256 + tid) * V;
        const bool active = p < n;
        unsigned a[V], c[V], out[V];
#pragma unroll
        for (int j = 0; j < V; j++) { a[j] = 0; c[j] = 0; }
        if (active) {
            load_elems<ElemT, V>(m + p, a);
            if (canvas_in) load_elems<ElemT, V>(canvas_in + p, c);
        }
        const unsigned y0 = (unsigned)p / width, x0 = (unsigned)p - y0 * width;      // (n < 2^32: launch_frame_deltas_rgba)
#pragma unroll
        for (int j = 0; j < V; j++) {
            unsigned x, y;
            step_xy(x0, y0, j, width, x, y);
            if (cleared && x >= cx0 && x < cx1 && y >= cy0 && y < cy1) c[j] = 0;
            bool change = false;
            if (a[j] == 0) c[j] = 0;                             // (it is 0 there already: the position lay in V[f - 1], or never showed)
            else if (c[j] == 0) change = true;
            else if (a[j] != c[j]) {
                change = true;
                if constexpr (Lossy) {
                    if (c[j] < rows) {                           // (an element that is no row is never an address: the flag fails the call)
                        const unsigned char *q = px + (p + j) * (size_t)ch;
                        if (DeltaLossy::dist2(c[j], q, pal, rows) <= tol2) change = false;   // the canvas entry still serves
                    }
                }
            }
            if (change) {
                c[j] = a[j]; cnt++;
                v[0] = max(v[0], width - x); v[1] = max(v[1], height - y); v[2] = max(v[2], x + 1u); v[3] = max(v[3], y + 1u);
            }
            out[j] = change ? a[j] : 0u;
        }
        if (active) {
            if (delta) store_elems<ElemT, V>(delta + p, out);
            store_elems<ElemT, V>(canvas_out + p, c);
        }
    }
    fold_box(v, cnt, cnt != 0, s_acc);
    __syncthreads();
    publish_box(words, f * (size_t)kDeltaSlots + blockIdx.x % (unsigned)kDeltaSlots, F * (size_t)kDeltaSlots * 4, s_acc);
}

template <typename ElemT, int V, bool Lossy>
static void launch_rgba_typed(const void *d_maps, size_t frames, size_t width, size_t height, size_t rows, int loop,
                              const unsigned char *d_px, int channels, const double *d_pal, double tol2, void *d_delta, void *d_shown,
                              void *d_canvas, unsigned long long *d_words, hipStream_t s) {
    const size_t n = width * height, blocks = ceil_div(n, (size_t)256 * V);
    const ElemT *maps = (const ElemT *)d_maps;
    // a frame's launch: at most kRgbaBlocksPerCu blocks per CU, each walking its tiles -- one set of atomics per block, and 2 x 4096 x
    // 4096 (16 384 tiles of four positions per lane) then meets on the slots with 2048 blocks instead of 16 384: 0.134 ms per
    // frame became 0.036
    const unsigned grid = (unsigned)std::min(blocks, (size_t)num_cus() * kRgbaBlocksPerCu);
    {
        KTIME("k_rgba_vanish", s, 2.0 * sizeof(ElemT) * n * frames);
        hipLaunchKernelGGL((k_rgba_vanish<ElemT, V>), (unsigned)(blocks * frames), 256, 0, s, maps, frames, n, (unsigned)rows, (unsigned)width,
                           (unsigned)height, loop, blocks, d_words);
        HIP_CHECK(hipGetLastError());
    }
    for (size_t f = 0; f < frames; f++) {
        const ElemT *m = maps + f * n;
        ElemT *delta = d_delta ? (ElemT *)d_delta + f * n : nullptr;
        const ElemT *in = f == 0 ? nullptr : (d_shown ? (const ElemT *)d_shown + (f - 1) * n : (const ElemT *)d_canvas);
        ElemT *out = d_shown ? (ElemT *)d_shown + f * n : (ElemT *)d_canvas;
        const unsigned char *px = Lossy ? d_px + f * n * (size_t)channels : nullptr;
        KTIME("k_frame_delta_rgba", s, ((double)sizeof(ElemT) * (f == 0 ? 2 : 3) + (d_delta ? sizeof(ElemT) : 0) + (Lossy ? channels : 0)) * n);
        hipLaunchKernelGGL((k_frame_delta_rgba<ElemT, Lossy, V>), grid, 256, 0, s, m, in, out, delta, frames, f, n, blocks, (unsigned)rows,
                           (unsigned)width, (unsigned)height, px, channels, d_pal, tol2, d_words);
        HIP_CHECK(hipGetLastError());
    }
}

void launch_frame_deltas_rgba(const void *d_maps, int elem_bytes, size_t frames, size_t width, size_t height, size_t rows, int loop, bool lossy,
                              const unsigned char *d_px, int channels, const double *d_pal, double tol2, void *d_delta, void *d_shown,
                              void *d_canvas, unsigned long long *d_words, hipStream_t s) {
    const size_t n = width * height;
    if (frames * n == 0) return;
    if (elem_bytes != 1 && elem_bytes != 4) throw HipError("patolette_amd: the frame deltas take elements of 1 or 4 bytes");
    if (width >> 31 || height >> 31 || n >> 32 || rows >> 32 || (ceil_div(n, 256) * frames) >> 31)
        throw HipError("patolette_amd: frame deltas: a size does not fit the kernels' 32-bit fields");
    if (lossy && (!d_px || !d_pal || rows < 1)) throw HipError("patolette_amd: the lossy frame deltas need pixels and a palette");
    if (!d_shown && !d_canvas) throw HipError("patolette_amd: the RGBA frame deltas need a canvas");
    HIP_CHECK(hipMemsetAsync(d_words, 0, frame_deltas_rgba_words(frames) * sizeof(unsigned long long), s));
    const bool quad = delta_quad(n, (uintptr_t)d_maps | (uintptr_t)d_delta | (uintptr_t)d_shown | (uintptr_t)d_canvas, elem_bytes);
    delta_dispatch(elem_bytes, quad, lossy, [&](auto elem, auto v, auto is_lossy) {
        launch_rgba_typed<decltype(elem), decltype(v)::value, decltype(is_lossy)::value>(d_maps, frames, width, height, rows, loop, d_px, channels, d_pal,
                                                                                        tol2, d_delta, d_shown, d_canvas, d_words, s);
    });
}

}  // namespace pamd
