// measure.hip -- what a map costs, per palette entry and per frame, on gfx950: include/patolette_amd.h, patolette_amd_measure.
//
// Every position is read once (element + pixel bytes) and enters at most two places: its palette entry and its frame.
// The partition is fixed by the sizes alone (measure.h): a block takes one tile of one frame, a lane the tile's positions
// tid, tid + 256, ... in ascending order, so every load instruction of a wavefront covers 64 consecutive positions.
// Per entry, integers only: count, sse and max_se go into the block's LDS cells with integer atomics (32-bit add, 64-bit add, 32-bit
// max).  A row's cell exists in as many copies as the chunk holds (up to eight) and a lane uses copy lane % copies, so that the lanes
// of one instruction that name one row queue at several addresses.  The block then flushes its non-zero rows, copies summed, with one
// set of global integer atomics each, into the slot its number selects (measure_slots: blocks do not meet on one address).  Beyond
// kMeasureChunk rows the cells are the global ones from the start.
// Per frame: a lane keeps its own count, sse, maximum and -- with the ICtCp part -- the sum of its D's (added in ascending position
// order) and their maximum in registers.  Lanes are combined by the xor butterfly (both partners add the same two values: one
// result), wavefronts through four LDS cells as (w0 + w1) + (w2 + w3), and the tile's record leaves with a plain vector store.
// k_measure_fold folds a frame's records: thread t adds records t, t + 256, ... in ascending order, then a halving tree.  No
// floating-point atomic in this file: d_sum is a function of the arguments alone.
// The ICtCp part is the lossy compare of the frame deltas (given_device.h, LossyLds), over kMeasureChunk rows.
#include "measure.h"

#define PAMD_POW_TABLES_IN_LDS
#include "given_device.h"

namespace pamd {

template <typename ElemT, bool WithD>
__global__ __launch_bounds__(256) void k_measure(const ElemT *__restrict__ maps, const unsigned char *__restrict__ px, int ch, size_t n,
                                                 unsigned tiles_per_frame, unsigned tile, unsigned rows, bool skip_on, unsigned skip,
                                                 const unsigned *__restrict__ p8, const double *__restrict__ pal /* planar (rows,3), ICtCp */,
                                                 unsigned slots, unsigned copies_log2, unsigned long long *e_sse, unsigned *e_cm, MeasureTile *tiles, unsigned *flag) {
    constexpr int C = kMeasureChunk;
    __shared__ unsigned long long s_sse[C];
    __shared__ unsigned s_cnt[C], s_max[C], s_p8[C];
    __shared__ unsigned long long s_fsse;
    __shared__ unsigned s_fcnt, s_fmax;
    __shared__ double s_wsum[4], s_wmax[4];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const bool resident = rows <= (unsigned)C;
    if constexpr (WithD) LossyLds<C>::fill(pal, rows);          // (the barrier below publishes it)
    // a row's cell exists 2^copies_log2 times (measure_copies_log2: as many as the chunk holds), a lane takes copy lane % copies: the
    // lanes of one LDS atomic that name one row -- most of a wavefront on a smooth image -- then queue at that many addresses, not one
    const unsigned copy = lane & ((1u << copies_log2) - 1u);
    if (resident) {
        for (unsigned j = tid; j < (rows << copies_log2); j += 256) { s_sse[j] = 0; s_cnt[j] = 0; s_max[j] = 0; }
        for (unsigned j = tid; j < rows; j += 256) s_p8[j] = p8[j];
    }
    if (tid == 0) { s_fsse = 0; s_fcnt = 0; s_fmax = 0; }
    __syncthreads();
    const size_t f = blockIdx.x / tiles_per_frame;
    const size_t p0 = (size_t)(blockIdx.x % tiles_per_frame) * tile, p1 = p0 + tile < n ? p0 + tile : n;
    const size_t base = f * n, slot_base = (size_t)(blockIdx.x % slots) * rows;
    unsigned cnt = 0, mx = 0;
    unsigned long long sse = 0;
    double ds = 0.0, dm = 0.0;
    bool bad = false;
    for (size_t p = p0 + tid; p < p1; p += 256) {
        const unsigned a = maps[base + p];
        if (skip_on && a == skip) continue;
        if (a >= rows) { bad = true; continue; }                 // (an element that is no row is never an address: `bad` fails the call)
        const unsigned char *q = px + (base + p) * (size_t)ch;
        const unsigned b0 = q[0], b1 = q[1], b2 = q[2], b[3] = {b0, b1, b2};
        const unsigned row = resident ? s_p8[a] : p8[a];
        const int e0 = (int)b0 - (int)(row & 255u), e1 = (int)b1 - (int)((row >> 8) & 255u), e2 = (int)b2 - (int)((row >> 16) & 255u);
        const unsigned e = (unsigned)(e0 * e0 + e1 * e1 + e2 * e2);
        cnt++; sse += e; mx = max(mx, e);
        if (resident) {
            const unsigned c = (a << copies_log2) | copy;
            atomicAdd(&s_cnt[c], 1u);
            atomicAdd(&s_sse[c], (unsigned long long)e);
            atomicMax(&s_max[c], e);
        } else {
            const size_t cell = slot_base + a;
            atomicAdd(e_cm + 2 * cell, 1u);
            atomicMax(e_cm + 2 * cell + 1, e);
            atomicAdd(e_sse + cell, (unsigned long long)e);
        }
        if constexpr (WithD) {
            const double d = LossyLds<C>::dist2(a, b, pal, rows);
            ds += d;
            dm = d > dm ? d : dm;
        }
    }
    // the frame's part: lanes by the butterfly, wavefronts through LDS
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += (unsigned)__shfl_xor((int)cnt, o);
        sse += __shfl_xor(sse, o);
        mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
        if constexpr (WithD) {
            ds = ds + __shfl_xor(ds, o);
            const double other = __shfl_xor(dm, o);
            dm = other > dm ? other : dm;
        }
    }
    if (lane == 0) {
        if (cnt) { atomicAdd(&s_fcnt, cnt); atomicAdd(&s_fsse, sse); atomicMax(&s_fmax, mx); }
        s_wsum[tid >> 6] = ds; s_wmax[tid >> 6] = dm;
    }
    if (__ballot(bad) && lane == 0) atomicOr(flag, 1u);
    __syncthreads();
    if (resident)
        for (unsigned j = tid; j < rows; j += 256) {
            unsigned c = 0, m = 0;
            unsigned long long q = 0;
            for (unsigned r = 0; r < (1u << copies_log2); r++) {
                const unsigned at = (j << copies_log2) + r;
                c += s_cnt[at]; q += s_sse[at]; m = max(m, s_max[at]);
            }
            if (c == 0) continue;                                // only the rows this tile touched
            const size_t cell = slot_base + j;
            atomicAdd(e_cm + 2 * cell, c);
            atomicAdd(e_sse + cell, q);
            if (m) atomicMax(e_cm + 2 * cell + 1, m);
        }
    if (tid == 0) {
        MeasureTile t;
        t.sse = s_fsse; t.count = s_fcnt; t.max_se = s_fmax;
        t.d_sum = (s_wsum[0] + s_wsum[1]) + (s_wsum[2] + s_wsum[3]);
        t.d_max = fmax(fmax(s_wmax[0], s_wmax[1]), fmax(s_wmax[2], s_wmax[3]));
        tiles[blockIdx.x] = t;
    }
}

// Blocks 0 .. frames-1: a frame's tile records into its five words -- thread t takes records t, t + 256, ... in ascending order, then
// a halving tree over the 256 threads (a fixed pattern: the same bits whatever ran before).  The blocks after them: 256 rows each,
// every row's slots summed in ascending order (integers).  `out`: the words behind the flag (measure.h).
__global__ __launch_bounds__(256) void k_measure_fold(const MeasureTile *__restrict__ tiles, unsigned frames, unsigned tiles_per_frame,
                                                      unsigned rows, unsigned slots, const unsigned long long *__restrict__ e_sse,
                                                      const unsigned *__restrict__ e_cm, unsigned long long *out) {
    __shared__ unsigned long long s_cnt[256], s_sse[256];
    __shared__ unsigned s_max[256];
    __shared__ double s_dsum[256], s_dmax[256];
    const unsigned tid = threadIdx.x;
    if (blockIdx.x >= frames) {
        const size_t r = (size_t)(blockIdx.x - frames) * 256 + tid;
        if (r >= rows) return;
        unsigned long long cnt = 0, sse = 0;
        unsigned mx = 0;
        for (unsigned s = 0; s < slots; s++) {
            const size_t cell = (size_t)s * rows + r;
            cnt += e_cm[2 * cell]; mx = max(mx, e_cm[2 * cell + 1]); sse += e_sse[cell];
        }
        out[3 * r] = cnt; out[3 * r + 1] = sse; out[3 * r + 2] = mx;
        return;
    }
    const MeasureTile *mine = tiles + (size_t)blockIdx.x * tiles_per_frame;
    unsigned long long cnt = 0, sse = 0;
    unsigned mx = 0;
    double ds = 0.0, dm = 0.0;
    for (unsigned i = tid; i < tiles_per_frame; i += 256) {
        const MeasureTile t = mine[i];
        cnt += t.count; sse += t.sse; mx = max(mx, t.max_se);
        ds += t.d_sum;
        dm = t.d_max > dm ? t.d_max : dm;
    }
    s_cnt[tid] = cnt; s_sse[tid] = sse; s_max[tid] = mx; s_dsum[tid] = ds; s_dmax[tid] = dm;
    for (unsigned o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) {
            s_cnt[tid] += s_cnt[tid + o]; s_sse[tid] += s_sse[tid + o]; s_max[tid] = max(s_max[tid], s_max[tid + o]);
            s_dsum[tid] = s_dsum[tid] + s_dsum[tid + o];
            s_dmax[tid] = s_dmax[tid + o] > s_dmax[tid] ? s_dmax[tid + o] : s_dmax[tid];
        }
    }
    if (tid == 0) {
        unsigned long long *o5 = out + 3 * (size_t)rows + 5 * (size_t)blockIdx.x;
        o5[0] = s_cnt[0]; o5[1] = s_sse[0]; o5[2] = s_max[0];
        o5[3] = (unsigned long long)__double_as_longlong(s_dsum[0]); o5[4] = (unsigned long long)__double_as_longlong(s_dmax[0]);
    }
}

template <typename ElemT>
static void launch_typed(const void *d_maps, unsigned blocks, size_t n, unsigned tpf, unsigned tile, const unsigned char *d_px, int channels,
                         unsigned rows, bool skip_on, unsigned skip, const unsigned *d_p8, const double *d_pal, unsigned slots,
                         unsigned long long *e_sse, unsigned *e_cm, MeasureTile *d_tiles, unsigned *d_flag, hipStream_t s) {
    if (d_pal)
        hipLaunchKernelGGL((k_measure<ElemT, true>), blocks, 256, 0, s, (const ElemT *)d_maps, d_px, channels, n, tpf, tile, rows, skip_on, skip, d_p8,
                           d_pal, slots, measure_copies_log2(rows), e_sse, e_cm, d_tiles, d_flag);
    else
        hipLaunchKernelGGL((k_measure<ElemT, false>), blocks, 256, 0, s, (const ElemT *)d_maps, d_px, channels, n, tpf, tile, rows, skip_on, skip, d_p8,
                           d_pal, slots, measure_copies_log2(rows), e_sse, e_cm, d_tiles, d_flag);
}

void launch_measure(const void *d_maps, int elem_bytes, size_t frames, size_t n, const unsigned char *d_px, int channels, size_t rows,
                    bool skip_on, unsigned skip, const unsigned *d_p8, const double *d_pal, unsigned long long *d_words,
                    MeasureTile *d_tiles, hipStream_t s) {
    const size_t N = frames * n;
    if (N == 0) return;
    if (elem_bytes != 1 && elem_bytes != 4) throw HipError("patolette_amd: measure takes elements of 1 or 4 bytes");
    if (!d_maps || !d_px || !d_p8 || rows < 1) throw HipError("patolette_amd: measure needs maps, pixels and a palette");
    const size_t tile = measure_tile(n), tpf = measure_tiles_per_frame(n), fold_blocks = frames + ceil_div(rows, 256);
    if (rows >> 32 || frames >> 31 || (frames * tpf) >> 31 || fold_blocks >> 31)
        throw HipError("patolette_amd: measure: a size does not fit the kernels' 32-bit fields");
    const unsigned slots = measure_slots(rows);
    const size_t flag_word = measure_flag_word(rows);
    HIP_CHECK(hipMemsetAsync(d_words, 0, (flag_word + 1) * sizeof(unsigned long long), s));
    unsigned long long *e_sse = d_words;
    unsigned *e_cm = reinterpret_cast<unsigned *>(d_words + (size_t)slots * rows);
    unsigned *d_flag = reinterpret_cast<unsigned *>(d_words + flag_word);
    {
        KTIME("k_measure", s, ((double)elem_bytes + channels) * N);
        if (elem_bytes == 1)
            launch_typed<unsigned char>(d_maps, (unsigned)(frames * tpf), n, (unsigned)tpf, (unsigned)tile, d_px, channels, (unsigned)rows, skip_on, skip,
                                        d_p8, d_pal, slots, e_sse, e_cm, d_tiles, d_flag, s);
        else
            launch_typed<unsigned int>(d_maps, (unsigned)(frames * tpf), n, (unsigned)tpf, (unsigned)tile, d_px, channels, (unsigned)rows, skip_on, skip,
                                       d_p8, d_pal, slots, e_sse, e_cm, d_tiles, d_flag, s);
        HIP_CHECK(hipGetLastError());
    }
    {
        KTIME("k_measure_fold", s, 32.0 * frames * tpf + 16.0 * slots * rows);
        hipLaunchKernelGGL(k_measure_fold, (unsigned)fold_blocks, 256, 0, s, d_tiles, (unsigned)frames, (unsigned)tpf, (unsigned)rows, slots, e_sse,
                           e_cm, d_words + flag_word + 1);
        HIP_CHECK(hipGetLastError());
    }
}

}  // namespace pamd
