// sweep_probe.hip -- what does the fetch and store path of the split sweeps (quant.hip: k_minmax, k_hist, k_count) cost?
//   hipcc --offload-arch=gfx950 -O3 -o tools/probe/sweep_probe tools/probe/sweep_probe.hip
// Replays the sweeps' read of three f64 planes (4096^2 pixels = 403 MB) in 8192-pixel tiles by 256-thread blocks, re-reading
// the same planes launch after launch in alternating tile order (as the sweeps of a split round do), and prints for every
// variant the best of 7 launches in us and the TB/s of plane bytes read.  Variants:
//   B   bytes per lane and load: 8 (one pixel) or 16 (two consecutive pixels)
//   nt  default or non-temporal loads
//   fl  loads in flight per lane before the first is consumed: 6, 12, 24
//   st  side store of 2 bytes per pixel (the bucket ids): none, or 2 / 4 / 16 bytes per storing lane
//   columns: tiles per block (1 = a block per tile, otherwise a run of consecutive tiles) x plane stride
//            (2^27 B = the pixel count, or 2^27 B + 9 * 256 B)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

typedef double d2 __attribute__((ext_vector_type(2)));
constexpr unsigned kTile = 8192;
constexpr size_t kPixels = (size_t)1 << 24;                  // 2048 full tiles
constexpr size_t kPad = 9 * 256 / 8;                         // doubles added to the plane stride

template <bool NT, typename T>
__device__ __forceinline__ T ld(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p); else return *p;
}

// B: bytes per load, FL: loads in flight per lane, ST: bytes per side store (0: none)
template <int B, bool NT, int FL, int ST>
__global__ __launch_bounds__(256) void k_sweep(const double *__restrict__ planes, const size_t stride, unsigned char *__restrict__ side,
                                               const int ntiles, const int per, const int rev, double *out) {
    constexpr int L = FL / 3;                                // loads per plane and trip
    constexpr unsigned PX = 256u * L * (B / 8);              // pixels of a trip
    static_assert(kTile % PX == 0, "a tile is a whole number of trips");
    const double *px = planes, *py = planes + stride, *pz = planes + 2 * stride;
    double acc = 0;
    const int nblk = (int)gridDim.x;
    const int bid = rev ? nblk - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const int tfirst = bid * per, tlast = min(ntiles, tfirst + per);
    for (int ti = tfirst; ti < tlast; ti++) {
        const size_t t0 = (size_t)ti * kTile;
        for (unsigned i = 0; i < kTile; i += PX) {
            double s = 0;
            if constexpr (B == 8) {
                double x[L], y[L], z[L];
#pragma unroll
                for (int u = 0; u < L; u++) {
                    const size_t p = t0 + i + u * 256 + threadIdx.x;
                    x[u] = ld<NT>(px + p); y[u] = ld<NT>(py + p); z[u] = ld<NT>(pz + p);
                }
#pragma unroll
                for (int u = 0; u < L; u++) s += (x[u] + y[u]) + z[u];
            } else {
                d2 x[L], y[L], z[L];
#pragma unroll
                for (int u = 0; u < L; u++) {
                    const size_t p = t0 + i + 2 * (u * 256 + threadIdx.x);
                    x[u] = ld<NT>((const d2 *)(px + p)); y[u] = ld<NT>((const d2 *)(py + p)); z[u] = ld<NT>((const d2 *)(pz + p));
                }
#pragma unroll
                for (int u = 0; u < L; u++) s += ((x[u].x + y[u].x) + z[u].x) + ((x[u].y + y[u].y) + z[u].y);
            }
            acc += s;
            if constexpr (ST > 0) {
                // the trip's 2 * PX bytes of ids, contiguous, ST bytes per lane by the first 2 * PX / ST lanes of the block
                const unsigned v = (unsigned)__double_as_longlong(s);
                constexpr unsigned ns = 2u * PX / ST;          // storing lanes per pass
                unsigned char *dst = side + 2 * (t0 + i);
                for (unsigned k = threadIdx.x; k < ns; k += 256) {
                    if constexpr (ST == 2) ((unsigned short *)dst)[k] = (unsigned short)v;
                    else if constexpr (ST == 4) ((unsigned *)dst)[k] = v;
                    else ((uint4 *)dst)[k] = make_uint4(v, v, v, v);
                }
            }
        }
    }
    if (acc == 1.2345e300) out[0] = acc;
}

struct Bufs { double *planes; unsigned char *side; double *out; hipEvent_t e0, e1; };

template <int B, bool NT, int FL, int ST>
static void run(const Bufs &b) {
    const int ntiles = (int)(kPixels / kTile);
    printf("%3d %3d %3d %3d ", B, NT ? 1 : 0, FL, ST);
    for (const size_t stride : {kPixels, kPixels + kPad}) {
        for (const int per : {1, 2, 4, 8}) {
            const int grid = (ntiles + per - 1) / per;
            float best = 1e9f;
            for (int rep = 0; rep < 8; rep++) {              // rep 0 warms up; the order alternates as the sweeps' does
                CK(hipEventRecord(b.e0));
                hipLaunchKernelGGL((k_sweep<B, NT, FL, ST>), grid, 256, 0, 0, b.planes, stride, b.side, ntiles, per, rep & 1, b.out);
                CK(hipEventRecord(b.e1)); CK(hipEventSynchronize(b.e1));
                float ms; CK(hipEventElapsedTime(&ms, b.e0, b.e1));
                if (rep) best = std::min(best, ms);
            }
            printf(" %6.1f %4.2f", best * 1e3, 24.0 * kPixels / (best * 1e-3) * 1e-12);
        }
        printf(" |");
    }
    printf("\n");
    fflush(stdout);
}
template <int B, bool NT, int FL>
static void run_st(const Bufs &b) { run<B, NT, FL, 0>(b); run<B, NT, FL, 2>(b); run<B, NT, FL, 4>(b); run<B, NT, FL, 16>(b); }
template <int B, bool NT>
static void run_fl(const Bufs &b) { run_st<B, NT, 6>(b); run_st<B, NT, 12>(b); run_st<B, NT, 24>(b); }

int main() {
    Bufs b;
    const size_t doubles = 3 * (kPixels + kPad) + 64;
    CK(hipMalloc(&b.planes, doubles * sizeof(double)));
    CK(hipMalloc(&b.side, 2 * kPixels));
    CK(hipMalloc(&b.out, 64));
    CK(hipMemset(b.planes, 0, doubles * sizeof(double)));
    CK(hipMemset(b.side, 0, 2 * kPixels));
    CK(hipEventCreate(&b.e0)); CK(hipEventCreate(&b.e1));
    printf("three-plane tile read, %zu pixels (%.0f MB), best of 7: us and TB/s of plane bytes per column\n", kPixels, 24.0 * kPixels * 1e-6);
    printf("%3s %3s %3s %3s  %-47s | %-47s |\n", "B", "nt", "fl", "st", "stride 2^27 B: 1, 2, 4, 8 tiles per block", "stride 2^27 B + 2304 B: 1, 2, 4, 8 tiles per block");
    run_fl<8, false>(b); run_fl<8, true>(b); run_fl<16, false>(b); run_fl<16, true>(b);
    return 0;
}
