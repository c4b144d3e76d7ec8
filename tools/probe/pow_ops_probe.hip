// Issue rate of the f64 instructions pamd_pow is made of (color_device.h), against v_fma_f64, on this part (not part of the product).
//   hipcc --offload-arch=gfx950 -O3 -o tools/probe/pow_ops_probe tools/probe/pow_ops_probe.hip
// Every test runs REPS x 64 copies of one instruction on 8 independent register sets (no copy waits for another: where the
// instruction writes what it reads, the eight chains interleave; elsewhere the destination is a register nobody reads), four
// wavefronts per SIMD on every CU, as k_convert runs.  Reported: ns and cycles (at 2.4 GHz) per wave-instruction per SIMD, and the
// ratio to v_fma_f64.  The integer and f64 forms that can stand in for a slow instruction are timed beside it.
#include <hip/hip_runtime.h>
#include <cstdio>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

constexpr int REPS = 256;

#define R8(S) S(0) S(1) S(2) S(3) S(4) S(5) S(6) S(7)
#define R64(S) R8(S) R8(S) R8(S) R8(S) R8(S) R8(S) R8(S) R8(S)

template <int T>
__global__ __launch_bounds__(256) void k_probe(float *out) {
    double d[8], e[8]; unsigned u[8], w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { d[i] = 1.0 + threadIdx.x * 0.001 + i; e[i] = 0.5 + i; u[i] = (threadIdx.x + 37 * i) & 7; w[i] = 0x3ff00000u + i; }
    const double c0 = 1.0001, c1 = 0.5;
    for (int r = 0; r < REPS; r++) {
        if constexpr (T == 0) {
#define S(i) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[i]) : "v"(c0), "v"(c1));
            R64(S)
#undef S
        } else if constexpr (T == 1) {
#define S(i) asm volatile("v_frexp_mant_f64 %0, %1" : "=v"(e[i]) : "v"(d[i]));
            R64(S)
#undef S
        } else if constexpr (T == 2) {
#define S(i) asm volatile("v_frexp_exp_i32_f64 %0, %1" : "=v"(w[i]) : "v"(d[i]));
            R64(S)
#undef S
        } else if constexpr (T == 3) {
#define S(i) asm volatile("v_ldexp_f64 %0, %1, %2" : "=v"(e[i]) : "v"(d[i]), "v"(u[i]));
            R64(S)
#undef S
        } else if constexpr (T == 4) {
#define S(i) asm volatile("v_cvt_i32_f64 %0, %1" : "=v"(w[i]) : "v"(d[i]));
            R64(S)
#undef S
        } else if constexpr (T == 5) {
#define S(i) asm volatile("v_cvt_f64_i32 %0, %1" : "=v"(e[i]) : "v"(u[i]));
            R64(S)
#undef S
        } else if constexpr (T == 6) {
#define S(i) asm volatile("v_rndne_f64 %0, %1" : "=v"(e[i]) : "v"(d[i]));
            R64(S)
#undef S
        } else if constexpr (T == 7) {
#define S(i) asm volatile("v_rcp_f64 %0, %1" : "=v"(e[i]) : "v"(d[i]));
            R64(S)
#undef S
        } else if constexpr (T == 8) {
#define S(i) asm volatile("v_div_scale_f64 %0, vcc, %1, %2, %1" : "=v"(e[i]) : "v"(d[i]), "v"(c0) : "vcc");
            R64(S)
#undef S
        } else if constexpr (T == 9) {
#define S(i) asm volatile("v_div_fmas_f64 %0, %1, %2, %3" : "=v"(e[i]) : "v"(d[i]), "v"(c0), "v"(c1) : "vcc");
            R64(S)
#undef S
        } else if constexpr (T == 10) {
#define S(i) asm volatile("v_div_fixup_f64 %0, %1, %2, %3" : "=v"(e[i]) : "v"(d[i]), "v"(c0), "v"(c1));
            R64(S)
#undef S
        } else if constexpr (T == 11) {
#define S(i) asm volatile("v_add_f64 %0, %0, %1" : "+v"(d[i]) : "v"(c1));
            R64(S)
#undef S
        } else if constexpr (T == 12) {
#define S(i) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(d[i]) : "v"(c0));
            R64(S)
#undef S
        } else if constexpr (T == 13) {
#define S(i) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(w[i]) : "v"(0x000fffffu), "v"(0x3ff00000u));
            R64(S)
#undef S
        } else if constexpr (T == 14) {
#define S(i) asm volatile("v_bfe_u32 %0, %0, 13, 7" : "+v"(w[i]));
            R64(S)
#undef S
        } else if constexpr (T == 15) {
#define S(i) asm volatile("v_lshrrev_b32 %0, 20, %0" : "+v"(w[i]));
            R64(S)
#undef S
        }
    }
    double acc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) acc += d[i] + e[i] + (double)u[i] + (double)w[i];
    if (acc == 1.2345e300) out[0] = (float)acc;
}

int main() {
    float *out;
    CK(hipMalloc(&out, 64));
    int cus = 256; hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    int khz = 2400000; hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0);
    printf("CUs %d, clock attribute %d kHz, 4 wavefronts per SIMD, %d x 64 instructions per wavefront\n", cus, khz, REPS);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const char *names[] = {"v_fma_f64", "v_frexp_mant_f64", "v_frexp_exp_i32_f64", "v_ldexp_f64", "v_cvt_i32_f64", "v_cvt_f64_i32", "v_rndne_f64",
                           "v_rcp_f64", "v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_add_f64", "v_mul_f64", "v_and_or_b32",
                           "v_bfe_u32", "v_lshrrev_b32"};
    const int wps = 4, blocks = cus * wps;                    // 256 threads = 4 waves = one per SIMD
    double fma_ns = 0;
    auto run = [&](int t, auto kern) {
        for (int i = 0; i < 2; i++) hipLaunchKernelGGL(kern, blocks, 256, 0, 0, out);
        hipEventRecord(e0);
        for (int i = 0; i < 5; i++) hipLaunchKernelGGL(kern, blocks, 256, 0, 0, out);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        const double ninst = (double)REPS * 64 * wps;         // wave-instructions per SIMD per launch
        const double ns = ms / 5 * 1e6 / ninst;
        if (t == 0) fma_ns = ns;
        printf("%-22s %7.2f ns/inst/SIMD  = %5.2f cycles @2.4GHz  = %5.2f x v_fma_f64\n", names[t], ns, ns * 2.4, ns / fma_ns);
    };
#define RUN(T) run(T, k_probe<T>);
    RUN(0) RUN(1) RUN(2) RUN(3) RUN(4) RUN(5) RUN(6) RUN(7) RUN(8) RUN(9) RUN(10) RUN(11) RUN(12) RUN(13) RUN(14) RUN(15)
    CK(hipDeviceSynchronize());
    return 0;
}
