// common.h -- shared declarations of the MI355X-native patolette pipeline (product code).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/patolette.h"
#include "../../include/patolette_amd.h"

namespace pamd {

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                         \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            char _buf[512];                                                                     \
            snprintf(_buf, sizeof _buf, "patolette_amd: HIP error %s at %s:%d (%s)",            \
                     hipGetErrorString(_e), __FILE__, __LINE__, #expr);                         \
            throw pamd::HipError(_buf);                                                         \
        }                                                                                       \
    } while (0)

constexpr int kBuckets = 512;        // reference: quantize/global.c:22, local.c:15
constexpr double kDelta = 1e-16;     // reference: math/misc.h:5

// ---- kernel timing (HIP events on the launch stream), enabled by patolette_amd_profile_enable ----
struct KernelTimer {
    struct Rec { hipEvent_t a, b; int id; double bytes; const double *src; };   // src: bytes = bytes-per-unit x *src, read at collect()
    bool enabled = false;
    std::string only;                // when not empty: time just the kernel of this name
    unsigned sample_period = 1;      // ... and of that kernel every sample_period-th launch (two event records cost ~12 us)
    unsigned long long only_seen = 0;
    std::vector<std::string> names;
    std::vector<double> total_ms, total_bytes;
    std::vector<size_t> launches;
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    int id_of(const char *name);
    hipEvent_t get_event();
    void begin(int id, hipStream_t s, double bytes, const double *src = nullptr);
    void end(hipStream_t s);
    void collect();          // call after the stream is synchronised
    void reset();
};
KernelTimer &ktimer();

struct ScopedKernel {
    bool on;
    hipStream_t s;
    ScopedKernel(const char *name, hipStream_t stream, double bytes, const double *src = nullptr)
        : on(ktimer().enabled && (ktimer().only.empty() || ktimer().only == name)), s(stream) {
        if (on && !ktimer().only.empty() && ktimer().sample_period > 1) on = (ktimer().only_seen++ % ktimer().sample_period) == 0;
        if (on) ktimer().begin(ktimer().id_of(name), s, bytes, src);
    }
    ~ScopedKernel() { if (on) ktimer().end(s); }
};
#define PAMD_CAT2(a, b) a##b
#define PAMD_CAT(a, b) PAMD_CAT2(a, b)
// bytes = ALGORITHMIC HBM bytes of the launch (DESIGN.md lists the per-unit figures)
#define KTIME(name, stream, bytes) pamd::ScopedKernel PAMD_CAT(_ktime_scope_, __LINE__)(name, stream, (double)(bytes))
// a launch whose extent only the device knows: `per_unit` bytes x the double at `src` (filled in by the time collect() runs);
// src null = the plain form with `units` known on the host.  A launch that turned out empty (*src == 0) is not counted.
#define KTIME_DYN(name, stream, per_unit, units, src) \
    pamd::ScopedKernel PAMD_CAT(_ktime_scope_, __LINE__)(name, stream, (src) ? (double)(per_unit) : (double)(per_unit) * (double)(units), src)

// ---- workspace debugging (patolette_amd_debug_workspace, TESTS ONLY) ----
// bit 0: fresh f64 / f32 memory of a DevBuf (and f64 of a PinBuf) starts as quiet NaN (all bytes 0xFF), the floating-point
// fields of the record types with a WsPoison hook likewise; integer memory is never touched.  bit 1: count growths that free
// or move an allocation while the calling engine's streams still hold queued work.  bit 2: also name each such growth on stderr.
// Off: one relaxed load per growth.  Environment default: PAMD_DEBUG_WORKSPACE (read once, at library load).
constexpr int kWsPoison = 1, kWsCount = 2, kWsLog = 4;
extern std::atomic<int> g_debug_ws;
extern std::atomic<unsigned long long> g_late_growths;
// the streams of the engine the calling thread runs (set by WsGuard in the run paths; pointers, so that a stream made later counts)
struct WsStreams { const hipStream_t *s[2] = {nullptr, nullptr}; };
WsStreams &ws_streams();
struct WsGuard {
    WsStreams prev;
    WsGuard(const hipStream_t *a, const hipStream_t *b) : prev(ws_streams()) { ws_streams().s[0] = a; ws_streams().s[1] = b; }
    ~WsGuard() { ws_streams() = prev; }
    WsGuard(const WsGuard &) = delete;
    WsGuard &operator=(const WsGuard &) = delete;
};
void ws_growth(size_t bytes, const char *file, int line);              // an existing allocation is about to be freed or moved
void ws_poison_dev(void *p, size_t bytes);                             // 0xFF bytes; complete when it returns
void ws_poison_dev_rows(void *p, size_t pitch, size_t width, size_t rows);   // `width` bytes at the start of every `pitch`-byte row
inline void ws_poison_host(double *p, size_t n) { for (size_t i = 0; i < n; i++) p[i] = __builtin_nan(""); }
// per element type: what a fresh stretch [a, b) of elements gets under bit 0.  Default: nothing (integers, records without a hook)
template <typename T> struct WsPoison {
    static void dev(T *, size_t, size_t) {}
    static void host(T *, size_t, size_t) {}
};
template <> struct WsPoison<double> {
    static void dev(double *p, size_t a, size_t b) { ws_poison_dev(p + a, (b - a) * sizeof(double)); }
    static void host(double *p, size_t a, size_t b) { ws_poison_host(p + a, b - a); }
};
template <> struct WsPoison<float> {
    static void dev(float *p, size_t a, size_t b) { ws_poison_dev(p + a, (b - a) * sizeof(float)); }
    static void host(float *, size_t, size_t) {}
};
template <> struct WsPoison<float4> {            // the saliency stage's barrier state: its skewed copy has cells no kernel writes
    static void dev(float4 *p, size_t a, size_t b) { ws_poison_dev(p + a, (b - a) * sizeof(float4)); }
    static void host(float4 *, size_t, size_t) {}
};

// ---- simple device buffer with capacity reuse ----
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    void reserve(size_t n, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
        if (n <= cap) return;
        const int dbg = g_debug_ws.load(std::memory_order_relaxed);
        if (dbg && p) ws_growth(n * sizeof(T), file, line);
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        HIP_CHECK(hipMalloc((void **)&p, n * sizeof(T)));
        cap = n;
        if (dbg & kWsPoison) WsPoison<T>::dev(p, 0, n);
    }
    // grow keeping the first `keep` elements
    void grow(size_t n, size_t keep, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
        if (n <= cap) return;
        const int dbg = g_debug_ws.load(std::memory_order_relaxed);
        if (dbg && p) ws_growth(n * sizeof(T), file, line);
        T *q = nullptr;
        size_t ncap = n + n / 2;
        HIP_CHECK(hipMalloc((void **)&q, ncap * sizeof(T)));
        if (dbg & kWsPoison) WsPoison<T>::dev(q, keep, ncap);
        if (p && keep) HIP_CHECK(hipMemcpy(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice));
        if (p) (void)hipFree(p);
        p = q; cap = ncap;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

// pinned host staging buffer
template <typename T>
struct PinBuf {
    T *p = nullptr;
    size_t cap = 0;
    void reserve(size_t n, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
        if (n <= cap) return;
        const int dbg = g_debug_ws.load(std::memory_order_relaxed);
        if (dbg && p) ws_growth(n * sizeof(T), file, line);
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        HIP_CHECK(hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault));
        cap = n;
        if (dbg & kWsPoison) WsPoison<T>::host(p, 0, n);
    }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
};

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// hipFuncSetAttribute applies to the current device: a once-step per device (one process may drive several GPUs).  Caller
// threads arrive here together (one engine each), so the step runs under the lock and the device counts as done only after
// the step has returned: a thread that finds `done` set may launch at once, one that does not waits for the step's end, and a
// step that throws (HIP_CHECK) leaves the device not done for the next caller.  Warm path: one acquire load.
struct PerDeviceOnce {
    std::mutex mu;
    std::atomic<bool> done[64] = {};
    template <class F> void once(F &&step) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { step(); return; }
        if (done[dev].load(std::memory_order_acquire)) return;
        std::lock_guard<std::mutex> lk(mu);
        if (done[dev].load(std::memory_order_relaxed)) return;
        step();
        done[dev].store(true, std::memory_order_release);
    }
};

inline int num_cus() {                                      // compute units of the current device (256 on MI355X)
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    return v;
}

}  // namespace pamd
