// pipeline.hip -- host orchestration of the MI355X-native patolette path and its C ABI.
//
// Stage sequencing follows lib/src/patolette.c:157-343 (convert -> GQ -> LQ -> [KMeans] ->
// NN map | dither -> palette back-conversion and write-out); everything O(N) runs in the HIP
// kernels of color.hip / quant.hip / kmeans.hip / map.hip on one stream.  The host keeps only
// the O(K) control work the reference also does serially: 3x3 eigen-solves, the 512-bucket DP
// of the global quantiser, and the greedy split selection (local.c:347-390) replayed over the
// candidate tree the GPU evaluates in rounds.
#include <algorithm>
#include <functional>
#include <chrono>
#include <cmath>
#include <atomic>
#include <memory>
#include <mutex>
#include <thread>
#include <future>
#include <type_traits>

#include "color_device.h"
#include "common.h"
#include "host_math.h"
#include "kmeans.h"
#include "map.h"
#include "ordered.h"
#include "delta.h"
#include "measure.h"
#include "lzw.h"
#include "lzw_near.h"
#include "deflate.h"
#include "hist.h"
#include "saliency.h"
#include "quant.h"
#include "rgba.h"
#include "compact.h"
#include "split_frontier.h"
#include "given.h"

namespace pamd {

// launchers defined in color.hip
void launch_convert(int which, const double *src, double *dst, size_t n, ConvertStats *stats, hipStream_t s, BinK sumk = BinK{0.0, 0.0},
                    BinK momk = BinK{0.0, 0.0}, size_t begin = 0, size_t end = ~(size_t)0, bool init_stats = true,
                    bool general = false);
void launch_convert_rows(int which, const double *rows, double *dst, size_t n, ConvertStats *stats, hipStream_t s,
                         BinK sumk = BinK{0.0, 0.0}, BinK momk = BinK{0.0, 0.0}, size_t begin = 0, size_t end = ~(size_t)0,
                         bool init_stats = true);
void launch_convert_u8(int which, const unsigned char *pixels, int channels, double *dst, size_t n, ConvertStats *stats,
                       hipStream_t s, BinK sumk = BinK{0.0, 0.0}, BinK momk = BinK{0.0, 0.0}, size_t begin = 0, size_t end = ~(size_t)0,
                       bool init_stats = true, bool general = false);
void launch_reconstruct(const void *map, int map_elem, size_t n, const unsigned char *pal_u8, int k, unsigned char *out,
                        hipStream_t s);
void launch_weight_stats(const double *w, size_t n, ConvertStats *stats, hipStream_t s);
void launch_pow(const double *x, double y, double *out, size_t n, hipStream_t s, int mode);
void launch_fill_image(double *d, size_t n, uint64_t seed, hipStream_t s);
void launch_fill_weights(double *d, size_t n, uint64_t seed, hipStream_t s);

// --------------------------------------------------------------------------------------------
// kernel timer
// --------------------------------------------------------------------------------------------
// (never destroyed: HIP objects must not be released after the runtime has shut down)
KernelTimer &ktimer() { static thread_local KernelTimer *t = new KernelTimer; return *t; }

// patolette_amd_debug_workspace (tests only; common.h)
std::atomic<int> g_debug_ws{getenv("PAMD_DEBUG_WORKSPACE") ? atoi(getenv("PAMD_DEBUG_WORKSPACE")) & (kWsPoison | kWsCount | kWsLog) : 0};
std::atomic<unsigned long long> g_late_growths{0};
WsStreams &ws_streams() { static thread_local WsStreams w; return w; }
void ws_growth(size_t bytes, const char *file, int line) {
    const int dbg = g_debug_ws.load(std::memory_order_relaxed);
    if (!(dbg & (kWsCount | kWsLog))) return;
    bool queued = false;                                   // (work that completes before this query goes unseen: a zero count is evidence only)
    for (const hipStream_t *sp : ws_streams().s)
        if (sp && *sp && hipStreamQuery(*sp) == hipErrorNotReady) queued = true;
    if (!queued) return;
    g_late_growths.fetch_add(1);
    if (dbg & kWsLog) fprintf(stderr, "patolette_amd: workspace growth to %zu bytes while work is queued (%s:%d)\n", bytes, file, line);
}
void ws_poison_dev(void *p, size_t bytes) {
    if (!bytes) return;
    HIP_CHECK(hipMemsetAsync(p, 0xFF, bytes, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
}
void ws_poison_dev_rows(void *p, size_t pitch, size_t width, size_t rows) {
    if (!width || !rows) return;
    HIP_CHECK(hipMemset2DAsync(p, pitch, 0xFF, width, rows, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
}
int KernelTimer::id_of(const char *name) {
    for (size_t i = 0; i < names.size(); i++) if (names[i] == name) return (int)i;
    names.emplace_back(name); total_ms.push_back(0); total_bytes.push_back(0); launches.push_back(0);
    return (int)names.size() - 1;
}
hipEvent_t KernelTimer::get_event() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); return e;
}
void KernelTimer::begin(int id, hipStream_t s, double bytes, const double *src) {
    Rec r; r.id = id; r.bytes = bytes; r.src = src; r.a = get_event(); r.b = get_event();
    HIP_CHECK(hipEventRecord(r.a, s));
    pending.push_back(r);
}
void KernelTimer::end(hipStream_t s) { HIP_CHECK(hipEventRecord(pending.back().b, s)); }
void KernelTimer::collect() {
    for (auto &r : pending) {
        float ms = 0;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess && !(r.src && *r.src == 0.0)) {
            total_ms[r.id] += ms; total_bytes[r.id] += r.src ? r.bytes * *r.src : r.bytes; launches[r.id] += 1;
        }
        pool.push_back(r.a); pool.push_back(r.b);
    }
    pending.clear();
}
void KernelTimer::reset() { collect(); names.clear(); total_ms.clear(); total_bytes.clear(); launches.clear(); }

// --------------------------------------------------------------------------------------------
// node table scatter / gather (host mirror <-> device table) in one copy + one tiny kernel
// --------------------------------------------------------------------------------------------
// The root's two tilings (consecutive runs of kTileA / kTileP pixels of node 0), its round list and the cleared bucket tables, made ON
// the device in one launch: before, the host built ~10 000 tile records and sent them up in four copies followed by three fills -- 30 us
// of host work during which the GPU had nothing queued behind the conversion, then seven 4.6-us operations in a row.
__global__ __launch_bounds__(256) void k_gq_prepare(Tile *tA, int ntA, Tile *tP, int ntP, unsigned long long N, int *round_nodes, int *node_tile0,
                                                    double *hist, unsigned long long nhist, unsigned long long *hsize, unsigned int *hcount) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x, t0 = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned long long i = t0; i < (unsigned long long)ntA; i += stride) {
        const unsigned long long o = i * (unsigned long long)kTileA;
        tA[i] = Tile{o, (unsigned)(N - o < (unsigned long long)kTileA ? N - o : (unsigned long long)kTileA), 0u};
    }
    for (unsigned long long i = t0; i < (unsigned long long)ntP; i += stride) {
        const unsigned long long o = i * (unsigned long long)kTileP;
        tP[i] = Tile{o, (unsigned)(N - o < (unsigned long long)kTileP ? N - o : (unsigned long long)kTileP), 0u};
    }
    for (unsigned long long i = t0; i < nhist; i += stride) hist[i] = 0.0;
    for (unsigned long long i = t0; i < (unsigned long long)kBuckets; i += stride) { hsize[i] = 0ULL; hcount[i] = 0u; }
    if (t0 == 0) { round_nodes[0] = 0; node_tile0[0] = 0; node_tile0[1] = ntP; }
}

__global__ void k_put_nodes(NodeDev *table, const NodeIn *stage, const int *ids, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const NodeIn in = stage[i];
    NodeDev &d = table[ids[i]];
    d.begin = in.begin; d.n = in.n; d.gn = in.gn; d.buf = in.buf; d.slot = in.slot; d.child0 = in.child0; d.nchild = in.nchild;
    for (int j = 0; j < 3; j++) { d.axis[j] = in.axis[j]; d.mean[j] = in.mean[j]; }
    d.sw = in.sw; d.klin = in.klin; d.kquad = in.kquad;
    node_reset_outputs(d);
    d.split = in.split; d.psplit = -1;
}
// one record, passed as a kernel argument: no staging copies (the root's record at the start of every call)
__global__ void k_put_node1(NodeDev *table, const int id, const NodeIn in) {
    NodeDev &d = table[id];
    d.begin = in.begin; d.n = in.n; d.gn = in.gn; d.buf = in.buf; d.slot = in.slot; d.child0 = in.child0; d.nchild = in.nchild;
    for (int j = 0; j < 3; j++) { d.axis[j] = in.axis[j]; d.mean[j] = in.mean[j]; }
    d.sw = in.sw; d.klin = in.klin; d.kquad = in.kquad;
    node_reset_outputs(d);
    d.split = in.split; d.psplit = -1;
}
__global__ void k_get_nodes(const NodeDev *table, NodeOut *stage, const int *ids, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const NodeDev &d = table[ids[i]];
    NodeOut o;
    o.begin = d.begin; o.n = d.n; o.gn = d.gn; o.buf = d.buf; o.degenerate = d.degenerate; o.split = d.split; o.psplit = d.psplit;
    o.sw = d.sw;
    for (int j = 0; j < 3; j++) o.mean[j] = d.mean[j];
    for (int q = 0; q < 7; q++) {                          // slot sums are exact (binned parts), any order
        double s0 = 0, s1 = 0;
        for (int k = 0; k < kSlots; k++) { s0 += d.acc[k][q][0]; s1 += d.acc[k][q][1]; }
        o.acc[q][0] = s0; o.acc[q][1] = s1;
    }
    stage[i] = o;
}

// One launch prepares a split round from the packet the host uploaded in one copy: node records into the table,
// the tile lists of both tilings (a pure function of the nodes' segments), and zeroed histograms.
struct RoundSetup {
    const NodeIn *recs; const int *ids; const int *tA0; const int *tP0;    // device pointers into the packet
    int nr, ntA, ntP;
    Tile *tilesA, *tilesP;
    double *hist; size_t nhist;
    unsigned long long *hsize; unsigned int *hcount; size_t nbk;
};
__device__ __forceinline__ int node_of_tile(const int *t0, int nr, int t) {   // largest r with t0[r] <= t
    int lo = 0, hi = nr;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (t0[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(256) void k_round_setup(NodeDev *table, RoundSetup a) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < (size_t)a.nr; i += stride) {
        const NodeIn in = a.recs[i];
        NodeDev &d = table[a.ids[i]];
        d.begin = in.begin; d.n = in.n; d.gn = in.gn; d.buf = in.buf; d.slot = in.slot; d.child0 = in.child0; d.nchild = in.nchild;
        for (int j = 0; j < 3; j++) { d.axis[j] = in.axis[j]; d.mean[j] = in.mean[j]; }
        d.sw = in.sw; d.klin = in.klin; d.kquad = in.kquad;
    }
    for (size_t i = tid; i < (size_t)a.nr * kNodeResetElems; i += stride)        // outputs of the round's nodes, one store per thread
        node_reset_element(table[a.ids[i / kNodeResetElems]], (int)(i % kNodeResetElems));
    for (size_t t = tid; t < (size_t)a.ntA; t += stride) {
        const int r = node_of_tile(a.tA0, a.nr, (int)t);
        const unsigned long long o = (unsigned long long)((int)t - a.tA0[r]) * kTileA, n = a.recs[r].n;
        a.tilesA[t] = Tile{a.recs[r].begin + o, (unsigned)(n - o < (unsigned long long)kTileA ? n - o : kTileA), (unsigned)a.ids[r]};
    }
    for (size_t t = tid; t < (size_t)a.ntP; t += stride) {
        const int r = node_of_tile(a.tP0, a.nr, (int)t);
        const unsigned long long o = (unsigned long long)((int)t - a.tP0[r]) * kTileP, n = a.recs[r].n;
        a.tilesP[t] = Tile{a.recs[r].begin + o, (unsigned)(n - o < (unsigned long long)kTileP ? n - o : kTileP), (unsigned)a.ids[r]};
    }
    for (size_t i = tid; i < a.nhist; i += stride) a.hist[i] = 0.0;
    for (size_t i = tid; i < a.nbk; i += stride) { a.hsize[i] = 0ULL; a.hcount[i] = 0u; }
}


// =============================================================================================
// The split loop driven from the DEVICE (local.c:318-404 for K <= 256 on one GPU)
// =============================================================================================
// The host-driven loop further down pays, per round, a stream synchronisation, the host's turn (the children's 3x3 eigen-solves,
// the greedy replay, the next round's packet) and an upload: 30-110 us of idle GPU nine times per image -- a third of a
// 1920x1080 call.  Here the rounds follow each other on the stream without the host looking, and the greedy loop of
// local.c:347-390 is replayed ONCE, afterwards, over the evaluated candidate tree (split_cluster(c) depends only on c's members,
// never on the greedy order).  Which leaves to evaluate is decided on the device by a rule that needs no replay and never
// misses a node the replay will commit:
//   the priority of an evaluated node is p(v) = min(benefit(v), p(parent(v))) (its ancestors are committed before it, so the
//   replay reaches v only after benefits >= p(v)).  If M = K - (base clusters) evaluated nodes have p >= tau, the replay's M
//   commits all have benefit >= tau (those M nodes and their ancestors are always available to it), so a leaf u with
//   min(ub(u), p(parent(u))) < tau -- ub an upper bound of any split's benefit -- is never committed and never blocks the
//   replay's exactness test (its bound is below every committed benefit).  tau = a lower estimate of the M-th largest p.
// Per round: k_lq_children (one wavefront per child: moment slots summed, distortion, the bound), k_lq_select (block 0: benefits and
// priorities of the nodes just split, tau, the next round's node list, tile prefixes and sizes; the other blocks meanwhile solve
// the children's eigen-problems with hm::eigen_sym3, the host's own code, whose ~12 us of dependent divisions and square roots
// would otherwise sit on the critical path), then the sweeps, launched with upper-bound grids and reading their sizes from
// device memory (RoundDyn).  The host synchronises once (as many rounds are enqueued as the previous image of this size needed;
// a surplus round is nine empty launches, a deficit one more synchronisation), downloads 16 bytes per node and replays.
// Same decisions as the host-driven loop: same sums, same solver, same comparisons; only the SET of evaluated nodes differs
// (a few more: the host prunes with a heuristic a replay in lock-step can afford).
// what the global quantiser left when it ran on the device (k_gq_control below): base clusters, failure, the cuts [0 = q0 .. q_kbase = 512]
struct GqOut { int kbase, error, pad[2]; int cuts[16]; unsigned long long ticks[8]; };   // ticks: wall_clock64 (100 MHz) at the kernel's phase boundaries, a diagnostic

constexpr int kLqDevMaxK = 256;                       // palette sizes the device-driven loop takes
constexpr int kLqNodeCap = 16 * kLqDevMaxK + 256;     // candidate-tree nodes; beyond it the call starts over on the host-driven loop
constexpr int kLqRoundCap = 512;                      // nodes evaluated per round (more candidates wait for the next one)
constexpr int kLqMaxRounds = 96;

// (LqRec, the record the device leaves per node for the replay: split_frontier.h)
struct LqCen { double mean[3]; double gn; };          // what PALETTE_create needs of a node (create.c:11-33) + its member count
struct LqHead {                                       // copied to the host at every check
    int done, error, rounds, nnodes, neval, pad;
    unsigned long long split_evals, split_px;
    double tau;
    double round_px[kLqMaxRounds], round_nr[kLqMaxRounds];
};
struct LqCtl {                                        // device memory
    LqHead h;
    int K, M, nleaves, pad;
    int ncids[2];                                     // children awaiting finalisation; [control call & 1]: k_lq_select's block 0 writes the NEXT
    RoundDyn dyn;                                     // call's list while the other blocks still read this one's
    int leaves[kLqNodeCap];
    int round_ids[kLqRoundCap];
    int cids[2][2 * kLqRoundCap];
    int tA0[kLqRoundCap + 1], tP0[kLqRoundCap + 1];
    int nparent[kLqNodeCap];
    double np[kLqNodeCap];                            // priority of the evaluated nodes
    LqRec nrec[kLqNodeCap];                           // -> host: the replay's table
    LqCen ncen[kLqNodeCap];                           // -> host: centres
};
// patolette_amd_debug_workspace bit 0: the control state's floating-point fields start as NaN (its integers stay as allocated)
template <> struct WsPoison<LqCtl> {
    static void dev(LqCtl *p, size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            char *c = reinterpret_cast<char *>(p + i);
            ws_poison_dev(c + offsetof(LqCtl, h) + offsetof(LqHead, tau), sizeof(double) * (1 + 2 * kLqMaxRounds));
            ws_poison_dev(c + offsetof(LqCtl, np), sizeof(LqCtl::np));
            ws_poison_dev_rows(c + offsetof(LqCtl, nrec), sizeof(LqRec), sizeof(double), kLqNodeCap);
            ws_poison_dev(c + offsetof(LqCtl, ncen), sizeof(LqCtl::ncen));
        }
    }
    static void host(LqCtl *, size_t, size_t) {}
};

// wave-wide maximum of a double through DPP row shifts and row broadcasts (lanes without a source keep their own value)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_max_f64(const double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int tlo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int thi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    return fmax(v, __hiloint2double(thi, tlo));
}

// The children the last round produced (first launch of a call: the base clusters), ONE WAVEFRONT EACH: the sixteen slots of the
// moment accumulators summed (exact parts: any order), the distortion, and an upper bound of any split's benefit
// (hm::lambda_max_bound x sum of weights: the scatter between two groups along their mean difference cannot exceed the node's
// scatter along that direction; see leaf_bound).  init_kbase > 0: the call's first launch, which also sets the loop's state up
// (the base clusters are nodes init_first .. init_first + init_kbase - 1).
__global__ __launch_bounds__(256) void k_lq_children(NodeDev *nodes, LqCtl *c, const int call, int init_kbase,
                                                     const int init_first, int init_nnodes, const int init_K, const GqOut *gq) {
    const bool init = init_kbase > 0;
    if (!init && c->h.done) return;
    if (init && gq) { init_kbase = gq->kbase; init_nnodes = init_first + init_kbase; }   // the global quantiser ran on the device (k_gq_control): its count
    const int ncids = init ? init_kbase : c->ncids[call & 1];
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (init && blockIdx.x == 0 && threadIdx.x == 0) {
        c->K = init_K; c->M = init_K - init_kbase; c->nleaves = 0; c->ncids[0] = init_kbase; c->dyn = RoundDyn{0, 0, 0, 0};
        c->h.done = 0; c->h.error = 0; c->h.rounds = 0; c->h.nnodes = init_nnodes; c->h.neval = 0; c->h.split_evals = 0ULL; c->h.split_px = 0ULL;
        c->h.tau = 0.0;
        for (int r = 0; r < kLqMaxRounds; r++) { c->h.round_px[r] = 0.0; c->h.round_nr[r] = 0.0; }
        if (gq && gq->error) { c->h.done = 1; c->h.error = 3; c->ncids[0] = 0; }
        // the records below the base clusters (the root) belong to no candidate: k_lq_select's rank count runs over ALL records below
        // nnodes, and what an earlier call or the allocator left there must not pass for an evaluated node (a stale record with a large
        // priority raised tau by one rank: a leaf the replay needed was dropped -- one call in some hundreds, engines out of the pool)
        for (int i = 0; i < init_first; i++) { c->nrec[i] = LqRec{0.0, -1, 1}; c->np[i] = 0.0; c->nparent[i] = -1; }
    }
    if (init && gq && gq->error) return;
    if (wave >= ncids) return;
    const int id = init ? init_first + wave : c->cids[call & 1][wave];
    if (init && lane == 0) c->cids[0][wave] = id;
    NodeDev &d = nodes[id];
    const double *acc = &d.acc[0][0][0];                            // acc[k][q][p]: 224 consecutive doubles; lane r < 14 sums element r of every slot
    double sum = 0;
    if (lane < 14) {
        double v[kSlots];
#pragma unroll
        for (int k = 0; k < kSlots; k++) v[k] = acc[k * 14 + lane];
#pragma unroll
        for (int k = 0; k < kSlots; k++) sum += v[k];
    }
    const double pair = sum + __shfl_down(sum, 1, 64);             // lanes 0, 2, .., 12: first + second part of quantity q = lane / 2
    double cov[7];
#pragma unroll
    for (int q = 0; q < 7; q++)
        cov[q] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(pair), 2 * q), __builtin_amdgcn_readlane(__double2loint(pair), 2 * q));
    if (lane != 0) return;
    double ub = cov[6];
    const bool single = d.gn <= 1ULL;
    const double sw = d.sw;
    if (single || !(sw > 0)) ub = 0;
    else {
        double c6[6];
        for (int q = 0; q < 6; q++) c6[q] = cov[q] / sw;
        const double b = hm::lambda_max_bound(c6) * sw * (1.0 + 1e-9) + 1e-9 * cov[6];
        if (b == b && b < ub) ub = b;
    }
    for (int q = 0; q < 6; q++) d.cov6[q] = cov[q];
    d.dist = cov[6]; d.ub = ub; d.axis_state = 0;
    c->nrec[id] = LqRec{single ? 0.0 : ub, -1, single ? 1 : 0};
    c->nparent[id] = init ? -1 : c->round_ids[wave >> 1];
    c->ncen[id] = LqCen{{d.mean[0], d.mean[1], d.mean[2]}, (double)d.gn};
    c->leaves[(init ? 0 : c->nleaves) + wave] = id;
}

__device__ __forceinline__ int block_excl_scan_256(const int v, int *sw /* [5] */, int &total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int inc = (int)wave_scan_incl_u32((unsigned)v);
    __syncthreads();                                   // sw may still be read from the previous scan
    if (lane == 63) sw[wid] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wid; w++) base += sw[w];
    total = sw[0] + sw[1] + sw[2] + sw[3];
    return base + inc - v;
}

// order-preserving 64-bit key of a priority (negative or NaN -> 0: below every threshold that matters)
__device__ __forceinline__ unsigned long long lq_key(const double p) { return p > 0.0 ? (unsigned long long)__double_as_longlong(p) : 0ULL; }

// The split loops' speculation: of the leaves that could still matter, those whose priority is below kSpecBeta times the best of
// them wait.  Swept 1/256 .. 1 on six kinds of content: 1/4 evaluates least (noise 514 -> 319 splits, lq -8 %).
constexpr double kSpecBeta = 0.25;

__global__ __launch_bounds__(256) void k_lq_select(NodeDev *nodes, LqCtl *c, const int call, const int e_lin, const int e_quad) {
    if (c->h.done) return;                                         // (set by an EARLIER launch only: every block of this one sees the same)
    const int tid = threadIdx.x, lane = tid & 63;
    const int cur = call & 1, nxt = cur ^ 1;
    const int ncids = c->ncids[cur];
    if (blockIdx.x > 0) {
        // ---- the other blocks: the children's principal axes (cluster.c:191-217 -> pca.c:122-149 -> dsyev), one wavefront per child,
        // needed by the NEXT round's projection only -- solved here, beside the selection, instead of in front of it
        const int w = ((int)blockIdx.x - 1) * 4 + (tid >> 6);
        if (w >= ncids) return;
        NodeDev &d = nodes[c->cids[cur][w]];
        if (d.gn <= 1ULL || !(d.sw > 0)) { if (lane == 0) d.axis_state = d.gn <= 1ULL ? 0 : -1; return; }
        double c6[6];
        for (int q = 0; q < 6; q++) c6[q] = d.cov6[q] / d.sw;
        double a[9] = {c6[0], c6[1], c6[2], c6[1], c6[3], c6[4], c6[2], c6[4], c6[5]};
        double wv[3];
        const int info = hm::eigen_sym3(a, wv);
        if (lane == 0) {
            if (info != 0) d.axis_state = -1;
            else { d.axis[0] = a[6]; d.axis[1] = a[7]; d.axis[2] = a[8]; d.axis_state = 1; }
        }
        return;
    }
    __shared__ int sw[5];
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long s_prefix, s_px;
    __shared__ int s_need, s_neval, s_first;
    __shared__ double s_umax[4];
    const int M = c->M;
    const int nn = c->h.nnodes;
    // ---- A. the nodes of the last round are split now: benefit (local.c:256-275) and priority.  A node whose eigen-solve failed a round
    // ago (never seen on finite input) was swept along a zero axis: it never splits, its children are dropped
    const int nr_prev = c->dyn.nr;
    int evald = 0;
    for (int i = tid; i < nr_prev; i += 256) {
        const int id = c->round_ids[i];
        const NodeDev &d = nodes[id];
        if (d.axis_state < 0) { c->nrec[id] = LqRec{0.0, -1, 1}; c->np[id] = 0.0; continue; }
        const int l = d.child0;
        const double b = d.dist - (nodes[l].dist + nodes[l + 1].dist);
        const int par = c->nparent[id];
        const double pp = par < 0 ? INFINITY : c->np[par];
        c->nrec[id].val = b; c->nrec[id].kn = 1;
        c->np[id] = b < pp ? b : pp;
        evald++;
    }
    if (tid == 0) { s_neval = 0; s_px = 0ULL; }
    __syncthreads();
    if (evald) atomicAdd(&s_neval, evald);
    __syncthreads();
    const int neval = c->h.neval + s_neval;
    // ---- B. tau: a lower estimate of the M-th largest priority among the evaluated nodes (three 8-bit radix passes on the order-preserving
    // key: the lower edge of the 2^-12-wide bin that holds it)
    double tau = 0.0;
    if (neval >= M && M > 0) {
        unsigned long long prefix = 0ULL;
        int need = M;
        for (int pass = 0; pass < 3; pass++) {
            const int shift = 56 - 8 * pass;
            hist[tid] = 0u;
            __syncthreads();
            for (int i = tid; i < nn; i += 256) {
                const LqRec r = c->nrec[i];
                if (r.kn && r.left >= 0) {
                    const unsigned long long k = lq_key(c->np[i]);
                    if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255ULL], 1u);
                }
            }
            __syncthreads();
            // the bin that holds the need-th largest key: the largest b > 0 whose bins b .. 255 hold `need` keys or more (else bin 0).
            // Thread t takes bin 255 - t: a block scan gives every suffix at once (one thread walking the 256 bins paid an LDS round
            // trip per bin, three passes a call: ~15 of the launch's 22 us)
            {
                const int mine = (int)hist[255 - tid];
                int total;
                const int excl = block_excl_scan_256(mine, sw, total);
                if (tid == 0) s_first = 256;
                __syncthreads();
                if (excl + mine >= need && tid <= 254) atomicMin(&s_first, tid);
                __syncthreads();
                const int f = s_first;
                if (f < 256) { if (tid == f) { s_need = need - excl; s_prefix = prefix | ((unsigned long long)(255 - f) << shift); } }
                else if (tid == 254) { s_need = need - (excl + mine); s_prefix = prefix; }
            }
            __syncthreads();
            need = s_need; prefix = s_prefix;
        }
        tau = __longlong_as_double((long long)prefix);
    }
    const double thr = fmax(kDelta, tau * (1.0 - 1e-9));
    // ---- C. the leaves to evaluate: the children just made and what earlier rounds left waiting.  A leaf whose priority cannot reach
    // tau never will (tau only grows): dropped for good.  Of the others, those far below the best of them wait (kSpecBeta, the host-driven
    // loop's own rule and value: most of them fall below tau before their turn comes -- 500 evaluations a 256-colour palette without
    // the rule, ~330 with it); the best one is always taken, so every round evaluates something, and the loop ends when no leaf reaches
    // tau -- the set the replay needs is complete either way.  After 48 rounds everything that reaches tau is taken (a bound on the
    // number of rounds whatever the content).
    const int nleaves = c->nleaves + ncids;
    auto leaf_prio = [&](const int id) -> double {
        const LqRec r = c->nrec[id];
        const int par = c->nparent[id];
        if (r.kn || (par >= 0 && nodes[par].axis_state < 0)) return -1.0;
        const double pp = par < 0 ? INFINITY : c->np[par];
        return r.val < pp ? r.val : pp;
    };
    double thr2 = thr;
    if (c->h.rounds < 48) {
        double u = -1.0;
        for (int i = tid; i < nleaves; i += 256) { const double pr = leaf_prio(c->leaves[i]); u = pr > u ? pr : u; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const double v = __shfl_xor(u, o, 64); u = v > u ? v : u; }
        __syncthreads();
        if (lane == 0) s_umax[tid >> 6] = u;
        __syncthreads();
        u = fmax(fmax(s_umax[0], s_umax[1]), fmax(s_umax[2], s_umax[3]));
        if (kSpecBeta * u > thr2) thr2 = kSpecBeta * u;
    }
    int nkeep = 0, nr = 0;
    for (int base = 0; base < nleaves; base += 256) {
        const int i = base + tid;
        int id = -1, sel = 0, keep = 0;
        if (i < nleaves) {
            id = c->leaves[i];
            const double pr = leaf_prio(id);
            sel = pr >= thr2 ? 1 : 0;
            keep = (!sel && pr >= thr) ? 1 : 0;                      // waits
        }
        int tsel, tkeep;
        const int psel = block_excl_scan_256(sel, sw, tsel);
        if (nr + tsel > kLqRoundCap && sel && nr + psel >= kLqRoundCap) { sel = 0; keep = 1; }   // the round is full: the rest waits for the next one
        const int pkeep = block_excl_scan_256(keep, sw, tkeep);
        if (sel) c->round_ids[nr + psel] = id;
        __syncthreads();
        if (keep) c->leaves[nkeep + pkeep] = id;
        nr = min(nr + tsel, kLqRoundCap);
        nkeep += tkeep;
        __syncthreads();
    }
    if (nr == 0) {                                                 // nothing left that the replay could commit: the loop is over
        if (tid == 0) { c->h.done = 1; c->h.neval = neval; c->h.tau = tau; c->nleaves = 0; c->ncids[nxt] = 0; c->dyn = RoundDyn{0, 0, 0, 0}; }
        return;
    }
    // ---- D. the round: slots, children ids, tile prefixes of both tilings (what the host's packet carries in the host-driven loop)
    if (nn + 2 * nr > kLqNodeCap) {                                // the candidate tree outgrew the table: the host-driven loop takes the call over
        if (tid == 0) { c->h.done = 1; c->h.error = 2; c->dyn = RoundDyn{0, 0, 0, 0}; }
        return;
    }
    int runA = 0, runP = 0;
    for (int base = 0; base < nr; base += 256) {
        const int r = base + tid;
        int ta = 0, tp = 0;
        unsigned long long n = 0ULL;
        if (r < nr) {
            const int id = c->round_ids[r];
            NodeDev &d = nodes[id];
            d.slot = r; d.child0 = nn + 2 * r; d.nchild = 2;
            int P = 1;                                              // the grids of the exact sums follow the node's own size (make_nodedev)
            while ((1ULL << P) < (d.gn > 1ULL ? d.gn : 2ULL)) P++;
            d.klin = make_bink(e_lin, P); d.kquad = make_bink(e_quad, P);
            c->nrec[id].left = nn + 2 * r;
            c->cids[nxt][2 * r] = nn + 2 * r; c->cids[nxt][2 * r + 1] = nn + 2 * r + 1;
            n = d.n;
            ta = (int)((n + kTileA - 1) / kTileA); tp = (int)((n + kTileP - 1) / kTileP);
        }
        int totA, totP;
        const int pa = block_excl_scan_256(ta, sw, totA);
        const int pp = block_excl_scan_256(tp, sw, totP);
        if (r < nr) { c->tA0[r] = runA + pa; c->tP0[r] = runP + pp; }
        runA += totA; runP += totP;
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);     // pixels of the round (a statistic)
        if (lane == 0 && n) atomicAdd(&s_px, n);
    }
    __syncthreads();
    if (tid == 0) {
        const int round = c->h.rounds;
        const unsigned long long rpx = s_px;
        c->tA0[nr] = runA; c->tP0[nr] = runP;
        c->nleaves = nkeep; c->ncids[nxt] = 2 * nr;
        c->dyn = RoundDyn{nr, runA, runP, 0};
        c->h.nnodes = nn + 2 * nr; c->h.neval = neval; c->h.tau = tau;
        c->h.split_evals += (unsigned long long)nr; c->h.split_px += rpx; c->h.rounds = round + 1;
        if (round < kLqMaxRounds) { c->h.round_px[round] = (double)rpx; c->h.round_nr[round] = (double)nr; }
    }
}

// What the host's replay needs of the loop's state -- the head, 16 bytes per node of the candidate tree and the nodes' centres --
// stored straight into pinned host memory by one launch (three copy-engine transfers of the full-capacity arrays before)
__global__ __launch_bounds__(256) void k_lq_export(const LqCtl *c, LqHead *head, LqRec *rec, LqCen *cen) {
    const int nn = c->h.nnodes;
    const int t = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int i = t; i < nn; i += stride) { rec[i] = c->nrec[i]; cen[i] = c->ncen[i]; }
    const double *src = reinterpret_cast<const double *>(&c->h);
    double *dst = reinterpret_cast<double *>(head);
    for (int i = t; i < (int)(sizeof(LqHead) / sizeof(double)); i += stride) dst[i] = src[i];
}

// the split trace's records of a device-driven call, made when somebody asks for them (patolette_amd_last_split_trace): one thread
// per commit of the replay
__global__ void k_lq_trace(const NodeDev *nodes, const LqCommit *commits, int n, patolette_amd__SplitRecord *out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const LqCommit cm = commits[t];
    const NodeDev &h = nodes[cm.node], &hl = nodes[cm.left], &hr = nodes[cm.left + 1];
    patolette_amd__SplitRecord tr;
    tr.row = cm.row; tr.new_row = cm.new_row;
    tr.split = hl.psplit < 0 ? -1 : (hl.psplit & 0xffff); tr.degenerate = hl.psplit < 0 ? 0 : (hl.psplit >> 16) & 1;
    tr.n = h.gn; tr.n_left = hl.gn; tr.n_right = hr.gn; tr.sw = h.sw;
    for (int j = 0; j < 3; j++) tr.axis[j] = h.axis[j];
    for (int q = 0; q < 6; q++) tr.cov6[q] = h.cov6[q] / h.sw;
    tr.dist = h.dist; tr.dist_left = hl.dist; tr.dist_right = hr.dist; tr.benefit = h.dist - (hl.dist + hr.dist);
    out[t] = tr;
}

// what k_round_setup does from the host's packet, from the control kernel's lists: cleared outputs of the round's nodes, both tile
// lists, zeroed histograms
__global__ __launch_bounds__(256) void k_round_setup_dyn(NodeDev *table, const LqCtl *c, Tile *tilesA, Tile *tilesP, double *hist,
                                                         unsigned long long *hsize, unsigned int *hcount, const size_t lqs) {
    const int nr = c->dyn.nr;
    if (nr == 0) return;
    const int ntA = c->dyn.ntA, ntP = c->dyn.ntP;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < (size_t)nr * kNodeResetElems; i += stride)
        node_reset_element(table[c->round_ids[i / kNodeResetElems]], (int)(i % kNodeResetElems));
    for (size_t t = tid; t < (size_t)ntA; t += stride) {
        const int r = node_of_tile(c->tA0, nr, (int)t);
        const NodeDev &d = table[c->round_ids[r]];
        const unsigned long long o = (unsigned long long)((int)t - c->tA0[r]) * kTileA, n = d.n;
        tilesA[t] = Tile{d.begin + o, (unsigned)(n - o < (unsigned long long)kTileA ? n - o : kTileA), (unsigned)c->round_ids[r]};
    }
    for (size_t t = tid; t < (size_t)ntP; t += stride) {
        const int r = node_of_tile(c->tP0, nr, (int)t);
        const NodeDev &d = table[c->round_ids[r]];
        const unsigned long long o = (unsigned long long)((int)t - c->tP0[r]) * kTileP, n = d.n;
        tilesP[t] = Tile{d.begin + o, (unsigned)(n - o < (unsigned long long)kTileP ? n - o : kTileP), (unsigned)c->round_ids[r]};
    }
    for (size_t i = tid; i < lqs * (size_t)nr; i += stride) hist[i] = 0.0;
    for (size_t i = tid; i < (size_t)nr * kBuckets; i += stride) { hsize[i] = 0ULL; hcount[i] = 0u; }
}

// =============================================================================================
// The global quantiser's decisions on the DEVICE (global.c:189-298, cells.c:114-328; round 6)
// =============================================================================================
// Before: eleven DP launches for every k up to 12, three downloads, the host's prefix sums, bias test and backtrack, an upload of
// the bucket -> cluster table and of the base clusters' records: ~50 us of launches and ~150 us of idle GPU in every call.  Here ONE
// block does what the host did, in the host's own arithmetic (the same expressions in the same order on the same sums; the
// eigen-solver is hm::eigen_sym3, compiled for both sides), and the partition follows on the stream without the host looking:
//   1. the eleven inclusive prefixes of the 512-bucket table, each a sequential chain as cells.c:114-136 builds them (one wavefront
//      per chain, out of LDS);
//   2. the principal axis of all buckets (cells.c:225-278);
//   3. for k = 2 .. 12: the bias termination test on the current cells (global.c:99-187; one wavefront per cell solves its 3x3, one
//      thread adds up in order), then -- only if the search goes on -- the DP (global.c:232-280): a FULL step k-1 (sixteen
//      wavefronts, one entry each at a time) and the single entry cut[k][512] the backtrack starts from.  The reference fills the
//      whole table first; what it reads of it is this.  Same candidates, same strict '<' in descending t (the largest t among equal
//      minima, t = n-1 first), so the cuts are the reference's.  Noise and most photographs stop at two cells: no full step at all;
//   4. the bucket -> base cluster table (global.c:328-335) and the base clusters' node records (count, weight, mean from the exact
//      bucket sums), the root's children.
// patolette_amd__SplitTrace's header and the host-driven split loop read GqOut after their next synchronisation.
struct GqTab {                                          // LDS: inclusive prefixes, 1-based (hm::CellMoments)
    unsigned long long w0[kBuckets + 1];
    double t[10][kBuckets + 9];                         // 0..2 w1[r], 3 w2, 4..9 wrs (00,01,11,02,12,22); + 8: the chains read ahead
    __device__ double distortion(int a, int b) const {  // cells.c:141-182
        if (w0[a] == w0[b]) return 0;
        const double q0 = t[0][b] - t[0][a], q1 = t[1][b] - t[1][a], q2 = t[2][b] - t[2][a];
        return t[3][b] - t[3][a] - (q0 * q0 + q1 * q1 + q2 * q2) / (double)(w0[b] - w0[a]);
    }
    __device__ double vcov(int a, int b, int r, int s) const {   // cells.c:184-223
        if (w0[a] == w0[b]) return 0;
        const double cnt = (double)(w0[b] - w0[a]);
        const int rs = 4 + s * (s + 1) / 2 + r;
        return (t[rs][b] - t[rs][a]) / cnt - (t[r][b] - t[r][a]) * (t[s][b] - t[s][a]) / (cnt * cnt);
    }
    __device__ bool axis(int a, int b, double ax[3]) const {     // cells.c:225-278
        double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int s = 0; s < 3; s++) for (int r = 0; r <= s; r++) m[s * 3 + r] = vcov(a, b, r, s);
        m[0 * 3 + 2] = m[2 * 3 + 0]; m[0 * 3 + 1] = m[1 * 3 + 0]; m[1 * 3 + 2] = m[2 * 3 + 1];
        double w[3];
        if (hm::eigen_sym3(m, w) != 0) return false;
        ax[0] = m[6]; ax[1] = m[7]; ax[2] = m[8];
        return true;
    }
    __device__ static double norm3(const double a[3]) { double s = 0; for (int i = 0; i < 3; i++) s += a[i] * a[i]; return sqrt(s); }   // pow(x, 2) is x * x
    __device__ double bias(int a, int b, const double ax[3]) const {   // cells.c:280-328
        double ca[3];
        if (!axis(a, b, ca)) return -1;
        const double norms = norm3(ax) * norm3(ca);
        if (norms < 1e-16) return 0;
        const double dot = (ca[0] * ax[0] + ca[1] * ax[1] + ca[2] * ax[2]);
        return fmin(1.0, fabs(dot / norms));
    }
};

// the inclusive prefixes, 1-based, as a test reads them back (patolette_amd_debug_gq_table): w0, then w1[0..2], w2, wrs[0..5]
struct GqPrefixes { unsigned long long w0[kBuckets + 1]; double t[10][kBuckets + 1]; };

// entry (k, n) of the DP by ONE wavefront (k_gq_dp's block, quant.hip): E_k[n] and L[k][n] from Ep = E_{k-1}
__device__ __forceinline__ void gq_dp_entry(const GqTab &c, const double *Ep, const int k, const int n, const int lane, double &e_out, int &cut_out) {
    double best = INFINITY; int bt = -1;
    for (int t = n - 2 - lane; t >= k - 1; t -= 64) {
        const double v = Ep[t] + c.distortion(t, n);
        if (v < best) { best = v; bt = t; }                          // descending t within the lane: first minimum = largest t
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_down(best, o, 64); const int t2 = __shfl_down(bt, o, 64);
        if (t2 >= 0 && (bt < 0 || v2 < best || (v2 == best && t2 > bt))) { best = v2; bt = t2; }
    }
    double e = Ep[n - 1]; int cut = n - 1;
    if (bt >= 0 && best < e) { e = best; cut = bt; }
    e_out = e; cut_out = cut;                                        // (lane 0 holds the wavefront's result)
}

__global__ __launch_bounds__(1024) void k_gq_control(const double *__restrict__ hist, const unsigned int *__restrict__ hcount, GqDpDev *g,
                                                     const int palette_size, const int weighted, NodeDev *nodes, const int base0,
                                                     unsigned char *lut, GqOut *out, GqOut *out_host, GqPrefixes *dbg_prefixes) {
    __shared__ GqTab c;
    __shared__ double E[2][kBuckets + 1];
    __shared__ int s_q[16], s_nq, s_stop, s_err, s_top;
    __shared__ double s_ax[3], s_cd[16], s_cb[16];
    __shared__ unsigned char s_lut[kBuckets];
    __shared__ double s_part[kGqMaxK][4][2];
    __shared__ unsigned long long s_cnt[kGqMaxK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ unsigned long long s_ticks[8];
    if (tid == 0) { for (int i = 0; i < 8; i++) s_ticks[i] = 0; s_ticks[0] = wall_clock64(); }
    // ---- 1. prefixes
    for (int i = tid; i < 10 * kBuckets; i += 1024) {
        const int hq = i / kBuckets, b = i - hq * kBuckets;
        c.t[hq][b + 1] = hist[(size_t)(hq * 2 + 0) * kBuckets + b] + hist[(size_t)(hq * 2 + 1) * kBuckets + b];
    }
    for (int b = tid; b < kBuckets; b += 1024) c.w0[b + 1] = hcount[b];
    if (tid < 10) c.t[tid][0] = 0;
    if (tid == 10) c.w0[0] = 0;
    __syncthreads();
    if (tid == 0) s_ticks[5] = wall_clock64();
    if (wv < 10) {
        // table[i] += table[i-1], i ascending: ONE sequential chain of 512 additions per table (cells.c:114-136), in registers.  Lane l
        // holds entries 8 l + 1 .. 8 l + 8.  Pass A walks the lanes in order -- every lane adds its eight entries to the running sum
        // it is handed (only lane l's are the chain's; the others' work is discarded) and the sum after lane l's entries goes on to
        // lane l + 1 through a scalar register; pass B lets every lane redo ITS eight additions from the sum it was handed: the same
        // operands in the same order, so the same bits.  (Through LDS, one lane per chain: ten wavefronts' loads and stores queued
        // on the CU's one LDS pipeline, 23 us; k_gq_prefix's chains, with a round trip per step, 16 us for five.)
        double *t = c.t[wv];
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = t[1 + lane * 8 + u];
        double carry = 0, cin = 0;
        for (int l = 0; l < 64; l++) {
            double a = carry;
#pragma unroll
            for (int u = 0; u < 8; u++) a = v[u] + a;
            cin = lane == l ? carry : cin;
            carry = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(a), l), __builtin_amdgcn_readlane(__double2loint(a), l));
        }
        double a = cin;
#pragma unroll
        for (int u = 0; u < 8; u++) { a = v[u] + a; t[1 + lane * 8 + u] = a; }
    }
    if (wv == 10) {                                                  // the counts: integers, any order -- a wave scan, eight buckets per lane
        unsigned long long v[8], run = 0;
#pragma unroll
        for (int u = 0; u < 8; u++) { run += c.w0[1 + lane * 8 + u]; v[u] = run; }
        unsigned long long inc = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        const unsigned long long before = inc - run;
#pragma unroll
        for (int u = 0; u < 8; u++) c.w0[1 + lane * 8 + u] = before + v[u];
    }
    __syncthreads();
    if (dbg_prefixes) {                                              // tests only (patolette_amd_debug_gq_table): the prefixes as the search reads them
        for (int i = tid; i <= kBuckets; i += 1024) dbg_prefixes->w0[i] = c.w0[i];
        for (int i = tid; i < 10 * (kBuckets + 1); i += 1024) { const int q = i / (kBuckets + 1), n = i - q * (kBuckets + 1); dbg_prefixes->t[q][n] = c.t[q][n]; }
    }
    if (tid == 0) s_ticks[1] = wall_clock64();
    // ---- 2. the axis of everything, E_1; L as the reference starts it (zero, L[i][i] = i: global.c:236-238)
    for (int i = tid; i < (kGqMaxK + 1) * (kBuckets + 1); i += 1024) { const int r = i / (kBuckets + 1), n = i - r * (kBuckets + 1); g->cut[r][n] = r == n ? r : 0; }
    for (int i = tid; i <= kBuckets; i += 1024) E[1][i] = i >= 1 ? c.distortion(0, i) : 0.0;
    if (tid == 0) {
        double ax[3] = {0, 0, 0};
        s_err = c.axis(0, kBuckets, ax) ? 0 : 1;
        s_ax[0] = ax[0]; s_ax[1] = ax[1]; s_ax[2] = ax[2];
        s_q[0] = 0; s_q[1] = kBuckets; s_nq = 2; s_stop = 0;
    }
    __syncthreads();
    const int kmax = palette_size < kGqMaxK ? palette_size : kGqMaxK;
    if (tid == 0) s_ticks[2] = wall_clock64();
    // ---- 3. E[k & 1 ^ 1] ... : E[(k - 1) & 1] holds E_{k-1} when iteration k reaches its DP
    for (int k = 2; k <= kmax && !s_err; k++) {
        const int cells = s_nq - 1;
        if (lane == 0 && wv < cells) {
            const double ax[3] = {s_ax[0], s_ax[1], s_ax[2]};
            s_cd[wv] = c.distortion(s_q[wv], s_q[wv + 1]);
            if (cells == 1) {                                        // the one cell is everything: its axis is `ax`, solved a moment ago
                const double norms = GqTab::norm3(ax) * GqTab::norm3(ax);
                s_cb[wv] = norms < 1e-16 ? 0.0 : fmin(1.0, fabs((ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) / norms));
            } else s_cb[wv] = c.bias(s_q[wv], s_q[wv + 1], ax);
        }
        __syncthreads();
        if (tid == 0) {                                              // gq_should_terminate (global.c:99-187)
            double distortion = 0;
            for (int j = 0; j < cells; j++) distortion += s_cd[j];
            int stop = 0;
            if (distortion < 1e-16) stop = 1;
            else {
                double bias = 0;
                for (int i = 0; i < cells; i++) {
                    const double cd = s_cd[i], cb = s_cb[i];
                    if (cb < 0) { stop = 1; break; }                 // (global.c:174-177 sets a flag its caller never reaches: the loop breaks first)
                    if (cb < 0.9) continue;
                    bias += (cd / distortion) * cb;
                }
                if (!stop) stop = bias < 0.1 ? 1 : 0;
            }
            s_stop = stop;
        }
        __syncthreads();
        if (s_stop) break;
        if (k > 2) {                                                 // the full step k-1: E_{k-1} and L[k-1][.] from E_{k-2}
            const int kk = k - 1;
            const double *Ep = E[(kk - 1) & 1];
            double *En = E[kk & 1];
            for (int n = wv; n <= kBuckets; n += 16) {                   // (sixteen wavefronts: the launch is 1024 threads, launch_bounds above)
                if (n < kk + 1) { if (lane == 0) En[n] = Ep[n]; continue; }
                double e; int cut;
                gq_dp_entry(c, Ep, kk, n, lane, e, cut);
                if (lane == 0) { En[n] = e; g->cut[kk][n] = cut; }
            }
            __syncthreads();
        }
        if (wv == 0) {
            double e; int cut;
            gq_dp_entry(c, E[(k - 1) & 1], k, kBuckets, lane, e, cut);
            if (lane == 0) s_top = cut;
        }
        __syncthreads();
        if (tid == 0) {                                              // the backtrack (global.c:282-296)
            int t = s_top;
            s_q[k - 1] = t;
            for (int j = k - 2; j >= 1; j--) { t = g->cut[j + 1][t]; s_q[j] = t; }
            s_q[0] = 0; s_q[k] = kBuckets; s_nq = k + 1;
        }
        __syncthreads();
    }
    const int kbase = s_nq - 1;
    if (tid == 0) s_ticks[3] = wall_clock64();
    // ---- 4. bucket -> base cluster (global.c:328-335), the clusters' records
    for (int b = tid; b < kBuckets; b += 1024) {
        int j = 0;
        while (j < kbase - 1 && !(b + 1 <= s_q[j + 1])) j++;
        s_lut[b] = (unsigned char)j;
        lut[b] = (unsigned char)j;
    }
    __syncthreads();
    const int nq = weighted ? 4 : 3;
    // the clusters' sums: wavefront (q, part) holds its row of the table, eight buckets per lane, and adds up every cluster's share
    // (exact parts on the bin grids: any order); wavefront 8 the counts
    if (wv < 2 * nq) {
        const int q = wv >> 1, part = wv & 1, qi = weighted ? 10 + q : q;
        const double *h = hist + (size_t)(qi * 2 + part) * kBuckets + lane * 8;
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = h[u];
        for (int j = 0; j < kbase; j++) {
            double a = 0;
#pragma unroll
            for (int u = 0; u < 8; u++) a += s_lut[lane * 8 + u] == j ? v[u] : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            if (lane == 0) s_part[j][q][part] = a;
        }
    } else if (wv == 8) {
        unsigned long long v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = hcount[lane * 8 + u];
        for (int j = 0; j < kbase; j++) {
            unsigned long long a = 0;
#pragma unroll
            for (int u = 0; u < 8; u++) a += s_lut[lane * 8 + u] == j ? v[u] : 0ULL;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            if (lane == 0) s_cnt[j] = a;
        }
    }
    __syncthreads();
    if (tid < kbase) {
        const int j = tid;
        unsigned long long pos = 0;
        for (int i = 0; i < j; i++) pos += s_cnt[i];
        const unsigned long long cnt = s_cnt[j];
        NodeDev &ch = nodes[base0 + j];
        ch.begin = pos; ch.n = cnt; ch.gn = cnt; ch.buf = 1; ch.slot = -1; ch.child0 = -1; ch.nchild = 0;
        const double sw = weighted ? (s_part[j][3][0] + s_part[j][3][1]) : (double)cnt;
        const double inv = 1 / sw;
        for (int q = 0; q < 3; q++) { ch.axis[q] = 0; ch.mean[q] = (s_part[j][q][0] + s_part[j][q][1]) * inv; }
        ch.sw = sw; ch.klin = nodes[0].klin; ch.kquad = nodes[0].kquad;
        node_reset_outputs(ch);
        ch.split = -1; ch.psplit = -1;
    }
    if (tid == 64) {
        NodeDev &root = nodes[0];
        root.child0 = base0; root.nchild = kbase;
        root.split = kbase == 2 ? s_q[1] - 1 : -1;                   // bucket b is in cluster 0 iff b + 1 <= cuts[1] (global.c:328-335)
        GqOut o;
        o.kbase = kbase; o.error = s_err; o.pad[0] = o.pad[1] = 0;
        for (int j = 0; j < 16; j++) o.cuts[j] = j <= kbase ? s_q[j] : 0;
        for (int j = 0; j < 8; j++) o.ticks[j] = s_ticks[j];
        o.ticks[4] = wall_clock64();
        *out = o;
        *out_host = o;                                               // pinned host memory: read after the caller's next synchronisation
    }
}

// the eigen-solver as the control kernel runs it, for the golden test (patolette_amd_eigen_sym3_device)
__global__ void k_eigen_batch(const double *a9, size_t count, double *w3, double *z9, int *info) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double a[9], w[3];
    for (int j = 0; j < 9; j++) a[j] = a9[i * 9 + j];
    info[i] = hm::eigen_sym3(a, w);
    for (int j = 0; j < 3; j++) w3[i * 3 + j] = w[j];
    for (int j = 0; j < 9; j++) z9[i * 9 + j] = a[j];
}

// ---- one image over several GPUs (patolette_amd_slice): the node table's reductions, packed for ONE collective ----
// The caller's collective is an element-wise SUM.  Extrema and per-rank counts travel in a table with one row per rank
// (zero except the sender's own row): after the SUM every rank holds every rank's row and takes the minimum, the maximum
// and the number of members on lower ranks (the node-wide slot of its first member: sort.c:61-79's round-robin rule).
__global__ void k_shard_pack_keys(const NodeDev *table, const int *ids, int n, int rank, int size, unsigned long long *buf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const NodeDev &d = table[ids[i]];
    unsigned long long a = ~0ULL, b = 0ULL;
    for (int k = 0; k < kSlots; k++) { a = d.minkey[k] < a ? d.minkey[k] : a; b = d.maxkey[k] > b ? d.maxkey[k] : b; }
    for (int r = 0; r < size; r++) {
        unsigned long long *row = buf + ((size_t)r * n + i) * 3;
        row[0] = r == rank ? a : 0ULL; row[1] = r == rank ? b : 0ULL; row[2] = r == rank ? d.n : 0ULL;
    }
}
__global__ void k_shard_unpack_keys(NodeDev *table, const int *ids, int n, int rank, int size, const unsigned long long *buf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    NodeDev &d = table[ids[i]];
    unsigned long long a = ~0ULL, b = 0ULL, before = 0ULL;
    for (int r = 0; r < size; r++) {
        const unsigned long long *row = buf + ((size_t)r * n + i) * 3;
        a = row[0] < a ? row[0] : a; b = row[1] > b ? row[1] : b;
        if (r < rank) before += row[2];
    }
    for (int k = 0; k < kSlots; k++) { d.minkey[k] = ~0ULL; d.maxkey[k] = 0ULL; }
    d.minkey[0] = a; d.maxkey[0] = b; d.gslot0 = before;
}
// centred moments: slot sums are exact (binned parts), so is their SUM over the ranks
__global__ void k_shard_pack_acc(const NodeDev *table, const int *ids, int n, double *buf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const NodeDev &d = table[ids[i]];
    for (int q = 0; q < 7; q++) {
        double s0 = 0, s1 = 0;
        for (int k = 0; k < kSlots; k++) { s0 += d.acc[k][q][0]; s1 += d.acc[k][q][1]; }
        buf[(size_t)i * 14 + 2 * q] = s0; buf[(size_t)i * 14 + 2 * q + 1] = s1;
    }
}
__global__ void k_shard_unpack_acc(NodeDev *table, const int *ids, int n, const double *buf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    NodeDev &d = table[ids[i]];
    for (int q = 0; q < 7; q++) {
        for (int k = 1; k < kSlots; k++) { d.acc[k][q][0] = 0; d.acc[k][q][1] = 0; }
        d.acc[0][q][0] = buf[(size_t)i * 14 + 2 * q]; d.acc[0][q][1] = buf[(size_t)i * 14 + 2 * q + 1];
    }
}
// k_cut / the host sized the children from the GROUP's bucket counts; their segments on this GPU are what k_scan found
__global__ void k_shard_children_local(NodeDev *table, const int *round_nodes, int nround) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nround) return;
    const NodeDev &nd = table[round_nodes[i]];
    for (int k = 0; k < nd.nchild; k++) {
        NodeDev &ch = table[nd.child0 + k];
        ch.begin = nd.cbegin[k]; ch.n = nd.cbegin[k + 1] - nd.cbegin[k];
    }
}

struct Bounds {
    double cmax, range, wmax; int e_lin, e_quad; double lo[3], hi[3];
    bool have_sum = false; double sum[3] = {0, 0, 0};        // column sums of the converted image, when the conversion took them
    bool have_mom = false;                                   // ... and the raw second moments with them: both as exact (hi, lo) pairs
    double sum2[3][2] = {{0, 0}, {0, 0}, {0, 0}}, mom2[6][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
    bool nonfinite = false;                                  // a converted value is NaN / Inf as f32 (KMeans then leaves the centres alone)
    double wmin = 0; bool bad_w = false;                     // the smallest positive weight as f32 (0: none), a negative / NaN / Inf weight
};

static int exp_bound(double v) {                 // smallest E with 2^E > v (v > 0)
    if (!(v > 0) || !std::isfinite(v)) return 1;
    return std::ilogb(v) + 1;
}

// --------------------------------------------------------------------------------------------
struct Shard {                       // this GPU's part of an image dealt out over a group (patolette_amd_slice)
    size_t total = 0, begin = 0;     // pixels of the whole image; first pixel of the slice
    patolette_amd__Comm comm{};
};

struct Engine {
    int device = -1;
    hipStream_t stream = nullptr;
    const Shard *shard = nullptr;    // set for the duration of a sliced call
    bool invariant = false;          // tiling-invariant children moments (always on while `shard` is set); a property of the CALLING
                                     // THREAD (tl_invariant), copied in whenever an engine starts serving a thread or a batch
    DevBuf<unsigned char> commbuf;
    PinBuf<unsigned char> h_comm;
    DevBuf<int> shard_ids;
    PinBuf<float> h_cent;            // KMeans centroids on their way to / from the device
    PinBuf<ConvertStats> h_cstats;
    hipEvent_t ev_stats = nullptr;
    hipStream_t stream2 = nullptr;        // run_host: the conversion of chunk i runs here while chunk i + 1 is on its way up
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_join = nullptr;
    size_t prep_N = 0, prep_planes = 0;   // gq_prepare() has staged the root's tiles and cleared the tables for an image of this size
    DevBuf<double> src, wsrc, cvt, bufA, bufB, aux;
    DevBuf<unsigned short> bkt;
    DevBuf<NodeDev> nodes;
    DevBuf<NodeIn> stage_in;
    DevBuf<NodeOut> stage_out;
    DevBuf<int> ids, round_nodes, node_tile0;
    DevBuf<Tile> tilesA, tilesP;
    DevBuf<double> hist, sum6, dpal;
    DevBuf<unsigned long long> hsize, tileoff;
    DevBuf<unsigned int> hcount, tilecnt;
    DevBuf<unsigned char> lut, dmap, src8, pal8, quant8;
    DevBuf<unsigned char> dl_maps, dl_shown;     // frame deltas from host maps: the maps (the deltas replace them in place), the shown maps
    DevBuf<unsigned long long> dl_words, dl_masks;   // ... the kernels' boxes, counts and flag; the ballots between them (delta.h)
    DevBuf<unsigned> dl_rows;                    // ... per-frame palettes: every table's rows, a word each, then the frames' tables
    DevBuf<unsigned long long> ms_words;         // measure: the entries' slots, the flag and the folded results (measure.h)
    DevBuf<MeasureTile> ms_tiles;                // ... the tiles' records between its two kernels
    DevBuf<unsigned> ms_p8;                      // ... the palette's bytes, a word per row
    DevBuf<LzwFrame> lz_frames;                  // gif_lzw: the frames' rectangles and first segments (lzw.h)
    DevBuf<unsigned> lz_stage, lz_bits, lz_out;  // ... the segments' staging areas and bit lengths; the packed streams
    DevBuf<unsigned long long> lz_gbit, lz_words;   // ... every segment's first bit in the output; the flag and the frames' offsets
    DevBuf<unsigned char> lz_near;               // gif_lzw_lossy: the table of near colours (lzw_near.h)
    DevBuf<unsigned char> df_stream;             // png_deflate: the frames' filtered streams, back to back (deflate.h)
    DevBuf<unsigned long long> df_base;          // ... the frames' first bytes in them
    DevBuf<unsigned> df_tokens;                  // ... the segments' tokens between parse and emit
    // the RGBA entry (run_rgba): tile counts / offsets + the opaque count, each pixel's compact number, the opaque pixels' RGB and
    // weights, the full index map on its way to the host, the count's pinned landing place
    DevBuf<unsigned> rgba_cnt;
    DevBuf<int> rgba_cpos;
    DevBuf<unsigned char> rgba_rgb, rgba_map;
    DevBuf<double> rgba_w;
    PinBuf<unsigned> h_rgba_m;
    // the remap with alpha (run_remap_rgba): the stamp's flag and, behind it, every frame's opaque count; their pinned landing place
    DevBuf<unsigned> rr_words;
    PinBuf<unsigned> h_rr_words;
    // the colour histogram (hist.h): the weights as units; the weights' flag, the totals and the export's count; the export's tile
    // offsets; the exported rows (bytes, counts, weights)
    DevBuf<unsigned long long> hs_units, hs_words, hs_counts;
    DevBuf<unsigned> hs_tiles;
    DevBuf<unsigned char> hs_rgb;
    DevBuf<double> hs_w;
    DevBuf<ConvertStats> cstats;
    PinBuf<NodeIn> h_stage_in;
    PinBuf<NodeOut> h_stage_out;
    PinBuf<int> h_ids, h_ids_get;
    PinBuf<int> h_round;
    PinBuf<double> h_dbl;
    PinBuf<unsigned char> h_bytes, h_packet, h_mapstage;
    DevBuf<unsigned char> packet;
    KMeansWork km;
    NNWork nn;
    SalWork sal;
    DevBuf<double> wsal;
    DevBuf<GqDpDev> gq;
    PinBuf<GqDpDev> h_gq;
    DevBuf<GqOut> gqout;                  // k_gq_control's result (device copy: the split loop's kernels read it; pinned copy: the host, after its next synchronisation)
    PinBuf<GqOut> h_gqout;
    PinBuf<double> h_pal;                 // the palette on its way to the mapping kernels
    DevBuf<LqCtl> lqctl;                  // the device-driven split loop's state; the host's copies of what the replay needs
    PinBuf<LqHead> h_lqhead;
    PinBuf<LqRec> h_lqrec;
    PinBuf<LqCen> h_lqcen;
    std::vector<LqRec> lq_rec_local;      // the replay's table, copied out of the pinned buffer
    std::vector<LqCommit> lq_commits;     // the replay's commits of the last device-driven call: the split trace is made from them on request
    bool trace_pending = false;
    size_t lq_hint_N = 0, lq_hint_K = 0; int lq_hint_rounds = 0;   // rounds the last image of this size and palette needed
    // KMeans subsample list = a prefix of rand_perm(N, seed 1234) (Clustering.cpp:311-319): a pure function of N, and the list
    // for FEWER samples is a prefix of the list for more.  perm_dev holds the first perm_nx entries for an image of perm_N pixels;
    // h_perm (pinned) the first hperm_nx for hperm_N, written by a helper thread (perm_job) that starts at call entry and is
    // waited for when the KMeans stage needs the list -- by then conversion and both quantisers have run (subsample_start/_list)
    DevBuf<int> perm_dev;
    size_t perm_N = 0, perm_nx = 0;
    PinBuf<int32_t> h_perm;
    size_t hperm_N = 0, hperm_nx = 0;
    hm::PermScratch perm_ws;          // the helper's tables (kept: no page faults after the first call)
    std::future<void> perm_job;
    patolette_amd__Stats stats{};
    double ms_saliency = 0.0;
    std::string last_error;
    std::vector<double> map_palette;             // the palette as the mapping stage used it (planar (len,3)): Rec2020 / ICtCp / sRGB
    // what the quantisers of the last call decided (patolette_amd_last_split_trace): a few hundred small records, always kept
    patolette_amd__SplitTrace trace_hdr{};
    std::vector<patolette_amd__SplitRecord> trace;
    std::vector<double> cluster_centers;         // PALETTE_create's rows, planar (len,3), before any KMeans

    void init() {
        if (stream) return;
        int cnt = 0;
        if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
            throw HipError("patolette_amd: no HIP device available (this library has no CPU fallback)");
        if (device < 0) { HIP_CHECK(hipGetDevice(&device)); }
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
    void sync() { HIP_CHECK(hipStreamSynchronize(stream)); if (ktimer().enabled) ktimer().collect(); }
    ~Engine() {                                  // buffers free themselves (DevBuf / PinBuf); only called while the runtime is alive
        if (stream) { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); if (ev_stats) (void)hipEventDestroy(ev_stats);
                      for (hipEvent_t e : {ev_up[0], ev_up[1], ev_join}) if (e) (void)hipEventDestroy(e);
                      if (stream2) (void)hipStreamDestroy(stream2);
                      (void)hipStreamDestroy(stream); }
    }
};

// Engines (HIP stream + ~170 bytes of workspace per pixel of the largest image seen) are pooled per device: a thread
// takes one at its first call and hands it back when it exits (no HIP call at thread or process exit: the runtime may
// already be shutting down), so short-lived caller threads neither leak a workspace each nor pay for a new one.
// patolette_amd_release_workspace() gives the memory back.
namespace {
std::mutex g_pool_mu;
std::vector<Engine *> g_pool;
// patolette_amd_set_invariant_sums: the caller's setting lives with the calling thread, not with a pooled engine (an engine
// outlives the thread it served and is handed to others).  -1 = not set: the environment's default.
thread_local int tl_invariant = -1;
bool invariant_default() {
    static const bool env = getenv("PAMD_INVARIANT_SUMS") && atoi(getenv("PAMD_INVARIANT_SUMS")) != 0;
    return tl_invariant < 0 ? env : tl_invariant != 0;
}
Engine *pool_acquire(int device, bool invariant) {   // device < 0: the current device is unknown -> only an engine bound to no GPU yet
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool.size(); i++)
            if (g_pool[i]->device == device || g_pool[i]->device < 0) {
                Engine *e = g_pool[i];
                g_pool.erase(g_pool.begin() + i);
                if (e->device < 0) e->device = device;
                e->invariant = invariant;
                return e;
            }
    }
    Engine *e = new Engine;
    e->device = device;
    e->invariant = invariant;
    return e;
}
void pool_release(Engine *e) { std::lock_guard<std::mutex> lk(g_pool_mu); g_pool.push_back(e); }
struct EngineHolder {
    Engine *e = nullptr;
    ~EngineHolder() { if (e) pool_release(e); }
};
EngineHolder &holder() { static thread_local EngineHolder h; return h; }
}  // namespace

static Engine &engine() {
    EngineHolder &h = holder();
    if (!h.e) {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
        h.e = pool_acquire(dev, invariant_default());
    }
    return *h.e;
}

// ---- the group's collective (element-wise in-place SUM lent by the caller) ----
static size_t comm_elem(int dtype) { return dtype == 2 ? 4 : 8; }
static void comm_sum_dev(Engine &E, void *d, size_t count, int dtype) {         // d: device memory
    if (!count) return;
    HIP_CHECK(hipStreamSynchronize(E.stream));
    const patolette_amd__Comm &c = E.shard->comm;
    int rc;
    if (c.host_buffers) {
        const size_t bytes = count * comm_elem(dtype);
        E.h_comm.reserve(bytes);
        HIP_CHECK(hipMemcpy(E.h_comm.p, d, bytes, hipMemcpyDeviceToHost));
        rc = c.allreduce_sum(c.ctx, E.h_comm.p, count, dtype);
        HIP_CHECK(hipMemcpy(d, E.h_comm.p, bytes, hipMemcpyHostToDevice));
    } else rc = c.allreduce_sum(c.ctx, d, count, dtype);
    if (rc != 0) throw HipError("patolette_amd: the caller's all-reduce reported a failure");
}
static void comm_sum_host(Engine &E, void *h, size_t count, int dtype) {        // h: host memory
    if (!count) return;
    const patolette_amd__Comm &c = E.shard->comm;
    const size_t bytes = count * comm_elem(dtype);
    int rc;
    if (c.host_buffers) rc = c.allreduce_sum(c.ctx, h, count, dtype);
    else {
        E.commbuf.reserve(bytes);
        HIP_CHECK(hipMemcpy(E.commbuf.p, h, bytes, hipMemcpyHostToDevice));
        rc = c.allreduce_sum(c.ctx, E.commbuf.p, count, dtype);
        HIP_CHECK(hipMemcpy(h, E.commbuf.p, bytes, hipMemcpyDeviceToHost));
    }
    if (rc != 0) throw HipError("patolette_amd: the caller's all-reduce reported a failure");
}
// every rank's row of n values (bit patterns travel as i64: one non-zero addend per element)
static std::vector<unsigned long long> comm_gather_u64(Engine &E, const unsigned long long *mine, size_t n) {
    const patolette_amd__Comm &c = E.shard->comm;
    std::vector<unsigned long long> all((size_t)c.size * n, 0ULL);
    for (size_t i = 0; i < n; i++) all[(size_t)c.rank * n + i] = mine[i];
    comm_sum_host(E, all.data(), all.size(), 1);
    return all;
}
// projection extrema + member counts of the nodes whose ids sit at d_ids (device): folded, exchanged, written back
static void shard_exchange_keys(Engine &E, const int *d_ids, int n) {
    if (!n) return;
    const patolette_amd__Comm &c = E.shard->comm;
    const size_t cnt = (size_t)c.size * n * 3;
    E.commbuf.reserve(cnt * 8);
    hipLaunchKernelGGL(k_shard_pack_keys, (n + 63) / 64, 64, 0, E.stream, E.nodes.p, d_ids, n, c.rank, c.size, (unsigned long long *)E.commbuf.p);
    HIP_CHECK(hipGetLastError());
    comm_sum_dev(E, E.commbuf.p, cnt, 1);
    hipLaunchKernelGGL(k_shard_unpack_keys, (n + 63) / 64, 64, 0, E.stream, E.nodes.p, d_ids, n, c.rank, c.size, (const unsigned long long *)E.commbuf.p);
    HIP_CHECK(hipGetLastError());
}
static void shard_exchange_acc(Engine &E, const int *d_ids, int n) {
    if (!n) return;
    E.commbuf.reserve((size_t)n * 14 * 8);
    hipLaunchKernelGGL(k_shard_pack_acc, (n + 63) / 64, 64, 0, E.stream, E.nodes.p, d_ids, n, (double *)E.commbuf.p);
    HIP_CHECK(hipGetLastError());
    comm_sum_dev(E, E.commbuf.p, (size_t)n * 14, 0);
    hipLaunchKernelGGL(k_shard_unpack_acc, (n + 63) / 64, 64, 0, E.stream, E.nodes.p, d_ids, n, (const double *)E.commbuf.p);
    HIP_CHECK(hipGetLastError());
}
static const int *shard_upload_ids(Engine &E, const std::vector<int> &ids) {
    E.shard_ids.reserve(ids.size());
    HIP_CHECK(hipStreamSynchronize(E.stream));
    HIP_CHECK(hipMemcpy(E.shard_ids.p, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice));
    return E.shard_ids.p;
}

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// host mirror of one tree node
struct HNode {
    unsigned long long begin = 0, n = 0;     // segment on this GPU
    unsigned long long gn = 0;               // members over the whole group (= n unless the image is sliced over GPUs)
    int buf = 0;
    double sw = 0, mean[3] = {0, 0, 0}, cov6[6] = {0, 0, 0, 0, 0, 0}, dist = 0;
    int left = -1, right = -1;
    int psplit = -1;                         // the parent's cut as the device took it (bucket | degenerate << 16): split trace
    bool split_done = false, nosplit = false;
    // filled when the moments arrive (leaf_bound): the principal axis (dsyev semantics) and an upper bound of the benefit
    // of ANY split of the node
    int axis_state = 0;                      // 0 not solved yet, 1 axis valid, -1 the solver failed (-> nosplit when evaluated)
    double axis[3] = {0, 0, 0};
    double ub = 0;
};

static NodeIn make_nodedev(const HNode &h, const Bounds &b) {
    NodeIn d;
    std::memset(&d, 0, sizeof d);
    d.begin = h.begin; d.n = h.n; d.gn = h.gn; d.buf = h.buf; d.slot = -1; d.child0 = -1; d.nchild = 0; d.split = -1;
    for (int j = 0; j < 3; j++) d.mean[j] = h.mean[j];
    d.sw = h.sw;
    int P = 1;
    while ((1ULL << P) < (h.gn > 1 ? h.gn : 2)) P++;
    d.klin = make_bink(b.e_lin, P);
    d.kquad = make_bink(b.e_quad, P);
    return d;
}

// Host staging buffers are pinned and one per purpose; every round ends with a stream sync (get_nodes), so a
// buffer is never rewritten while an earlier async copy from it is still in flight.
static void put_nodes(Engine &E, const std::vector<int> &ids, const std::vector<NodeIn> &recs) {
    const int n = (int)ids.size();
    if (!n) return;
    if (n == 1) {
        hipLaunchKernelGGL(k_put_node1, 1, 1, 0, E.stream, E.nodes.p, ids[0], recs[0]);
        HIP_CHECK(hipGetLastError());
        return;
    }
    E.stage_in.reserve(n); E.ids.reserve(n); E.h_stage_in.reserve(n); E.h_ids.reserve(n);
    std::memcpy(E.h_stage_in.p, recs.data(), n * sizeof(NodeIn));
    std::memcpy(E.h_ids.p, ids.data(), n * sizeof(int));
    HIP_CHECK(hipMemcpyAsync(E.stage_in.p, E.h_stage_in.p, n * sizeof(NodeIn), hipMemcpyHostToDevice, E.stream));
    HIP_CHECK(hipMemcpyAsync(E.ids.p, E.h_ids.p, n * sizeof(int), hipMemcpyHostToDevice, E.stream));
    hipLaunchKernelGGL(k_put_nodes, (n + 63) / 64, 64, 0, E.stream, E.nodes.p, E.stage_in.p, E.ids.p, n);
    HIP_CHECK(hipGetLastError());
    // no sync: h_stage_in / h_ids belong to put_nodes alone and every put is followed by a stream sync (get_nodes or an
    // explicit one) before the next put rewrites them
}

static void get_nodes(Engine &E, const std::vector<int> &ids, std::vector<NodeOut> &recs) {
    const int n = (int)ids.size();
    recs.resize(n);
    if (!n) return;
    E.stage_out.reserve(n); E.ids.reserve(n); E.h_stage_out.reserve(n); E.h_ids_get.reserve(n);
    std::memcpy(E.h_ids_get.p, ids.data(), n * sizeof(int));
    HIP_CHECK(hipMemcpyAsync(E.ids.p, E.h_ids_get.p, n * sizeof(int), hipMemcpyHostToDevice, E.stream));
    hipLaunchKernelGGL(k_get_nodes, (n + 63) / 64, 64, 0, E.stream, E.nodes.p, E.stage_out.p, E.ids.p, n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(E.h_stage_out.p, E.stage_out.p, n * sizeof(NodeOut), hipMemcpyDeviceToHost, E.stream));
    E.sync();
    std::memcpy(recs.data(), E.h_stage_out.p, n * sizeof(NodeOut));
}

// as get_nodes, the ids already on the device (part of the round packet)
static void get_nodes_dev(Engine &E, const int *d_ids, int n, std::vector<NodeOut> &recs) {
    recs.resize(n);
    if (!n) return;
    E.h_stage_out.reserve(n);
    // the kernel stores the records straight into pinned host memory (device-visible): no copy engine round trip
    hipLaunchKernelGGL(k_get_nodes, (n + 63) / 64, 64, 0, E.stream, E.nodes.p, E.h_stage_out.p, d_ids, n);
    HIP_CHECK(hipGetLastError());
    E.sync();
    std::memcpy(recs.data(), E.h_stage_out.p, n * sizeof(NodeOut));
}

static void absorb_moments(HNode &h, const NodeOut &d) {
    for (int q = 0; q < 6; q++) h.cov6[q] = d.acc[q][0] + d.acc[q][1];
    h.dist = d.acc[6][0] + d.acc[6][1];
}

// principal axis from the node's covariance sums (pca.c:62-101 divides by sum(w), then dsyev)
static bool node_axis(const HNode &h, double axis[3]) {
    if (h.axis_state != 0) {
        for (int j = 0; j < 3; j++) axis[j] = h.axis[j];
        return h.axis_state > 0;
    }
    double c6[6];
    for (int q = 0; q < 6; q++) c6[q] = h.cov6[q] / h.sw;
    return hm::principal_axis(c6, axis);
}

// Solve the node's 3x3 once, when its moments arrive: the axis its split evaluation will use, and an upper bound of the
// benefit of splitting it.  The benefit (local.c:256-274: distortion minus the children's) is the between-group scatter
// sum_g sw_g |mu_g - mu|^2 of the two children; the mean difference has ONE direction u, and the scatter between groups
// along u cannot exceed the node's total scatter along u, u' S u <= lambda_max(S) = sw * lambda_max(cov).  That holds for
// any two-way partition, so it bounds the benefit of the cut the reference will choose -- about three times tighter than
// the distortion (the trace of S) for a roundish cluster.  The margins cover the roundings of the computed sums (~1e-15
// relative to the distortion) with six orders to spare.
static void leaf_bound(HNode &h) {
    h.ub = h.dist;
    h.axis_state = 0;
    if (h.gn <= 1 || !(h.sw > 0)) { h.ub = 0; return; }          // never split (local.c:262-264)
    double c6[6];
    for (int q = 0; q < 6; q++) c6[q] = h.cov6[q] / h.sw;
    double a[9] = {c6[0], c6[1], c6[2], c6[1], c6[3], c6[4], c6[2], c6[4], c6[5]};
    double w[3];
    if (hm::eigen_sym3(a, w) != 0) { h.axis_state = -1; return; }
    h.axis[0] = a[6]; h.axis[1] = a[7]; h.axis[2] = a[8]; h.axis_state = 1;
    const double b = w[2] * h.sw * (1.0 + 1e-9) + 1e-9 * h.dist;
    if (b == b && b < h.ub) h.ub = b;                              // NaN / larger: keep the distortion
}

// The element counts of the quantisers' tables, from three inputs: the pixels on this GPU, the plane count and the nodes a round may
// hold -- 1 for the root, nr for a round of the host-driven split loop, kLqRoundCap for the device-driven one.  A round of several
// nodes has up to one partial tile per node on top of the image's own.
struct QuantSizes {
    size_t bufA, bufB, bkt, tilesA, tilesP, tilecnt, tileoff, hist, hsize, hcount, lut;
    QuantSizes(size_t pixels, size_t planes, size_t nodes) {
        const size_t slack = nodes > 1 ? nodes : 0;
        bufA = bufB = planes * pixels + 64;                      // + the slack k_scatter_bin's pixel-less lanes store to
        bkt = pixels;
        tilesA = ceil_div(pixels, (size_t)kTileA) + slack; tilesP = ceil_div(pixels, (size_t)kTileP) + slack;
        tilecnt = tileoff = tilesP * kMaxChildren;
        hist = std::max(hist_slot_doubles(), (size_t)kNQ_LQ * 2 * kBuckets * nodes);
        hsize = hcount = lut = nodes * kBuckets;
    }
};
// DevBuf::reserve frees the old allocation: call this only where the stream holds no queued work, or where an earlier call has
// reserved as much already (a no-op then)
static void reserve_quant_tables(Engine &E, const QuantSizes &z, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    E.bufA.reserve(z.bufA, file, line); E.bufB.reserve(z.bufB, file, line); E.bkt.reserve(z.bkt, file, line);
    E.tilesA.reserve(z.tilesA, file, line); E.tilesP.reserve(z.tilesP, file, line);
    E.tilecnt.reserve(z.tilecnt, file, line); E.tileoff.reserve(z.tileoff, file, line);
    E.hist.reserve(z.hist, file, line); E.hsize.reserve(z.hsize, file, line); E.hcount.reserve(z.hcount, file, line); E.lut.reserve(z.lut, file, line);
}

// --------------------------------------------------------------------------------------------
// GQ + LQ + PALETTE_create on the converted image in E.cvt (planar, stride N, optional w plane)
// returns centres planar (len,3)
// --------------------------------------------------------------------------------------------
// Everything the global quantiser needs that depends on the image SIZE only: workspace, the root's two tilings, cleared bucket
// tables.  run_device() enqueues it right behind the conversion kernel, so these small copies and fills run while the host waits
// for the conversion's bounds instead of between the quantiser's kernels.
static void gq_prepare(Engine &E, size_t N, bool weighted) {
    hipStream_t s = E.stream;
    const size_t planes = weighted ? 4 : 3;
    const QuantSizes z(N, planes, 1);
    reserve_quant_tables(E, z);
    const int ntA = (int)z.tilesA, ntP = (int)z.tilesP;
    E.h_round.reserve(kBuckets);                                // (receives the bucket counts later: sized once, before any copy uses it)
    E.round_nodes.reserve(1); E.node_tile0.reserve(2);
    const size_t hs = hist_slot_doubles();
    hipLaunchKernelGGL(k_gq_prepare, 64, 256, 0, s, E.tilesA.p, ntA, E.tilesP.p, ntP, (unsigned long long)N, E.round_nodes.p, E.node_tile0.p,
                       E.hist.p, (unsigned long long)hs, E.hsize.p, E.hcount.p);
    HIP_CHECK(hipGetLastError());
    E.prep_N = N; E.prep_planes = planes;
}



// patolette_amd_set_split_loop: 2 (default) the device-driven loop for images below kLqDeviceAutoPixels, 1 wherever it applies,
// 0 the host-driven one everywhere.  Measured, round 6 (profiles/r06_split_loop_ab.txt), per call, device against host-driven:
// first version 1920x1080 1.61 / 1.77 ms, 4096^2 5.81 / 5.80, 8192^2 21.7 / 21.0 (every leaf that could reach tau was evaluated at
// once: ~500 evaluations where the host's lock-step pruning makes ~320); with the global quantiser on the device too and the
// host loop's own waiting rule in k_lq_select (same ~320 evaluations): 1.38 / 1.53, 5.28-5.46 / 5.66-5.87, 21.4-21.5 / 21.2-21.7.
std::atomic<int> g_lq_device{getenv("PAMD_LQ_DEVICE") ? atoi(getenv("PAMD_LQ_DEVICE")) : 2};
// patolette_amd_set_global_quantiser: 1 (default) the global quantiser's decisions on the device (k_gq_control), 0 the host's turn
std::atomic<int> g_gq_device{getenv("PAMD_GQ_DEVICE") ? atoi(getenv("PAMD_GQ_DEVICE")) : 1};
constexpr size_t kLqDeviceAutoPixels = (size_t)40 << 20;

static bool lq_device_eligible(const Engine &E, size_t N, size_t K, bool verbose, bool allow_device) {
    const int lq_mode = g_lq_device.load(std::memory_order_relaxed);
    return allow_device && (lq_mode == 1 || (lq_mode == 2 && N < kLqDeviceAutoPixels)) && !E.shard && !verbose && K <= (size_t)kLqDevMaxK;
}

// What the quantisers of a call on an image of N pixels will reserve -- gq_prepare's tables, the node table and, when the call may
// take the device-driven split loop, that loop's tables at their caps (lq_device_loop) -- reserved before the call enqueues
// anything.  DevBuf::reserve frees the old allocation: never while queued work may still use it (the host-driven loop grows its
// tables only after a synchronisation, see lq_host_round).  A no-op on every later call at this size.
static void ws_prepare(Engine &E, size_t N, size_t K, bool weighted, bool verbose) {
    const size_t planes = weighted ? 4 : 3;
    const bool lq_dev = lq_device_eligible(E, N, K, verbose, true);
    E.cvt.reserve(planes * N); E.cstats.reserve(1);
    reserve_quant_tables(E, QuantSizes(N, planes, lq_dev ? (size_t)kLqRoundCap : 1));
    E.round_nodes.reserve(1); E.node_tile0.reserve(2); E.h_round.reserve(kBuckets);
    E.nodes.reserve(std::max<size_t>(4 * K + 64, lq_dev ? (size_t)kLqNodeCap : 0));
    E.h_dbl.reserve(16 * kBuckets * 2 + 64);
    E.gq.reserve(1); E.gqout.reserve(1); E.h_gqout.reserve(1); E.h_gq.reserve(1);
    const size_t nput = kGqMaxK + 1;                               // put_nodes / get_nodes of the global quantiser: the root and its base clusters
    E.stage_in.reserve(nput); E.stage_out.reserve(nput); E.ids.reserve(nput); E.h_stage_in.reserve(nput); E.h_stage_out.reserve(nput);
    E.h_ids.reserve(nput); E.h_ids_get.reserve(nput);
    E.h_cent.reserve(3 * K);                                       // KMeans: the centroids' pinned copy
    // the map stage's palette (at most K rows) on the device and pinned: an engine that met a smaller K first would otherwise grow
    // them in the map stage, where the second stream may still hold work of this call
    E.dpal.reserve(3 * K); E.h_pal.reserve(3 * K);
    if (lq_dev) { E.lqctl.reserve(1); E.h_lqhead.reserve(1); E.h_lqrec.reserve(kLqNodeCap); E.h_lqcen.reserve(kLqNodeCap); }
}

// The local quantiser driven from the device (k_lq_children / k_lq_select above).  In: the base clusters are nodes first_base ..
// first_base + kbase - 1 of the table with their segments, means and moment accumulators complete on the stream (no synchronisation
// yet).  Returns 0 (centres, stats filled in; the trace on request), -2 if the candidate tree outgrew the device's table (the caller
// starts over on the host loop).
static int lq_device_loop(Engine &E, size_t N, size_t K, bool weighted, bool inv_sums, const Bounds &bnd, const QuantBuffers &qlq, int kbase,
                          int first_base, int nnodes, std::vector<double> &centers, size_t &len, unsigned long long *max_members) {
    hipStream_t s = E.stream;
    const size_t lqs = (size_t)kNQ_LQ * 2 * kBuckets;
    const QuantSizes z(N, weighted ? 4 : 3, kLqRoundCap);          // (ws_prepare reserved as much: the stream holds queued work here)
    const int ntA_ub = (int)z.tilesA, ntP_ub = (int)z.tilesP;      // the image's tiles + one partial tile per node of a round
    E.lqctl.reserve(1); E.h_lqhead.reserve(1); E.h_lqrec.reserve(kLqNodeCap); E.h_lqcen.reserve(kLqNodeCap);
    reserve_quant_tables(E, z);
    LqCtl *c = E.lqctl.p;
    LqHead *head = E.h_lqhead.p;
    for (int r = 0; r < kLqMaxRounds; r++) { head->round_px[r] = 0.0; head->round_nr[r] = 0.0; }
    const RoundDyn *dyn = &c->dyn;
    const int *d_round = c->round_ids, *d_tP0 = c->tP0;
    int call = 0;                                                  // control calls so far: the parity selects the children list (LqCtl::cids)
    // kbase < 0: the global quantiser ran on the device too (k_gq_control): the count of base clusters is in E.gqout, twelve at most
    const GqOut *gq = kbase < 0 ? (const GqOut *)E.gqout.p : nullptr;
    const int kb_ub = kbase < 0 ? kGqMaxK : kbase;
    auto control = [&]() {
        const bool first = call == 0;
        {
            KTIME("k_lq_children", s, 0.0);
            if (first) hipLaunchKernelGGL(k_lq_children, (kb_ub + 3) / 4, 256, 0, s, E.nodes.p, c, call, kb_ub, first_base, nnodes, (int)K, gq);
            else hipLaunchKernelGGL(k_lq_children, 2 * kLqRoundCap / 4, 256, 0, s, E.nodes.p, c, call, 0, 0, 0, 0, (const GqOut *)nullptr);
        }
        KTIME("k_lq_select", s, 0.0);
        hipLaunchKernelGGL(k_lq_select, 1 + (first ? (kb_ub + 3) / 4 : 2 * kLqRoundCap / 4), 256, 0, s, E.nodes.p, c, call, bnd.e_lin, bnd.e_quad);
        HIP_CHECK(hipGetLastError());
        call++;
    };
    int enq = 0;                                                   // rounds enqueued so far
    auto round = [&]() {
        if (enq >= kLqMaxRounds) throw HipError("patolette_amd: split loop exceeded its round limit");
        const double *px_src = &head->round_px[enq], *nr_src = &head->round_nr[enq];
        const bool rev = enq % 2 == 1;                             // the sweeps alternate their direction (see the host loop)
        // the round's set-up (tile lists, cleared bucket tables) rides on its first sweep; PAMD_LQ_SETUP_KERNEL=1: a launch of its own (A/B)
        static const bool setup_kernel = getenv("PAMD_LQ_SETUP_KERNEL") && atoi(getenv("PAMD_LQ_SETUP_KERNEL")) != 0;
        if (setup_kernel) {
            hipLaunchKernelGGL(k_round_setup_dyn, 1024, 256, 0, s, E.nodes.p, (const LqCtl *)c, E.tilesA.p, E.tilesP.p, E.hist.p, E.hsize.p, E.hcount.p, lqs);
            HIP_CHECK(hipGetLastError());
            launch_minmax(qlq, E.tilesA.p, ntA_ub, 0, E.nodes.p, s, rev, dyn, px_src);
        } else {
            const RoundLists rl{c->round_ids, c->tA0, c->tP0, E.tilesA.p, E.tilesP.p, E.hist.p, lqs, E.hsize.p, E.hcount.p};
            launch_minmax(qlq, E.tilesA.p, ntA_ub, 0, E.nodes.p, s, rev, dyn, px_src, &rl);
        }
        launch_hist(qlq, false, E.tilesA.p, ntA_ub, 0, E.nodes.p, E.hist.p, E.hsize.p, E.hcount.p, s, !rev, false, dyn, px_src);
        launch_cut(weighted, E.nodes.p, d_round, kLqRoundCap, E.hist.p, E.hsize.p, E.hcount.p, E.lut.p, s, dyn, nr_src);
        launch_partition(qlq, E.tilesP.p, ntP_ub, 0, d_round, d_tP0, kLqRoundCap, E.nodes.p, E.lut.p, E.tilecnt.p, E.tileoff.p, true, s, inv_sums, rev, dyn, px_src);
        enq++;
        control();
    };
    control();                                                     // the base clusters' moments and bounds, round 1
    int want = (E.lq_hint_N == N && E.lq_hint_K == K && E.lq_hint_rounds > 0) ? E.lq_hint_rounds : 9;
    const bool fault_full = g_debug_fault.load(std::memory_order_relaxed) == 4;
    if (fault_full) want = 3;
    for (;;) {
        while (enq < want) round();
        hipLaunchKernelGGL(k_lq_export, 16, 256, 0, s, (const LqCtl *)c, head, E.h_lqrec.p, E.h_lqcen.p);
        HIP_CHECK(hipGetLastError());
        E.sync();
        if (fault_full) return -2;                                 // patolette_amd_debug_fault(4): the table "filled up" after three rounds
        if (head->done) break;
        want = enq + 2;
    }
    if (head->error == 2) return -2;
    if (head->error == 3) return -1;                               // the global quantiser's eigen-solve failed (global.c:214-217)
    if (kbase < 0) kbase = E.h_gqout.p->kbase;
    E.lq_hint_N = N; E.lq_hint_K = K; E.lq_hint_rounds = head->rounds;
    LqReplay rp;
    const double t_rp0 = now_ms();
    // the records as the device left them in pinned memory are cache misses one by one (the replay hops from node to node: 36 us for
    // 254 steps); one sequential copy brings them in (18-28 us)
    E.lq_rec_local.resize((size_t)head->nnodes);
    std::memcpy(E.lq_rec_local.data(), E.h_lqrec.p, (size_t)head->nnodes * sizeof(LqRec));
    const int fault = g_debug_fault.load(std::memory_order_relaxed);
    const bool replay_ok = lq_replay(E.lq_rec_local.data(), kbase, first_base, K, kDelta, fault, rp);
    const double t_rp1 = now_ms();
    static const bool replay_check = getenv("PAMD_LQ_REPLAY_CHECK") != nullptr;
    if (replay_check || !replay_ok) {
        LqReplay ref;
        const bool ref_ok = lq_replay_plain(E.lq_rec_local.data(), kbase, first_base, K, kDelta, fault, ref);
        if (ref_ok != replay_ok || ref.result != rp.result || ref.stopped_early != rp.stopped_early)
            fprintf(stderr, "patolette_amd: split loop: the two replays DISAGREE (plain %d, %zu rows; blocked %d, %zu rows), kbase %d, K %zu, nodes %d, rounds %d\n",
                    (int)ref_ok, ref.result.size(), (int)replay_ok, rp.result.size(), kbase, K, head->nnodes, head->rounds);
        else if (!replay_ok)
            fprintf(stderr, "patolette_amd: split loop: both replays blocked after %zu commits, kbase %d, K %zu, nodes %d, rounds %d, evaluated %d, tau %.17g\n",
                    rp.commits.size(), kbase, K, head->nnodes, head->rounds, head->neval, head->tau);
    }
    if (!replay_ok) throw HipError("patolette_amd: split loop: the replay met an unevaluated node");
    len = rp.result.size();
    centers.assign(3 * len, 0.0);
    unsigned long long mg = 0;
    for (size_t i = 0; i < len; i++) {
        const LqCen &cn = E.h_lqcen.p[rp.result[i]];
        for (int j = 0; j < 3; j++) centers[(size_t)j * len + i] = cn.mean[j];      // create.c:11-33
        mg = std::max(mg, (unsigned long long)cn.gn);
    }
    if (max_members) *max_members = mg;
    E.stats.split_evals = (size_t)head->split_evals; E.stats.split_px = (size_t)head->split_px; E.stats.lq_rounds = (size_t)head->rounds;
    E.lq_commits.swap(rp.commits);
    E.trace.clear();
    E.trace_pending = true;
    E.trace_hdr.stopped_early = rp.stopped_early ? 1 : 0;
    static const bool lq_times = getenv("PAMD_LQ_TIMES") != nullptr;
    if (lq_times) {
        fprintf(stderr, "patolette_amd: device-driven split loop: %d rounds, %d evaluated, %zu commits, tau %.3g; host replay %.1f us\n", head->rounds, head->neval,
                E.lq_commits.size(), head->tau, 1e3 * (t_rp1 - t_rp0));
        if (gq) {
            const unsigned long long *t = E.h_gqout.p->ticks;
            fprintf(stderr, "patolette_amd: k_gq_control us: prefixes %.1f, axis %.1f, search %.1f, records %.1f\n", (t[1] - t[0]) * 0.01, (t[2] - t[1]) * 0.01,
                    (t[3] - t[2]) * 0.01, (t[4] - t[3]) * 0.01);
            fprintf(stderr, "patolette_amd: k_gq_control us: of the prefixes, staging %.1f\n", (t[5] - t[0]) * 0.01);
        }
    }
    return 0;
}

// the split trace of a device-driven call, fetched when asked for (the node table stays on the device until the engine's next call)
static void materialise_trace(Engine &E) {
    if (!E.trace_pending) return;
    E.trace_pending = false;
    const int n = (int)E.lq_commits.size();
    E.trace.assign(n, patolette_amd__SplitRecord{});
    if (!n) return;
    DevBuf<LqCommit> dc; DevBuf<patolette_amd__SplitRecord> dr;
    dc.reserve(n); dr.reserve(n);
    HIP_CHECK(hipMemcpyAsync(dc.p, E.lq_commits.data(), sizeof(LqCommit) * n, hipMemcpyHostToDevice, E.stream));
    hipLaunchKernelGGL(k_lq_trace, (n + 63) / 64, 64, 0, E.stream, (const NodeDev *)E.nodes.p, (const LqCommit *)dc.p, n, dr.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(E.trace.data(), dr.p, sizeof(patolette_amd__SplitRecord) * n, hipMemcpyDeviceToHost, E.stream));
    HIP_CHECK(hipStreamSynchronize(E.stream));
}

// One quantize_clusters_run call: what its stages (below, in their order) share
struct QuantCall {
    Engine &E;
    const size_t N, Nt, K;                                      // pixels on this GPU (a sliced image: this GPU's part), of the whole image; palette size
    const bool weighted, inv_sums, verbose, dev_eligible;
    const Shard *sh;                                            // the image is dealt out over a group of GPUs
    const Bounds &bnd;
    std::vector<double> &centers; size_t &len; unsigned long long *max_members;
    const QuantBuffers qroot, qlq;
    const int ntA0, ntP0;                                       // the root's tilings (gq_prepare)
    const size_t hs;                                            // doubles of the global quantiser's histogram
    double t0;                                                  // start of the running stage (stats.ms_gq, ms_lq)
    std::vector<HNode> hn;                                      // id 0: the root
    bool mom_path = false;                                      // the root's covariance came with the conversion pass: one sweep less
    double axis[3] = {0, 0, 0};                                 // the root's principal axis
    int kbase = 0;
    std::vector<int> base_ids;
    std::vector<NodeOut> got;
};

// ---------------- global quantiser (global.c:388-443) ----------------
// unweighted PCA of all pixels: mean, centred covariance, dsyev
static void gq_root_mean(QuantCall &C) {
    Engine &E = C.E;
    const size_t Nt = C.Nt;
    const Bounds &bnd = C.bnd;
    HNode root; root.begin = 0; root.n = C.N; root.gn = Nt; root.buf = 0; root.sw = (double)Nt;
    E.h_dbl.reserve(16 * kBuckets * 2 + 64);
    if (bnd.have_sum) {
        const double inv = 1 / (double)Nt;                      // matrix2D.c:229; the sums came with the conversion pass
        for (int j = 0; j < 3; j++) root.mean[j] = bnd.sum[j] * inv;
    } else {
        int rootP = 1; while ((1ULL << rootP) < (Nt > 1 ? Nt : 2)) rootP++;
        E.sum6.reserve(kSum3Slots * 6);
        launch_sum3(E.cvt.p, C.N, make_bink(bnd.e_lin, rootP), E.sum6.p, E.stream);
        if (C.sh) comm_sum_dev(E, E.sum6.p, kSum3Slots * 6, 0);
        HIP_CHECK(hipMemcpyAsync(E.h_dbl.p, E.sum6.p, kSum3Slots * 6 * sizeof(double), hipMemcpyDeviceToHost, E.stream));
        E.sync();
        const double inv = 1 / (double)Nt;                      // matrix2D.c:229
        for (int j = 0; j < 3; j++) {
            double p0 = 0, p1 = 0;                              // slot partials are exact multiples of the bin grids
            for (int sl = 0; sl < kSum3Slots; sl++) { p0 += E.h_dbl.p[sl * 6 + 2 * j]; p1 += E.h_dbl.p[sl * 6 + 2 * j + 1]; }
            root.mean[j] = (p0 + p1) * inv;
        }
    }
    C.hn.push_back(root);                                       // id 0
}

// every sweep over the pixels starts where the previous one stopped (see the split rounds below): the conversion wrote the
// image front to back, so the root's moments are taken back to front, the extrema front to back, ...
static void gq_root_covariance(QuantCall &C) {
    Engine &E = C.E;
    const Bounds &bnd = C.bnd;
    std::vector<HNode> &hn = C.hn;
    C.mom_path = bnd.have_mom && !C.sh;                         // one sweep less: the directions of the following ones flip
    if (C.mom_path) {
        // The conversion pass took the column sums S1 and the raw second moments S2 as exact pairs: the centred sums
        // S2_jk - S1_j S1_k / n (pca.c:62-101 about the mean, matrix2D.c:200-233) follow in extended precision, then ONE rounding
        // to double -- instead of a sweep over the image and a round trip.  What the shortcut cannot undo: every product x_j x_k was
        // rounded to double before it was binned (relative 2^-53, systematic for a flat image), so the difference is good to
        // ~1e-16 of S2 and no better: an image whose spread is tiny against its mean -- trace(cov) below 1e-6 of trace(S2), i.e.
        // fewer than ~10 digits left --, or a difference that came out negative, takes the centred sweep below instead.
        const long double nn = (long double)C.Nt;
        long double s1[3], c6[6], s2d[3] = {0, 0, 0};
        for (int j = 0; j < 3; j++) s1[j] = (long double)bnd.sum2[j][0] + (long double)bnd.sum2[j][1];
        static const int ja[6] = {0, 1, 2, 1, 2, 2}, jb[6] = {0, 0, 0, 1, 1, 2};       // xx, yx, zx, yy, zy, zz
        for (int q = 0; q < 6; q++) {
            const long double s2 = (long double)bnd.mom2[q][0] + (long double)bnd.mom2[q][1];
            if (ja[q] == jb[q]) s2d[ja[q]] = s2;
            c6[q] = s2 - s1[ja[q]] * s1[jb[q]] / nn;
        }
        const long double tr = c6[0] + c6[3] + c6[5], tr2 = s2d[0] + s2d[1] + s2d[2];
        if (!(tr > 1e-6L * tr2) || c6[0] < 0 || c6[3] < 0 || c6[5] < 0) C.mom_path = false;
        else {
            for (int q = 0; q < 6; q++) hn[0].cov6[q] = (double)c6[q];
            hn[0].dist = (double)tr;
        }
    }
    if (!C.mom_path) {
        NodeIn d = make_nodedev(hn[0], bnd);
        put_nodes(E, {0}, {d});
        launch_cov_nodes(C.qroot, E.cvt.p, E.tilesA.p, C.ntA0, C.N, E.nodes.p, E.stream, true);
        if (C.sh) shard_exchange_acc(E, shard_upload_ids(E, {0}), 1);
        get_nodes(E, {0}, C.got);
        absorb_moments(hn[0], C.got[0]);
    }
}

// the root's axis, the head of the split trace, then projection, 512 buckets, cell moments (sort.c, cells.c:53-139).
// false: the eigen-solve failed
static bool gq_root_histogram(QuantCall &C) {
    Engine &E = C.E;
    hipStream_t s = E.stream;
    const HNode &root = C.hn[0];
    if (!node_axis(root, C.axis)) return false;
    E.trace.clear();
    E.trace_pending = false;
    E.trace_hdr = patolette_amd__SplitTrace{};
    for (int j = 0; j < 3; j++) E.trace_hdr.gq_axis[j] = C.axis[j];
    for (int q = 0; q < 6; q++) E.trace_hdr.gq_cov6[q] = root.cov6[q] / root.sw;
    {
        NodeIn d = make_nodedev(root, C.bnd);
        for (int j = 0; j < 3; j++) d.axis[j] = C.axis[j];
        d.slot = 0;
        put_nodes(E, {0}, {d});
    }
    launch_minmax(C.qroot, E.tilesA.p, C.ntA0, C.N, E.nodes.p, s, C.mom_path);
    if (C.sh) shard_exchange_keys(E, shard_upload_ids(E, {0}), 1);
    launch_hist(C.qroot, true, E.tilesA.p, C.ntA0, C.N, E.nodes.p, E.hist.p, E.hsize.p, E.hcount.p, s, !C.mom_path, C.Nt >= ((size_t)1 << 18));
    if (C.sh) { comm_sum_dev(E, E.hist.p, C.hs, 0); comm_sum_dev(E, E.hcount.p, kBuckets, 2); }
    return true;
}

// what k_gq_control decided, into the head of the split trace (after a synchronisation)
static void gq_trace_header(Engine &E) {
    const GqOut &o = *E.h_gqout.p;
    E.trace_hdr.n_base = o.kbase;
    for (int j = 0; j <= o.kbase && j < 14; j++) E.trace_hdr.gq_cuts[j] = (size_t)o.cuts[j];
}

// The hand-over to the device-driven split loop, behind either turn of the global quantiser: no synchronisation here, the control
// kernel takes the base clusters' moments itself.  kbase < 0: the count of base clusters is the device's too (k_gq_control).
static int finish_device_loop(QuantCall &C, int kbase, int first_base, int nnodes) {
    Engine &E = C.E;
    if (kbase >= 0) E.stats.n_base_clusters = (size_t)kbase;
    E.stats.ms_gq = now_ms() - C.t0;
    C.t0 = now_ms();
    const int rc = lq_device_loop(E, C.N, C.K, C.weighted, C.inv_sums, C.bnd, C.qlq, kbase, first_base, nnodes, C.centers, C.len, C.max_members);
    if (kbase < 0) {
        gq_trace_header(E);
        E.stats.n_base_clusters = (size_t)E.h_gqout.p->kbase;
    }
    if (rc != 0) return rc;
    E.stats.n_clusters = C.len;
    E.trace_hdr.n_clusters = (int32_t)C.len; E.trace_hdr.n_records = (int32_t)E.lq_commits.size();
    E.cluster_centers = C.centers;
    E.stats.ms_lq = now_ms() - C.t0;
    return 0;
}

// what the turns of the global quantiser answer besides a return code of the call: go on with the host-driven split loop
constexpr int kHostLoop = 1;

// The quantiser's decisions (global.c:189-298) on the device, the partition behind them without the host looking (k_gq_control):
// one GPU, palettes of more than twelve colours (so that base clusters < K whatever the image), not verbose.  PAMD_GQ_DEVICE=0:
// the host's turn everywhere (A/B; what sliced images, small palettes and verbose calls always take)
static int gq_device_turn(QuantCall &C) {
    Engine &E = C.E;
    hipStream_t s = E.stream;
    E.gq.reserve(1); E.gqout.reserve(1); E.h_gqout.reserve(1);
    *E.h_gqout.p = GqOut{};
    {
        KTIME("k_gq_control", s, (double)C.hs * 8);
        hipLaunchKernelGGL(k_gq_control, 1, 1024, 0, s, (const double *)E.hist.p, (const unsigned int *)E.hcount.p, E.gq.p, (int)std::min<size_t>(C.K, (size_t)1 << 30),
                           C.weighted ? 1 : 0, E.nodes.p, 1, E.lut.p, E.gqout.p, E.h_gqout.p, (GqPrefixes *)nullptr);
        HIP_CHECK(hipGetLastError());
    }
    launch_partition(C.qroot, E.tilesP.p, C.ntP0, C.N, E.round_nodes.p, E.node_tile0.p, 1, E.nodes.p, E.lut.p, E.tilecnt.p, E.tileoff.p, true, s, C.inv_sums,
                     C.mom_path, nullptr, nullptr, true);
    launch_cov_children(C.qroot, E.tilesA.p, C.ntA0, C.N, E.nodes.p, s, !C.mom_path, true);
    if (C.dev_eligible) return finish_device_loop(C, -1, 1, 0);
    // the host-driven split loop: the count comes down with the base clusters' records (the first kbase of twelve)
    std::vector<int> all(kGqMaxK);
    for (int j = 0; j < kGqMaxK; j++) all[j] = 1 + j;
    get_nodes(E, all, C.got);
    if (E.h_gqout.p->error) return -1;
    gq_trace_header(E);
    C.kbase = E.h_gqout.p->kbase;
    for (int j = 0; j < C.kbase; j++) {
        const NodeOut &g = C.got[j];
        HNode c; c.buf = 1; c.begin = g.begin; c.n = g.n; c.gn = g.gn; c.sw = g.sw;
        for (int q = 0; q < 3; q++) c.mean[q] = g.mean[q];
        absorb_moments(c, g);
        leaf_bound(c);
        C.base_ids.push_back((int)C.hn.size());
        C.hn.push_back(c);
    }
    return kHostLoop;
}

// What the host's turn decides from the downloaded table (`hh`: quantity q, part p, bucket b at (q * 2 + p) * 512 + b; `hc`: the
// buckets' counts) and the device's cut table: the cuts, the bucket -> base cluster table and the base clusters' records.
// gq_host_turn and the table-level test entry (patolette_amd_debug_gq_table) both come here.
struct GqDecision {
    std::vector<size_t> cuts;
    int kbase = 0;
    std::vector<unsigned char> lut;
    struct Base { unsigned long long begin, n; double sw, mean[3]; } base[kGqMaxK];
};
static bool gq_host_decide(const double *hh, const unsigned int *hc, const bool weighted, const size_t K, const int (*cut)[kBuckets + 1], GqDecision &D,
                           hm::CellMoments *prefixes = nullptr) {
    auto H = [&](int q, int b) { return hh[(size_t)(q * 2 + 0) * kBuckets + b] + hh[(size_t)(q * 2 + 1) * kBuckets + b]; };

    auto cm = std::make_unique<hm::CellMoments>();
    std::memset(cm.get(), 0, sizeof(hm::CellMoments));
    for (int b = 0; b < kBuckets; b++) {
        cm->w0[b + 1] = hc[b];
        for (int r = 0; r < 3; r++) cm->w1[r][b + 1] = H(r, b);
        cm->w2[b + 1] = H(3, b);
        for (int q = 0; q < 6; q++) cm->wrs[q][b + 1] = H(4 + q, b);
    }
    for (int i = 1; i <= kBuckets; i++) {                       // cells.c:114-136 sequential prefix
        cm->w0[i] += cm->w0[i - 1]; cm->w2[i] += cm->w2[i - 1];
        for (int r = 0; r < 3; r++) cm->w1[r][i] += cm->w1[r][i - 1];
        for (int q = 0; q < 6; q++) cm->wrs[q][i] += cm->wrs[q][i - 1];
    }
    if (prefixes) *prefixes = *cm;
    D.cuts = hm::gq_principal_quantizer(K, *cm, cut);
    const std::vector<size_t> &cuts = D.cuts;
    if (cuts.size() < 2) return false;
    const int kbase = D.kbase = (int)cuts.size() - 1;

    // base clusters: bucket b belongs to the first cell j with b+1 <= q[j+1] (global.c:328-335)
    std::vector<unsigned char> &lut = D.lut;
    lut.assign(kBuckets, 0);
    for (int b = 0; b < kBuckets; b++) {
        int j = 0;
        while (j < kbase - 1 && !((size_t)(b + 1) <= cuts[j + 1])) j++;
        lut[b] = (unsigned char)j;
    }
    unsigned long long pos = 0;
    for (int j = 0; j < kbase; j++) {
        GqDecision::Base &c = D.base[j];
        c.begin = pos;
        unsigned long long cnt = 0;
        double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};          // exact: parts lie on the bin grids
        for (int b = 0; b < kBuckets; b++) if (lut[b] == j) {
            cnt += hc[b];
            for (int q = 0; q < (weighted ? 4 : 3); q++) {
                int qi = weighted ? 10 + q : q;
                s0[q] += hh[(size_t)(qi * 2 + 0) * kBuckets + b];
                s1[q] += hh[(size_t)(qi * 2 + 1) * kBuckets + b];
            }
        }
        c.n = cnt;
        c.sw = weighted ? (s0[3] + s1[3]) : (double)cnt;
        const double inv = 1 / c.sw;
        for (int q = 0; q < 3; q++) c.mean[q] = (s0[q] + s1[q]) * inv;
        pos += cnt;
    }
    return true;
}

// The host's turn of the global quantiser: the cell moments come down, hm::gq_principal_quantizer decides, the bucket table and the
// base clusters' records go up, the partition follows
static int gq_host_turn(QuantCall &C) {
    Engine &E = C.E;
    hipStream_t s = E.stream;
    const size_t K = C.K, hs = C.hs;
    const bool weighted = C.weighted;
    std::vector<HNode> &hn = C.hn;
    const int gq_kmax = (int)std::min<size_t>(K, kGqMaxK);
    E.gq.reserve(1); E.h_gq.reserve(1);
    launch_gq_dp(E.hist.p, E.hcount.p, gq_kmax, E.gq.p, s);
    HIP_CHECK(hipMemcpyAsync(E.h_gq.p->cut, E.gq.p->cut, sizeof(E.h_gq.p->cut), hipMemcpyDeviceToHost, s));
    std::vector<double> hh(hs);
    std::vector<unsigned int> hc(kBuckets);
    HIP_CHECK(hipMemcpyAsync(E.h_dbl.p, E.hist.p, hs * sizeof(double), hipMemcpyDeviceToHost, s));
    E.h_round.reserve(kBuckets);
    HIP_CHECK(hipMemcpyAsync(E.h_round.p, E.hcount.p, kBuckets * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    E.sync();
    std::memcpy(hh.data(), E.h_dbl.p, hs * sizeof(double));
    std::memcpy(hc.data(), E.h_round.p, kBuckets * sizeof(unsigned int));
    GqDecision D;
    if (!gq_host_decide(hh.data(), hc.data(), weighted, K, E.h_gq.p->cut, D)) return -1;
    const std::vector<size_t> &cuts = D.cuts;
    const std::vector<unsigned char> &lut = D.lut;
    const int kbase = C.kbase = D.kbase;
    E.trace_hdr.n_base = kbase;
    for (int j = 0; j <= kbase && j < 14; j++) E.trace_hdr.gq_cuts[j] = cuts[j];
    // Two base clusters (what noise and most photographs give): the partition is a binary split like the local quantiser's, so
    // it takes the same pipelined kernel and the children's centred moments ride along instead of costing a sweep of their own
    const bool gq_binary = kbase == 2;
    std::vector<int> &base_ids = C.base_ids;
    for (int j = 0; j < kbase; j++) {
        const GqDecision::Base &b = D.base[j];
        HNode c; c.buf = 1; c.begin = b.begin;
        c.n = b.n; c.gn = b.n;                                       // sliced image: the segment on this GPU follows from the partition
        c.sw = b.sw;
        for (int q = 0; q < 3; q++) c.mean[q] = b.mean[q];
        base_ids.push_back((int)hn.size());
        hn.push_back(c);
    }
    {
        NodeIn d = make_nodedev(hn[0], C.bnd);
        for (int j = 0; j < 3; j++) d.axis[j] = C.axis[j];
        d.slot = 0; d.child0 = base_ids[0]; d.nchild = kbase;
        if (gq_binary) d.split = (int)cuts[1] - 1;               // bucket b is in cluster 0 iff b + 1 <= cuts[1] (global.c:328-335)
        std::vector<int> ids = {0};
        std::vector<NodeIn> recs = {d};
        for (int id : base_ids) { ids.push_back(id); NodeIn c = make_nodedev(hn[id], C.bnd); c.klin = d.klin; c.kquad = d.kquad; recs.push_back(c); }
        put_nodes(E, ids, recs);
    }
    E.h_bytes.reserve(kBuckets);                                // pinned: no synchronisation before the partition
    std::memcpy(E.h_bytes.p, lut.data(), kBuckets);
    HIP_CHECK(hipMemcpyAsync(E.lut.p, E.h_bytes.p, kBuckets, hipMemcpyHostToDevice, s));
    launch_partition(C.qroot, E.tilesP.p, C.ntP0, C.N, E.round_nodes.p, E.node_tile0.p, 1, E.nodes.p, E.lut.p, E.tilecnt.p, E.tileoff.p, gq_binary, s, C.inv_sums,
                     C.mom_path);
    if (C.sh) { hipLaunchKernelGGL(k_shard_children_local, 1, 64, 0, s, E.nodes.p, E.round_nodes.p, 1); HIP_CHECK(hipGetLastError()); }
    if (!gq_binary) launch_cov_children(C.qroot, E.tilesA.p, C.ntA0, C.N, E.nodes.p, s, !C.mom_path);
    if (C.sh) shard_exchange_acc(E, shard_upload_ids(E, base_ids), (int)base_ids.size());
    if (C.dev_eligible && (size_t)kbase < K) return finish_device_loop(C, kbase, base_ids[0], (int)hn.size());
    get_nodes(E, base_ids, C.got);
    for (size_t i = 0; i < base_ids.size(); i++) {
        absorb_moments(hn[base_ids[i]], C.got[i]);
        if (C.sh) { hn[base_ids[i]].begin = C.got[i].begin; hn[base_ids[i]].n = C.got[i].n; }
        leaf_bound(hn[base_ids[i]]);
    }
    return kHostLoop;
}

// ---------------- local quantiser (local.c:318-404), driven from the host ----------------
static bool hn_known(const HNode &h) { return h.nosplit || h.gn <= 1 || h.split_done; }
// the frontier's view of the host's node mirror: the benefit if the node's split is known, else its bound
struct HnRec {
    const std::vector<HNode> &hn;
    FrontierRec operator()(int id) const {
        const HNode &h = hn[id];
        if (!hn_known(h)) return FrontierRec{h.ub, false, h.left};
        if (h.nosplit || h.gn <= 1) return FrontierRec{0, true, h.left};       // children == NULL -> 0 (local.c:262-264)
        return FrontierRec{h.dist - (hn[h.left].dist + hn[h.right].dist), true, h.left};
    }
};
// PAMD_LQ_TIMES, a diagnostic: where the host's turn between two rounds goes
struct LqLaps {
    static bool env() { static const bool v = getenv("PAMD_LQ_TIMES") != nullptr; return v; }
    const bool on = env();
    double greedy = 0, select = 0, axes = 0, packet = 0, enqueue = 0, wait = 0, children = 0, mark = now_ms();
    void lap(double &acc) { if (on) { const double t = now_ms(); acc += t - mark; mark = t; } }
};
struct LqHostLoop {
    SplitFrontier F;                                            // the frontier in the reference's order
    std::vector<int> leaves;                                    // candidate-tree nodes with moments but no split yet
    LqLaps laps;
};

// a child as its parent's round left it on the device: segment, centre, moments; then its axis and bound
static void absorb_child(HNode &c, const NodeOut &d) {
    c.begin = d.begin; c.n = d.n; c.gn = d.gn; c.buf = d.buf; c.sw = d.sw; c.psplit = d.psplit;
    for (int j = 0; j < 3; j++) c.mean[j] = d.mean[j];
    absorb_moments(c, d);
    leaf_bound(c);
}

// The leaves worth a round's evaluation have a bound of at least this.  Leaves whose distortion (an upper bound of their benefit)
// is far below the current best benefit are left for later; the exactness test of the greedy step catches them if they ever
// become relevant.
static double lq_round_threshold(const SplitFrontier &F, size_t K) {
    double thr = std::max(kDelta, kSpecBeta * F.reference_benefit());
    // exact pruning: with R commits left, a leaf whose distortion is below the R-th largest
    // KNOWN frontier benefit can never be chosen (its own and all its descendants' benefits are
    // bounded by that distortion, and R better candidates outlast the remaining commits)
    const size_t R = K - F.count;
    std::vector<double> kb;
    F.known_values(kb);
    if (kb.size() >= R && R > 0) {
        std::nth_element(kb.begin(), kb.begin() + (R - 1), kb.end(), std::greater<double>());
        thr = std::max(thr, kb[R - 1] * (1.0 - 1e-9));
    }
    return thr;
}

// The greedy step is blocked: evaluate, in ONE round, the split of every leaf of the candidate tree that could still
// matter -- undecided frontier nodes and, speculatively, the children of decided ones (a node's
// split depends only on its members, never on the greedy order).
static void lq_host_round(QuantCall &C, LqHostLoop &L) {
    Engine &E = C.E;
    hipStream_t s = E.stream;
    std::vector<HNode> &hn = C.hn;
    LqLaps &laps = L.laps;
    const HnRec rec{hn};
    const double thr = lq_round_threshold(L.F, C.K);
    laps.lap(laps.greedy);
    std::vector<int> round;
    {
        std::vector<int> keep;
        for (int id : L.leaves) {
            HNode &h = hn[id];
            if (hn_known(h)) continue;                          // n <= 1 / nosplit: never split
            if (h.ub >= thr) round.push_back(id); else keep.push_back(id);
        }
        L.leaves.swap(keep);
    }
    if (round.empty()) {                                        // every blocking node is a leaf with dist >= ref_b >= thr
        throw HipError("patolette_amd: split loop blocked without candidates");
    }
    laps.lap(laps.select);
    // axes on the host (dsyev semantics), children ids, device records
    HIP_CHECK(hipStreamSynchronize(s));
    E.nodes.grow(hn.size() + 2 * round.size() + 2, hn.size());
    std::vector<int> todo;
    std::vector<NodeIn> recs;
    for (int id : round) {
        double ax[3];
        if (!node_axis(hn[id], ax)) { hn[id].nosplit = true; continue; }
        NodeIn d = make_nodedev(hn[id], C.bnd);
        for (int j = 0; j < 3; j++) d.axis[j] = ax[j];
        d.slot = (int)todo.size();
        d.child0 = (int)hn.size(); d.nchild = 2;
        hn[id].left = (int)hn.size(); hn[id].right = (int)hn.size() + 1;        // a consecutive pair (the frontier's right = left + 1)
        hn.push_back(HNode()); hn.push_back(HNode());
        todo.push_back(id); recs.push_back(d);
    }
    L.F.reload(rec);                                            // a failed eigen-solve above makes a node known (no split)
    laps.lap(laps.axes);
    if (todo.empty()) return;
    const int nr = (int)todo.size();
    size_t rpx = 0;
    for (int id : todo) rpx += hn[id].n;
    static const bool lq_trace = getenv("PAMD_LQ_TRACE") != nullptr;       // one line per split round on stderr
    if (lq_trace) fprintf(stderr, "patolette_amd: split round %zu: %d nodes, %zu pixels (%.2f of the image), %zu of %zu colours committed\n",
                          E.stats.lq_rounds + 1, nr, rpx, (double)rpx / (double)(C.N ? C.N : 1), L.F.count, C.K);
    // one packet, one copy: node records, ids, children ids, the tile prefixes of both tilings.  (Measured and removed:
    // the round issued chunk-major, groups of nodes of a few MB each taken through minmax -> hist -> cut -> count -> scan ->
    // scatter before the next group starts, so that the second and third read of a node may find it in the Infinity Cache;
    // profiles/r06_lq_chunk_major.txt.)
    std::vector<int> cids;
    for (int id : todo) { cids.push_back(hn[id].left); cids.push_back(hn[id].right); }
    std::vector<int> tAg = {0}, tPg = {0};                       // the nodes' tile prefixes (nr + 1 entries each)
    for (int id : todo) {
        const unsigned long long n = hn[id].n;
        tAg.push_back(tAg.back() + (int)((n + kTileA - 1) / kTileA)); tPg.push_back(tPg.back() + (int)((n + kTileP - 1) / kTileP));
    }
    const int ntA = tAg[nr], ntP = tPg[nr];
    const size_t o_recs = 0, o_ids = o_recs + (size_t)nr * sizeof(NodeIn), o_cids = o_ids + (size_t)nr * sizeof(int),
                 o_tA = o_cids + cids.size() * sizeof(int), o_tP = o_tA + tAg.size() * sizeof(int),
                 pk_bytes = o_tP + tPg.size() * sizeof(int);
    E.h_packet.reserve(pk_bytes); E.packet.reserve(pk_bytes);
    // the round's tables and the children's pinned records: grown here, while the stream is idle (the last round ended with
    // get_nodes_dev's synchronisation), not behind the packet's copy
    const size_t lqs = (size_t)kNQ_LQ * 2 * kBuckets;
    reserve_quant_tables(E, QuantSizes(C.N, C.weighted ? 4 : 3, (size_t)nr));
    E.h_stage_out.reserve(cids.size());
    std::memcpy(E.h_packet.p + o_recs, recs.data(), (size_t)nr * sizeof(NodeIn));
    std::memcpy(E.h_packet.p + o_ids, todo.data(), (size_t)nr * sizeof(int));
    std::memcpy(E.h_packet.p + o_cids, cids.data(), cids.size() * sizeof(int));
    std::memcpy(E.h_packet.p + o_tA, tAg.data(), tAg.size() * sizeof(int));
    std::memcpy(E.h_packet.p + o_tP, tPg.data(), tPg.size() * sizeof(int));
    laps.lap(laps.packet);
    HIP_CHECK(hipMemcpyAsync(E.packet.p, E.h_packet.p, pk_bytes, hipMemcpyHostToDevice, s));
    // the sweeps of a round alternate their direction through the pixels (the first one runs against the partition that
    // wrote them): each starts on what the previous one touched last
    const bool rev = E.stats.lq_rounds % 2 == 1;                // (the base clusters' moments were taken back to front)
    const int *d_ids = (const int *)(E.packet.p + o_ids), *d_cids = (const int *)(E.packet.p + o_cids);
    const int *d_tA0 = (const int *)(E.packet.p + o_tA), *d_tP0 = (const int *)(E.packet.p + o_tP);
    RoundSetup rs{(const NodeIn *)(E.packet.p + o_recs), d_ids, d_tA0, d_tP0, nr, ntA, ntP,
                  E.tilesA.p, E.tilesP.p, E.hist.p, lqs * nr, E.hsize.p, E.hcount.p, (size_t)nr * kBuckets};
    {
        const size_t work = std::max<size_t>(std::max<size_t>(std::max<size_t>(ntP, lqs * nr / 4), (size_t)nr * kNodeResetElems), 256);
        hipLaunchKernelGGL(k_round_setup, (unsigned)std::min<size_t>((work + 255) / 256, 2048), 256, 0, s, E.nodes.p, rs);
        HIP_CHECK(hipGetLastError());
    }
    launch_minmax(C.qlq, E.tilesA.p, ntA, rpx, E.nodes.p, s, rev);
    if (C.sh) shard_exchange_keys(E, d_ids, nr);
    launch_hist(C.qlq, false, E.tilesA.p, ntA, rpx, E.nodes.p, E.hist.p, E.hsize.p, E.hcount.p, s, !rev);
    if (C.sh) {
        comm_sum_dev(E, E.hist.p, lqs * nr, 0);
        if (C.weighted) comm_sum_dev(E, E.hsize.p, (size_t)nr * kBuckets, 1);
        comm_sum_dev(E, E.hcount.p, (size_t)nr * kBuckets, 2);
    }
    launch_cut(C.weighted, E.nodes.p, d_ids, nr, E.hist.p, E.hsize.p, E.hcount.p, E.lut.p, s);
    launch_partition(C.qlq, E.tilesP.p, ntP, rpx, d_ids, d_tP0, nr, E.nodes.p, E.lut.p, E.tilecnt.p, E.tileoff.p, true, s, C.inv_sums, rev);
    if (C.sh) {
        hipLaunchKernelGGL(k_shard_children_local, (nr + 63) / 64, 64, 0, s, E.nodes.p, d_ids, nr);
        HIP_CHECK(hipGetLastError());
        shard_exchange_acc(E, d_cids, 2 * nr);
    }
    laps.lap(laps.enqueue);
    get_nodes_dev(E, d_cids, (int)cids.size(), C.got);
    laps.lap(laps.wait);
    for (size_t i = 0; i < cids.size(); i++) absorb_child(hn[cids[i]], C.got[i]);
    for (int id : todo) { hn[id].split_done = true; E.stats.split_evals++; E.stats.split_px += hn[id].n; }
    for (int id : cids) L.leaves.push_back(id);
    L.F.reload(rec);                                            // the round's nodes are known now
    E.stats.lq_rounds++;
    laps.lap(laps.children);
}

// The greedy loop of local.c:347-390: commit while the step is exact, evaluate a round of candidates when it is blocked
static void lq_host_loop(QuantCall &C, LqHostLoop &L) {
    Engine &E = C.E;
    const std::vector<HNode> &hn = C.hn;
    const HnRec rec{hn};
    SplitFrontier &F = L.F;
    E.stats.split_evals = 0; E.stats.split_px = 0; E.stats.lq_rounds = 0;
    if (F.count >= C.K) return;
    while (F.count < C.K) {
        const SplitFrontier::Step st = F.step(rec, g_debug_fault.load(std::memory_order_relaxed));
        if (st.status == SplitFrontier::kBlocked) { lq_host_round(C, L); continue; }
        if (st.status == SplitFrontier::kStopped) { E.trace_hdr.stopped_early = 1; break; }   // benefit < DELTA: stop, keep `count` clusters
        const HNode &h = hn[st.commit.node];
        const int l = st.commit.left, r = l + 1;
        patolette_amd__SplitRecord tr{};
        tr.row = st.commit.row; tr.new_row = st.commit.new_row;
        tr.split = hn[l].psplit < 0 ? -1 : (hn[l].psplit & 0xffff); tr.degenerate = hn[l].psplit < 0 ? 0 : (hn[l].psplit >> 16) & 1;
        tr.n = h.gn; tr.n_left = hn[l].gn; tr.n_right = hn[r].gn; tr.sw = h.sw;
        for (int j = 0; j < 3; j++) tr.axis[j] = h.axis[j];
        for (int q = 0; q < 6; q++) tr.cov6[q] = h.cov6[q] / h.sw;
        tr.dist = h.dist; tr.dist_left = hn[l].dist; tr.dist_right = hn[r].dist; tr.benefit = st.benefit;
        E.trace.push_back(tr);
        if (C.verbose) { printf("patolette ======== Processed colors: %zu\r", F.count); fflush(stdout); }   // local.c:386-389
    }
    const LqLaps &t = L.laps;
    if (t.on) fprintf(stderr, "patolette_amd: split loop host ms: greedy %.3f select %.3f axes %.3f packet %.3f enqueue %.3f wait(gpu) %.3f children %.3f\n",
                      t.greedy, t.select, t.axes, t.packet, t.enqueue, t.wait, t.children);
}

// PALETTE_create (create.c:11-33) over the frontier's rows, the largest cluster, the stats
static void lq_host_epilogue(QuantCall &C, const SplitFrontier &F) {
    Engine &E = C.E;
    const std::vector<HNode> &hn = C.hn;
    const size_t len = C.len = F.count;
    C.centers.assign(3 * len, 0.0);
    for (size_t i = 0; i < len; i++) for (int j = 0; j < 3; j++) C.centers[(size_t)j * len + i] = hn[F.result[i]].mean[j];   // create.c:11-33
    if (C.max_members) { *C.max_members = 0; for (size_t i = 0; i < len; i++) *C.max_members = std::max(*C.max_members, hn[F.result[i]].gn); }
    E.stats.n_clusters = len;
    E.trace_hdr.n_clusters = (int32_t)len; E.trace_hdr.n_records = (int32_t)E.trace.size();
    E.cluster_centers = C.centers;
    E.stats.ms_lq = now_ms() - C.t0;
}

static int quantize_clusters_run(Engine &E, size_t N, size_t K, bool weighted, const Bounds &bnd,
                                 std::vector<double> &centers, size_t &len, bool verbose, unsigned long long *max_members, bool allow_device) {
    const size_t planes = weighted ? 4 : 3;
    const Shard *sh = E.shard;                                  // the image is dealt out over a group of GPUs: N is this GPU's part
    if (E.prep_N != N || E.prep_planes != planes) gq_prepare(E, N, weighted);   // (the stage-level entry points come here unprepared)
    E.prep_N = 0;
    // PAMD_LQ_DEVICE=0: the host-driven split loop everywhere (A/B, and what sliced images, K > 256 and verbose calls always take)
    const bool dev_eligible = lq_device_eligible(E, N, K, verbose, allow_device);
    E.nodes.reserve(std::max<size_t>(4 * K + 64, dev_eligible ? (size_t)kLqNodeCap : 0));
    const QuantSizes root(N, planes, 1);
    QuantCall C{E, N, sh ? sh->total : N, K, weighted, sh || E.invariant, verbose, dev_eligible, sh, bnd, centers, len, max_members,
                QuantBuffers{{E.cvt.p, E.bufA.p}, E.bkt.p, N, weighted}, QuantBuffers{{E.bufB.p, E.bufA.p}, E.bkt.p, N, weighted},
                (int)root.tilesA, (int)root.tilesP, hist_slot_doubles(), now_ms()};
    C.hn.reserve(4 * K + 64);

    gq_root_mean(C);
    gq_root_covariance(C);
    if (!gq_root_histogram(C)) return -1;
    const bool gq_dev = g_gq_device.load(std::memory_order_relaxed) != 0 && !sh && !verbose && K > (size_t)kGqMaxK;
    const int rc = gq_dev ? gq_device_turn(C) : gq_host_turn(C);
    if (rc != kHostLoop) return rc;                             // failed, or the device-driven split loop has finished the call
    E.stats.n_base_clusters = (size_t)C.kbase;
    if (verbose) printf("patolette ======== Base cluster count: %zu\n", (size_t)C.kbase);     // patolette.c:227-229
    E.stats.ms_gq = now_ms() - C.t0;
    C.t0 = now_ms();

    LqHostLoop L{SplitFrontier(K, C.kbase, C.base_ids[0], kDelta, HnRec{C.hn}), C.base_ids, LqLaps{}};
    lq_host_loop(C, L);
    lq_host_epilogue(C, L.F);
    return 0;
}

static int quantize_clusters(Engine &E, size_t N, size_t K, bool weighted, const Bounds &bnd,
                             std::vector<double> &centers, size_t &len, bool verbose = false, unsigned long long *max_members = nullptr) {
    WsGuard wg(&E.stream, &E.stream2);
    int rc = quantize_clusters_run(E, N, K, weighted, bnd, centers, len, verbose, max_members, true);
    if (rc == -2) {                                             // the device-driven loop ran out of node records: once more, host-driven
        E.prep_N = 0;
        rc = quantize_clusters_run(E, N, K, weighted, bnd, centers, len, verbose, max_members, false);
    }
    return rc;
}

// --------------------------------------------------------------------------------------------
// KMeans refinement (refine.c:165-221); centres planar (k,3) f64 in/out
// --------------------------------------------------------------------------------------------
// largest_cluster: pixels of the most populous cluster the centres come from (0 = unknown): a dominant colour means one very long
// centroid chain, and the iterations then take the sorted path with the block-parallel chain from the start (kmeans_iterate)
// patolette_amd_set_kmeans_update: process-wide (the batch entry's helper threads must see the caller's choice).  -1: not set, the
// environment's default (PAMD_KMEANS_UPDATE)
std::atomic<int> g_km_update{-1};
// patolette_amd_set_subsample_cache: 1 (default) keep the subsample list on the device between calls on images of one size;
// 0 every call makes it again (on the helper thread): what a first call of a size costs, call after call
std::atomic<int> g_perm_cache{1};

// Call entry: if this image will be subsampled (assuming the quantisers deliver all K clusters; fewer only shorten the list),
// start making the list on a helper thread.  take = the longest list any cluster count <= K can ask for: min(ms, N).
static void subsample_start(Engine &E, size_t Nt, size_t K, size_t max_samples) {
    if (E.perm_job.valid()) {                                                   // a job left behind by a call that threw
        try { E.perm_job.get(); } catch (...) { E.hperm_N = 0; E.hperm_nx = 0; }   // ... and that may itself have failed: its list is void then
    }
    const size_t ms = std::max(max_samples, (size_t)(256 * 256));                // refine.c:21
    if (K == 0 || Nt < K) return;
    const size_t nxK = K * (size_t)(int)(ms / K);
    if (!(Nt > nxK)) return;                                                     // Clustering.cpp:311: no subsampling
    const size_t take = std::min(ms, Nt);
    if (!g_perm_cache.load(std::memory_order_relaxed)) { E.perm_N = 0; E.perm_nx = 0; E.hperm_N = 0; E.hperm_nx = 0; }
    if (E.perm_N == Nt && E.perm_nx >= nxK) return;                              // on the device already
    if (E.hperm_N == Nt && E.hperm_nx >= nxK) return;
    E.h_perm.reserve(take);
    E.hperm_N = 0; E.hperm_nx = 0;
    int32_t *dst = E.h_perm.p;
    hm::PermScratch *ws = &E.perm_ws;
    E.perm_job = std::async(std::launch::async, [dst, Nt, take, ws] { hm::rand_perm_prefix(Nt, take, 1234u, dst, *ws); });   // random.cpp:184-194
    E.hperm_N = Nt; E.hperm_nx = take;                                           // valid once perm_job has been waited for
}
// The KMeans stage: the first nx entries of rand_perm(Nt) on the device; no stream synchronisation (pinned staging)
static const int *subsample_list(Engine &E, size_t Nt, size_t nx, hipStream_t s) {
    if (E.perm_job.valid()) {
        try { E.perm_job.get(); } catch (...) { E.hperm_N = 0; E.hperm_nx = 0; throw; }
    }
    if (E.perm_N == Nt && E.perm_nx >= nx) return E.perm_dev.p;
    if (!(E.hperm_N == Nt && E.hperm_nx >= nx)) {                                // no helper was started (a stage-level call, fewer clusters than K)
        E.h_perm.reserve(nx);
        hm::rand_perm_prefix(Nt, nx, 1234u, E.h_perm.p, E.perm_ws);
        E.hperm_N = Nt; E.hperm_nx = nx;
    }
    E.perm_dev.reserve(E.hperm_nx);
    HIP_CHECK(hipMemcpyAsync(E.perm_dev.p, E.h_perm.p, E.hperm_nx * sizeof(int), hipMemcpyHostToDevice, s));
    E.perm_N = Nt; E.perm_nx = E.hperm_nx;
    return E.perm_dev.p;
}
static bool km_update_order_free() {
    static const bool env = getenv("PAMD_KMEANS_UPDATE") && atoi(getenv("PAMD_KMEANS_UPDATE")) != 0;
    const int v = g_km_update.load(std::memory_order_relaxed);
    return v < 0 ? env : v != 0;
}
// The domain in which every f32 intermediate of an iteration stays finite (patolette_amd.h, patolette_amd_kmeans_refine states the
// rule).  Outside it an assignment kernel can return index -1 (every candidate distance NaN: |x|^2 = +inf, or every centre NaN after
// a sum overflowed or 1 / h met a subnormal h), which then indexes counters and the sorted copy.
//   B = max(1, |x|, |initial centre|); m = min(nx, 2^25): a chain of non-negative addends <= T stops growing at 2^25 T, and below
//   that its roundings add at most a factor e^2.  A weighted centre is acc / h with |acc| <= (1 + e)^n sum w |x| and
//   h >= (1 - e)^n sum w (e = 2^-24, recursive summation of non-negative terms): |centre| <= exp(n 2^-23) B whatever the weights;
//   also h >= the smallest positive weight, so |centre| <= 4 m (wmax / wmin) B.  Cb = 4 x the smaller of the two (the +-1/1024
//   nudges of split_clusters, at most one per halving of a size: < 1.14; the rounding of 1 / h and of the product);
//   unweighted the count is exact or stuck at 2^24: Cb = 8 B.  A distance is at most |x|^2 + |y|^2 + 2 |x.y| <= 12 Cb^2.
// min_w: the smallest positive weight as f32, 0 = there is none (every cluster is empty: centres 0)
static bool km_domain_ok(const double bound_x, const double bound_c, const bool weighted, const double bound_w, const double min_w, const size_t nx) {
    const double fmax = 3.4028234663852886e38, fmin = 1.1754943508222875e-38;
    const double B = std::max(1.0, std::max(bound_x, bound_c)), m = (double)std::min<size_t>(nx, (size_t)1 << 25);
    if (!(B < fmax) || !(bound_w < fmax)) return false;
    double Cb = 8.0 * B;
    if (weighted) {
        if (min_w > 0 && min_w < fmin) return false;                              // 1 / h overflows from a subnormal h
        const double by_n = std::exp(std::min((double)nx * 0x1p-23, 700.0)) * B;
        Cb = 4.0 * (min_w > 0 ? std::min(by_n, 4.0 * m * (std::max(bound_w, min_w) / min_w) * B) : by_n);
    }
    Cb += 8.0;                                                                     // products w x that underflow: <= m 2^-149 / 2^-126
    return 16.0 * Cb * Cb <= fmax && 4.0 * m * std::max(bound_w, 1.0) * B <= fmax;
}
// bound_x / bound_w: upper bounds of |colour value| and of the weights over the image (the order-free update scales by them)
// min_w: the smallest positive weight as f32, 0 = none; bad_w: a weight is negative or not finite as f32
static void kmeans_refine(Engine &E, size_t N, bool weighted, std::vector<double> &centers, size_t k, int niter, size_t max_samples,
                          bool nonfinite, unsigned long long largest_cluster, double bound_x, double bound_w, double min_w = 0, bool bad_w = false) {
    hipStream_t s = E.stream;
    E.km.route = 0;
    const KmSums sums_v{bound_x, bound_w};
    const KmSums *sums = km_update_order_free() ? &sums_v : nullptr;
    std::vector<float> cent(3 * k);
    for (size_t i = 0; i < k; i++) for (int j = 0; j < 3; j++) cent[3 * i + j] = (float)centers[(size_t)j * k + i];   // refine.c:102-125
    const size_t min_samples = 256 * 256;                                          // refine.c:21
    const size_t ms = std::max(max_samples, min_samples);
    const int mppc = (int)(ms / k);                                                // refine.c:87
    // Clustering.cpp:272-278 (fewer points than centroids) and :295-304 (a NaN / Inf among the f32 inputs) throw; refine.c:91
    // swallows the exception and the palette stays the initial centres
    const Shard *sh = E.shard;                                                     // sliced image: N is this GPU's part, the sample set is the whole image's
    const size_t Nt = sh ? sh->total : N;
    auto expect_longest = [&](size_t nx_) { return (size_t)((double)largest_cluster / (double)(Nt ? Nt : 1) * (double)nx_); };
    bool ok = Nt >= k && !nonfinite && !bad_w;
    size_t nx = Nt;
    E.stats.kmeans_samples = 0;
    const bool sub = ok && Nt > k * (size_t)mppc;                                  // Clustering.cpp:311-319
    if (sub) nx = k * (size_t)mppc;
    // DEPARTURES (patolette_amd.h): a subsample of fewer than k + 1 samples (k > max_samples: 0 of them) -- the reference's
    // split_clusters then walks for ever with n - k wrapped; and input outside the finite domain
    if (ok && sub && nx < k + 1) ok = false;
    if (ok && nx != k) {
        double bound_c = 0;
        for (size_t i = 0; i < 3 * k; i++) bound_c = std::max(bound_c, std::fabs((double)cent[i]));
        for (size_t i = 0; i < 3 * k && ok; i++) ok = std::isfinite(cent[i]);
        ok = ok && km_domain_ok(bound_x, bound_c, weighted, bound_w, min_w, nx);
    }
    if (ok) {
        E.km.reserve(nx, (int)k);
        const int *dperm = nullptr;
        if (sub) dperm = subsample_list(E, Nt, nx, s);                            // faiss draws the subsample from rand_perm(N, seed 1234)
        if (sh) {
            // every GPU contributes the samples that fall into its slice (zero bits elsewhere); the integer SUM of the bit
            // patterns hands every GPU the whole sample set, and each runs the same deterministic iterations on it
            kmeans_gather_slice(E.cvt.p, N, weighted, dperm, nx, sh->begin, E.km, s);
            comm_sum_dev(E, E.km.sx.p, nx, 2); comm_sum_dev(E, E.km.sy.p, nx, 2); comm_sum_dev(E, E.km.sz.p, nx, 2);
            if (weighted) comm_sum_dev(E, E.km.sw.p, nx, 2);
            if (nx == k) {                                                         // Clustering.cpp:331-352: centroids = first k input vectors
                std::vector<float> f(3 * k);
                HIP_CHECK(hipMemcpy(f.data(), E.km.sx.p, k * sizeof(float), hipMemcpyDeviceToHost));
                HIP_CHECK(hipMemcpy(f.data() + k, E.km.sy.p, k * sizeof(float), hipMemcpyDeviceToHost));
                HIP_CHECK(hipMemcpy(f.data() + 2 * k, E.km.sz.p, k * sizeof(float), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < k; i++) for (int j = 0; j < 3; j++) cent[3 * i + j] = f[(size_t)j * k + i];
            } else {
                HIP_CHECK(hipMemcpyAsync(E.km.cent.p, cent.data(), 3 * k * sizeof(float), hipMemcpyHostToDevice, s));
                HIP_CHECK(hipStreamSynchronize(s));
                kmeans_iterate(E.km, nx, (int)k, weighted, niter, s, expect_longest(nx), sums);
                HIP_CHECK(hipMemcpyAsync(cent.data(), E.km.cent.p, 3 * k * sizeof(float), hipMemcpyDeviceToHost, s));
                E.sync();
                E.stats.kmeans_samples = nx;
            }
        } else if (nx == k) {                                                      // Clustering.cpp:331-352: centroids = first k input vectors
            std::vector<double> first(3 * k);
            for (int j = 0; j < 3; j++) HIP_CHECK(hipMemcpy(first.data() + (size_t)j * k, E.cvt.p + (size_t)j * N, k * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < k; i++) for (int j = 0; j < 3; j++) cent[3 * i + j] = (float)first[(size_t)j * k + i];
        } else {
            kmeans_gather(E.cvt.p, N, weighted, dperm, nx, E.km, s);
            E.h_cent.reserve(3 * k);                                               // pinned: no synchronisation before the iterations
            std::memcpy(E.h_cent.p, cent.data(), 3 * k * sizeof(float));
            HIP_CHECK(hipMemcpyAsync(E.km.cent.p, E.h_cent.p, 3 * k * sizeof(float), hipMemcpyHostToDevice, s));
            kmeans_iterate(E.km, nx, (int)k, weighted, niter, s, expect_longest(nx), sums);
            HIP_CHECK(hipMemcpyAsync(E.h_cent.p, E.km.cent.p, 3 * k * sizeof(float), hipMemcpyDeviceToHost, s));
            E.sync();
            std::memcpy(cent.data(), E.h_cent.p, 3 * k * sizeof(float));
            E.stats.kmeans_samples = nx;
        }
    }
    for (size_t i = 0; i < k; i++) for (int j = 0; j < 3; j++) centers[(size_t)j * k + i] = (double)cent[3 * i + j];   // refine.c:202-212
}

static void palette_rows(std::vector<double> &pal, size_t len, void (*f)(double[3])) {
    for (size_t i = 0; i < len; i++) {
        double c[3] = {pal[i], pal[len + i], pal[2 * len + i]};
        f(c);
        pal[i] = c[0]; pal[len + i] = c[1]; pal[2 * len + i] = c[2];
    }
}

// pal's `rows` rows into E.dpal, which the caller has reserved as it has E.h_pal.  From a pinned copy: no wait for the transfer (a
// pageable source is staged and waited for, ~15 us with nothing queued behind it); the copy is this engine's and is next written by
// its next call, after this one's final synchronisation
static void upload_palette(Engine &E, const std::vector<double> &pal, size_t rows) {
    std::memcpy(E.h_pal.p, pal.data(), 3 * rows * sizeof(double));
    HIP_CHECK(hipMemcpyAsync(E.dpal.p, E.h_pal.p, 3 * rows * sizeof(double), hipMemcpyHostToDevice, E.stream));
}

// between_copy_and_wait: work to enqueue behind the statistics' download while the host is still waiting for it
static Bounds read_bounds(Engine &E, bool weighted, const std::function<void()> &between_copy_and_wait = nullptr) {
    E.h_cstats.reserve(1);
    HIP_CHECK(hipMemcpyAsync(E.h_cstats.p, E.cstats.p, sizeof(ConvertStats), hipMemcpyDeviceToHost, E.stream));
    if (between_copy_and_wait) {                               // wait for the download alone, not for what is enqueued behind it
        if (!E.ev_stats) HIP_CHECK(hipEventCreateWithFlags(&E.ev_stats, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(E.ev_stats, E.stream));
        between_copy_and_wait();
        HIP_CHECK(hipEventSynchronize(E.ev_stats));
    } else E.sync();
    const ConvertStats &cs = *E.h_cstats.p;
    Bounds b;
    b.cmax = 0; b.range = 0;
    unsigned long long kmin[3], kmax[3], kw = 0ULL, nonfinite = cs.nonfinite_f32 != 0u ? 1ULL : 0ULL;
    double parts[3][2];
    for (int p = 0; p < 3; p++) {
        kmin[p] = ~0ULL; kmax[p] = 0ULL;
        for (int t = 0; t < kStatSlots; t++) { kmin[p] = std::min(kmin[p], cs.minkey[t][p]); kmax[p] = std::max(kmax[p], cs.maxkey[t][p]); }
        parts[p][0] = 0; parts[p][1] = 0;                      // slot partials are exact multiples of the bin grids
        for (int t = 0; t < kStatSlots; t++) { parts[p][0] += cs.sum[t][p][0]; parts[p][1] += cs.sum[t][p][1]; }
    }
    unsigned long long kwmin = ~0ULL, bad_w = weighted && cs.bad_weight != 0u ? 1ULL : 0ULL;
    for (int t = 0; t < kStatSlots; t++) { kw = std::max(kw, cs.wmaxkey[t]); kwmin = std::min(kwmin, cs.wminkey[t]); }
    if (E.shard) {                                             // one image over several GPUs: the bounds and sums of ALL its pixels
        const unsigned long long mine[10] = {kmin[0], kmin[1], kmin[2], kmax[0], kmax[1], kmax[2], kw, nonfinite, kwmin, bad_w};
        const std::vector<unsigned long long> all = comm_gather_u64(E, mine, 10);
        for (int r = 0; r < E.shard->comm.size; r++) {
            const unsigned long long *row = all.data() + (size_t)r * 10;
            for (int p = 0; p < 3; p++) { kmin[p] = std::min(kmin[p], row[p]); kmax[p] = std::max(kmax[p], row[3 + p]); }
            kw = std::max(kw, row[6]); nonfinite |= row[7]; kwmin = std::min(kwmin, row[8]); bad_w |= row[9];
        }
        comm_sum_host(E, &parts[0][0], 6, 0);
    }
    for (int p = 0; p < 3; p++) {
        const unsigned long long ka = kmin[p], kb = kmax[p];
        double mn = key_f64(ka), mx = key_f64(kb);
        if (!(mn <= mx)) { mn = 0; mx = 0; }
        b.lo[p] = mn; b.hi[p] = mx;
        b.cmax = std::max(b.cmax, std::max(std::fabs(mn), std::fabs(mx)));
        b.range = std::max(b.range, mx - mn);
    }
    b.wmax = weighted ? std::max(1.0, key_f64(kw)) : 1.0;
    b.wmin = weighted && std::isfinite(key_f64(kwmin)) ? key_f64(kwmin) : 0.0;
    b.bad_w = bad_w != 0ULL;
    const double lin = b.wmax * std::max(b.cmax, 1.0);
    const double quad = 3.0 * b.wmax * std::max(std::max(b.range, b.cmax), 1e-300) * std::max(std::max(b.range, b.cmax), 1e-300);
    b.e_lin = exp_bound(lin);
    b.e_quad = exp_bound(std::max(quad, 1e-300));
    for (int p = 0; p < 3; p++) { b.sum[p] = parts[p][0] + parts[p][1]; b.sum2[p][0] = parts[p][0]; b.sum2[p][1] = parts[p][1]; }
    for (int q = 0; q < 6; q++)
        for (int t = 0; t < kStatSlots; t++) { b.mom2[q][0] += cs.mom[t][q][0]; b.mom2[q][1] += cs.mom[t][q][1]; }   // exact: parts on the grids
    b.nonfinite = nonfinite != 0ULL;
    return b;
}

// --------------------------------------------------------------------------------------------
// the full path, inputs resident in HBM
// --------------------------------------------------------------------------------------------
// The RGBA entry's compact image: the pipeline runs on the M opaque pixels as an M x 1 image, and the dither walks the width x height
// curve over them (DitherJob's cpos: cpos[pixel] = compact number or -1)
struct DitherMask { size_t width, height; const int *cpos; };
// The frames entry's stack: the pipeline runs on count * width * height pixels as ONE image of width x (count * height) -- the palette
// stage sees a list of colours, the nearest map is position-independent -- and only the dither knows the frames: each is walked along
// its own width x height curve from the empty queue (DitherJob's frames)
struct Frames { size_t count, width, height; };

struct Pixels {                      // device-resident input image: planar f64 sRGB, or interleaved 8-bit sRGB
    const double *f64 = nullptr;
    const unsigned char *u8 = nullptr;
    int channels = 3;
    bool rows = false;               // f64 as (N,3) row-major instead of planar
    bool converted = false;          // E.cvt already holds the converted image and E.cstats its statistics (upload_image: chunk by chunk behind the upload)
};

// What stage S1 launches: the conversion and the sums that ride with it (run_device; upload_image when it converts behind the upload)
struct ConvertPlan { int which; BinK sumk, momk; };
static ConvertPlan convert_plan(const Engine &E, const patolette__QuantizationOptions *opt, size_t N) {
    ConvertPlan p{PAMD_COPY, BinK{0.0, 0.0}, BinK{0.0, 0.0}};
    if (opt->color_space == patolette__CIELuv) p.which = PAMD_SRGB_TO_CIELUV;
    else if (opt->color_space == patolette__ICtCp) p.which = PAMD_SRGB_TO_ICTCP;
    // the root mean of the global quantiser (matrix2D.c:229) rides along with the conversion where the colour space bounds
    // the values a priori: |I| <= 1, |Ct|, |Cp| <= 0.5 (2^1); L <= 100, |u|, |v| < 256 (2^8).  sRGB passes user data through.
    const size_t Nt = E.shard ? E.shard->total : N;            // a slice sums on the grids of the whole image
    int rootP = 1; while ((1ULL << rootP) < (Nt > 1 ? Nt : 2)) rootP++;
    if (p.which == PAMD_SRGB_TO_ICTCP) p.sumk = make_bink(1, rootP);
    else if (p.which == PAMD_SRGB_TO_CIELUV) p.sumk = make_bink(8, rootP);
    // one GPU: the raw second moments ride along too (products < 1, resp. < 2^16), and the root's covariance needs no sweep
    if (!E.shard) {
        if (p.which == PAMD_SRGB_TO_ICTCP) p.momk = make_bink(1, rootP);
        else if (p.which == PAMD_SRGB_TO_CIELUV) p.momk = make_bink(16, rootP);
    }
    return p;
}
// Stage S1's launch for a device image as `px` describes it, into E.cvt / E.cstats on stream s: the whole image, or the pixels
// [lo, hi) of it (upload_image's pieces; `first`: the launch that initialises the statistics)
static void convert_pixels(Engine &E, const ConvertPlan &cp, const Pixels &px, size_t N, hipStream_t s, size_t lo = 0, size_t hi = ~(size_t)0,
                           bool first = true) {
    if (px.u8) launch_convert_u8(cp.which, px.u8, px.channels, E.cvt.p, N, E.cstats.p, s, cp.sumk, cp.momk, lo, hi, first);
    else if (px.rows) launch_convert_rows(cp.which, px.f64, E.cvt.p, N, E.cstats.p, s, cp.sumk, cp.momk, lo, hi, first);
    else launch_convert(cp.which, px.f64, E.cvt.p, N, E.cstats.p, s, cp.sumk, cp.momk, lo, hi, first);
}

// A palette's write-out (patolette.c:327-336): K rows, planar -- `off` rows of zeros (the RGBA entry's transparent row), the `rows`
// rows of `pal` (planar with that stride), -1 for the unused ones
static void write_palette(double *out, size_t K, size_t off, const std::vector<double> &pal, size_t rows) {
    for (size_t j = 0; j < K * 3; j++) out[j] = j % K < off ? 0.0 : -1.0;
    for (int j = 0; j < 3; j++) for (size_t i = 0; i < rows; i++) out[K * (size_t)j + off + i] = pal[(size_t)j * rows + i];
}

// the dither launchers' counters of their last walk, added to the call's statistics (which start at zero: a call of one walk gets
// that walk's counters, run_remap_rgba's frame-by-frame walks their sums)
static void add_dither_stats(Engine &E) {
    E.stats.dither_segments += E.nn.dither_segments; E.stats.dither_repairs += E.nn.dither_repairs; E.stats.dither_rounds += E.nn.dither_rounds;
    E.stats.dither_through += E.nn.dither_through; E.stats.dither_jumps += E.nn.dither_jumps; E.stats.dither_solo += E.nn.dither_solo;
}
// whether the map stage writes the map at all: a 1x1 dither visits nothing (riemersma.c:452-456)
static bool map_touched(bool dither, size_t width, size_t height) { return !(dither && std::max(width, height) <= 1); }

static void run_device(Engine &E, size_t width, size_t height, Pixels px, const double *d_weights, size_t K,
                       const patolette__QuantizationOptions *opt, double *palette, void *d_map, int map_elem, const DitherMask *mask = nullptr,
                       const Frames *frames = nullptr) {
    // d_map == nullptr with palette_only unset: the palette takes the same conversions, the map kernels are skipped
    hipStream_t s = E.stream;
    const size_t N = width * height;
    const bool weighted = d_weights != nullptr;
    const double t_start = now_ms();
    WsGuard wg(&E.stream, &E.stream2);
    E.stats = patolette_amd__Stats{};
    E.prep_N = 0;
    ws_prepare(E, N, K, weighted, opt->verbose);
    if (opt->kmeans_niter > 0) subsample_start(E, E.shard ? E.shard->total : N, K, opt->kmeans_max_samples);
    // S1: colour conversion into the working image (x|y|z|w planar), patolette.c:201-207
    double t0 = now_ms();                                        // (E.cvt and E.cstats: ws_prepare)
    if (E.shard && opt->dither && !opt->palette_only)
        throw HipError("patolette_amd: dithering walks the whole image along one curve; it is not available per slice");
    const ConvertPlan cp = convert_plan(E, opt, N);
    if (!px.converted) convert_pixels(E, cp, px, N, s);          // (else upload_image has converted the image chunk by chunk behind its upload)
    if (weighted) {
        HIP_CHECK(hipMemcpyAsync(E.cvt.p + 3 * N, d_weights, N * sizeof(double), hipMemcpyDeviceToDevice, s));
        launch_weight_stats(d_weights, N, E.cstats.p, s);
    }
    // the quantiser's size-only preparations go behind the statistics' download: they run while the host derives the bounds
    Bounds bnd = read_bounds(E, weighted, [&] { gq_prepare(E, N, weighted); });
    bnd.have_sum = cp.sumk.M0 != 0.0;
    bnd.have_mom = cp.momk.M0 != 0.0;
    E.stats.ms_convert = now_ms() - t0;

    // S2 + S3: global + local quantiser (progress lines as patolette.c:209-229 prints them when verbose)
    if (opt->verbose) printf("patolette ======== Palette generation \n");
    std::vector<double> pal;
    size_t len = 0;
    unsigned long long largest_cluster = 0;
    if (quantize_clusters(E, N, K, weighted, bnd, pal, len, opt->verbose, &largest_cluster) != 0) throw HipError("internal quantization error");

    // S4: optional KMeans refinement
    t0 = now_ms();
    if (opt->kmeans_niter > 0) {
        if (opt->verbose) printf("patolette ======== KMeans refinement\n");                // patolette.c:249-251
        kmeans_refine(E, N, weighted, pal, len, opt->kmeans_niter, opt->kmeans_max_samples, bnd.nonfinite, largest_cluster, bnd.cmax, bnd.wmax, bnd.wmin, bnd.bad_w);
    }
    E.stats.ms_kmeans = now_ms() - t0;

    // S5: palette map
    t0 = now_ms();
    if (!opt->palette_only) {
        E.dpal.reserve(3 * len);
        if (opt->verbose) printf(opt->dither ? "patolette ======== Dithering\n" : "patolette ======== NN mapping\n");
        if (opt->dither) {                                                     // patolette.c:268-299
            int pix = PAMD_SRGB_TO_REC2020;
            void (*pf)(double[3]) = hm::color::srgb_to_rec2020;
            if (opt->color_space == patolette__CIELuv) { pix = PAMD_CIELUV_TO_REC2020; pf = hm::color::cieluv_to_rec2020; }
            else if (opt->color_space == patolette__ICtCp) { pix = PAMD_ICTCP_TO_REC2020; pf = hm::color::ictcp_to_rec2020; }
            palette_rows(pal, len, pf);
            E.map_palette = pal;
            if (d_map) {
                HIP_CHECK(hipMemcpyAsync(E.dpal.p, pal.data(), 3 * len * sizeof(double), hipMemcpyHostToDevice, s));
                HIP_CHECK(hipStreamSynchronize(s));
                // (masked: this image is the M x 1 list of opaque pixels, and the layout is decided on M as well)
                DitherJob job;
                job.width = width; job.height = height;
                if (mask) { job.width = mask->width; job.height = mask->height; job.cpos = mask->cpos; job.opaque = N; }
                else if (frames) { job.frames = frames->count; job.width = frames->width; job.height = frames->height; }
                job.d_pal = E.dpal.p; job.h_pal = pal.data(); job.k = (int)len;
                job.out = d_map; job.elem_bytes = map_elem;
                job.plane_stride = N;                                          // plane stride of cvt is N for x,y,z
                if (frames ? dither_frames_lane_layout(frames->count, frames->width, frames->height, (int)len)
                           : dither_lane_layout(width, height, (int)len)) {      // decided ONCE: launch_dither is told
                    // the pixels go into curve order anyway: their conversion to linear Rec2020 rides on that pass
                    job.planes = E.cvt.p; job.which = pix; job.layout = 1;
                } else {
                    E.aux.reserve(3 * N);
                    launch_convert(pix, E.cvt.p, E.aux.p, N, nullptr, s);
                    job.planes = E.aux.p; job.which = PAMD_COPY; job.layout = 0;
                }
                launch_dither(job, E.nn, s);
                add_dither_stats(E);
            }
            palette_rows(pal, len, hm::color::rec2020_to_srgb);
        } else {                                                               // patolette.c:300-324
            const double *pixels = E.cvt.p;
            const double *blo = bnd.lo, *bhi = bnd.hi;                         // exact min/max of the pixels being mapped
            Bounds b2;
            if (opt->color_space == patolette__CIELuv) {
                if (d_map) {
                    E.aux.reserve(3 * N);
                    launch_convert(PAMD_CIELUV_TO_ICTCP, E.cvt.p, E.aux.p, N, E.cstats.p, s);
                    b2 = read_bounds(E, false);
                    blo = b2.lo; bhi = b2.hi;
                    pixels = E.aux.p;
                }
                palette_rows(pal, len, hm::color::cieluv_to_rec2020);
                palette_rows(pal, len, hm::color::rec2020_to_srgb);
                palette_rows(pal, len, hm::color::srgb_to_ictcp);
            }
            E.map_palette = pal;
            if (d_map) {
                E.h_pal.reserve(3 * len);
                upload_palette(E, pal, len);
                launch_nn_map(pixels, N, N, E.dpal.p, (int)len, d_map, map_elem, blo, bhi, E.nn, s);
            }
            palette_rows(pal, len, hm::color::ictcp_to_rec2020);
            palette_rows(pal, len, hm::color::rec2020_to_srgb);
        }
        E.sync();
    }
    E.stats.ms_map = now_ms() - t0;
    // S6: palette write-out, unused rows = -1
    write_palette(palette, K, 0, pal, len);
    E.stats.ms_total = now_ms() - t_start;
}

struct CodeError : std::runtime_error {        // failure with a dedicated exit code (saliency stage)
    int code;
    CodeError(int c, const char *m) : std::runtime_error(m), code(c) {}
};

// weights the Python binding derives when tile_size > 0 (patolette.pyx:407-414), left on the device
// frames > 1 (8-bit input only): that many width x height images one after another, each weighted as an image of its own
static const double *derive_weights(Engine &E, const double *d_f64, const unsigned char *d_u8, int channels, size_t width,
                                    size_t height, double tile_size, size_t frames = 1) {
    const size_t n = width * height;
    E.wsal.reserve(frames * n);
    const double t0 = now_ms();
    int rc = kSalOk;
    for (size_t f = 0; f < frames && rc == kSalOk; f++)
        rc = saliency_weights(E.sal, d_f64, d_u8 ? d_u8 + f * n * (size_t)channels : nullptr, channels, width, height, tile_size, E.wsal.p + f * n,
                              E.stream);
    if (ktimer().enabled) ktimer().collect();
    E.ms_saliency = now_ms() - t0;
    if (rc == kSalBadShape) throw CodeError(-5, "saliency weights: image shape not supported");
    if (rc == kSalSingular) throw CodeError(-6, "saliency weights: singular border covariance");
    if (rc == kSalDegenerate) throw CodeError(-7, "saliency weights: degenerate saliency map");
    return E.wsal.p;
}

static int validate(size_t width, size_t height, size_t K) {               // patolette.c:61-95
    const size_t px = width * height;
    if (px == 0) return -2;
    if (K < 1) return -3;
    if (px > (size_t)40000 * 40000) return -4;
    return 0;
}

static int map_elem_for(size_t K) { return K <= 256 ? 1 : 4; }

// The C ABI hands the index map back as size_t (patolette.h: `size_t *palette_map`): 8 bytes per pixel on the host for 1 (or
// 4) on the device.  The narrow map crosses PCIe in chunks through pinned staging while a few host threads widen the
// previous chunk into the caller's buffer.
static void download_map_widened(Engine &E, const void *d_map, int me, size_t N, size_t *out) {
    if (N == 0) return;
    const size_t chunk = (size_t)2 << 20;                                   // elements per chunk
    const size_t nchunks = ceil_div(N, chunk);
    E.h_mapstage.reserve(2 * chunk * (size_t)me);
    const int T = (int)std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)std::thread::hardware_concurrency(), ceil_div(N, (size_t)1 << 18)}));
    std::atomic<size_t> ready{0};
    std::vector<std::atomic<int>> done(nchunks);
    for (auto &d : done) d.store(0);
    std::atomic<bool> failed{false};
    auto worker = [&](int tid) {
        for (size_t c = 0; c < nchunks; c++) {
            while (ready.load(std::memory_order_acquire) <= c) {
                if (failed.load(std::memory_order_relaxed)) return;
                std::this_thread::yield();
            }
            const size_t lo = c * chunk, cnt = std::min(chunk, N - lo);
            const size_t a = cnt * (size_t)tid / (size_t)T, b = cnt * (size_t)(tid + 1) / (size_t)T;
            const unsigned char *src = E.h_mapstage.p + (c & 1) * chunk * (size_t)me;
            given_elems_out(src, me, out + lo, 8, a, b);
            done[c].fetch_add(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < T; t++) pool.emplace_back(worker, t);
    auto issue = [&](size_t c) {
        const size_t lo = c * chunk, cnt = std::min(chunk, N - lo);
        HIP_CHECK(hipMemcpyAsync(E.h_mapstage.p + (c & 1) * chunk * (size_t)me, (const unsigned char *)d_map + lo * (size_t)me, cnt * (size_t)me,
                                 hipMemcpyDeviceToHost, E.stream));
    };
    try {
        issue(0);
        for (size_t c = 0; c < nchunks; c++) {
            HIP_CHECK(hipStreamSynchronize(E.stream));
            ready.store(c + 1, std::memory_order_release);
            if (c + 1 < nchunks) {
                // chunk c+1 reuses the half chunk c-1 was staged in: every thread must be done with c-1 (the calling thread
                // is worker 0 and widens its share of chunk c only after issuing the copy)
                if (c >= 1) while (done[c - 1].load(std::memory_order_acquire) < T) std::this_thread::yield();
                issue(c + 1);
            }
            {   // worker 0's share of chunk c
                const size_t lo = c * chunk, cnt = std::min(chunk, N - lo);
                const size_t b = cnt / (size_t)T;
                const unsigned char *src = E.h_mapstage.p + (c & 1) * chunk * (size_t)me;
                given_elems_out(src, me, out + lo, 8, 0, b);
                done[c].fetch_add(1, std::memory_order_release);
            }
        }
    } catch (...) {
        failed.store(true);
        for (auto &th : pool) th.join();
        throw;
    }
    for (auto &th : pool) th.join();
}

// A host image up into E.src (f64: planar, or (N,3) row-major when `rows`) or E.src8 (interleaved 8-bit pixels of 3 or 4 channels), which
// the caller has reserved as it has E.cvt (with the weights' plane if the call has weights: run_device must not move what is converted
// here) and E.cstats -- ws_prepare; `host` describes it as Pixels describes a device image.  Nothing is waited for.
// Large images go up in pieces and what a piece completes is converted (on a second stream) while the next one is on the link:
// the conversion (0.5 ms of a 4096^2 image's 7 ms upload) disappears behind the copy.  Its statistics are exact sums and keyed
// extrema, so the chunking changes no bit.  With derived weights too: the saliency stage reads the sRGB source, which stays where it is.
// Returns the image as it now lies on the device, `converted` set where E.cvt / E.cstats hold the converted image.
static Pixels upload_image(Engine &E, const Pixels &host, size_t N, const patolette__QuantizationOptions *opt) {
    hipStream_t s = E.stream;
    Pixels dev = host;
    if (host.u8) dev.u8 = E.src8.p; else dev.f64 = E.src.p;
    unsigned char *dst = host.u8 ? E.src8.p : (unsigned char *)E.src.p;
    const unsigned char *from = host.u8 ? host.u8 : (const unsigned char *)host.f64;
    const size_t px_bytes = host.u8 ? (size_t)host.channels : 3 * sizeof(double);
    const size_t chunk_min = getenv("PAMD_UPLOAD_CHUNK_MIN") ? (size_t)atoll(getenv("PAMD_UPLOAD_CHUNK_MIN")) : ((size_t)1 << 21);   // (read per call: tests lower it)
    if (!(N >= chunk_min && !E.shard)) {
        HIP_CHECK(hipMemcpyAsync(dst, from, N * px_bytes, hipMemcpyHostToDevice, s));
        return dev;
    }
    if (!E.stream2) {
        HIP_CHECK(hipStreamCreateWithFlags(&E.stream2, hipStreamNonBlocking));
        for (hipEvent_t *e : {&E.ev_up[0], &E.ev_up[1], &E.ev_join}) HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    const ConvertPlan cp = convert_plan(E, opt, N);
    HIP_CHECK(hipEventRecord(E.ev_join, s));                     // whatever the engine's stream still holds comes first
    HIP_CHECK(hipStreamWaitEvent(E.stream2, E.ev_join, 0));
    // planar source: the first two planes go up whole (every copy call has a fixed cost: 24 pieces made the upload 0.44 ms
    // longer than one), the third in four pieces with the conversion of the pixels it completes behind each; row-major
    // and 8-bit sources: four pieces of whole pixels
    const bool planar = host.f64 && !host.rows;
    const size_t head = planar ? 2 * N * sizeof(double) : 0, step = planar ? sizeof(double) : px_bytes;   // bytes ahead of the pieces; per pixel of a piece
    if (planar) HIP_CHECK(hipMemcpyAsync(dst, from, head, hipMemcpyHostToDevice, s));
    const size_t nch = 4, per = ((N + nch - 1) / nch + 255) & ~(size_t)255;
    size_t c = 0;
    for (size_t lo = 0; lo < N; lo += per, c++) {
        const size_t cnt = std::min(per, N - lo);
        HIP_CHECK(hipMemcpyAsync(dst + head + lo * step, from + head + lo * step, cnt * step, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipEventRecord(E.ev_up[c & 1], s));
        HIP_CHECK(hipStreamWaitEvent(E.stream2, E.ev_up[c & 1], 0));
        convert_pixels(E, cp, dev, N, E.stream2, lo, lo + cnt, c == 0);
    }
    HIP_CHECK(hipEventRecord(E.ev_join, E.stream2));
    HIP_CHECK(hipStreamWaitEvent(s, E.ev_join, 0));
    // A stream whose LAST operation is a wait on an event keeps answering hipErrorNotReady to hipStreamQuery, even after
    // hipStreamSynchronize on it has returned; a record behind the wait makes the stream's state readable again (the late-growth
    // count of patolette_amd_debug_workspace asks exactly that question).  Both pieces' waits on ev_up[0] are enqueued by now.
    HIP_CHECK(hipEventRecord(E.ev_up[0], s));
    dev.converted = true;
    return dev;
}

// The front half of the quantising drivers (run_host, run_u8, run_rgba): what run_device takes -- the image on the device and its
// weights there (given, derived, or null) -- and the time from t_start until the upload's wait was over.
// src: frames x width x height pixels as the caller gives them, host memory unless `on_device`; `weights` likewise.  stage: the
// pixels go into the workspace -- a host image always (upload_image); a device image where the kernels cannot read it in place
// (run_rgba's unaligned pixels).  The caller has reserved what its output half takes and has enqueued nothing: this reserves the rest,
// uploads, waits for what came from the host, and derives the weights the binding derives when tile_size > 0 (each frame as an image
// of its own).  counted (run_rgba's opaque count): enqueued behind the upload; it waits for the stream itself -- one wait for the
// upload and its own download -- and says whether anything is left to quantise: only then are weights derived.
struct QuantInput { Pixels px; const double *d_w; double ms_upload; };
static QuantInput quant_input(Engine &E, double t_start, const Pixels &src, bool on_device, bool stage, size_t frames, size_t width, size_t height,
                              const double *weights, double tile_size, size_t K, const patolette__QuantizationOptions *opt,
                              const std::function<bool(const unsigned char *)> &counted = nullptr) {
    const size_t N = frames * width * height;
    const bool derive = !weights && tile_size > 0.0, weighted = weights || derive;
    if (stage) { if (src.u8) E.src8.reserve(N * (size_t)src.channels); else E.src.reserve(3 * N); }
    if (weights && !on_device) E.wsrc.reserve(N);
    if (derive) { E.wsal.reserve(N); saliency_reserve(E.sal, width, height); }
    ws_prepare(E, N, K, weighted, opt->verbose);   // (the workspace as run_device will want it: nothing is queued yet)
    QuantInput in{src, weights, 0.0};
    if (!on_device) in.px = upload_image(E, src, N, opt);
    else if (stage) {
        HIP_CHECK(hipMemcpyAsync(E.src8.p, src.u8, N * (size_t)src.channels, hipMemcpyDeviceToDevice, E.stream));
        in.px.u8 = E.src8.p;
    }
    if (weights && !on_device) {
        HIP_CHECK(hipMemcpyAsync(E.wsrc.p, weights, N * sizeof(double), hipMemcpyHostToDevice, E.stream));
        in.d_w = E.wsrc.p;
    }
    bool any = true;
    if (counted) any = counted(in.px.u8);
    else if (!on_device) HIP_CHECK(hipStreamSynchronize(E.stream));
    in.ms_upload = now_ms() - t_start;
    E.ms_saliency = 0.0;
    if (derive && any) in.d_w = derive_weights(E, in.px.f64, in.px.u8, in.px.rows ? -3 : in.px.channels, width, height, tile_size, frames);
    return in;
}
// ... and their epilogue, behind the output half that began at t_out: run_device has written its own stages' times and their total
static void quant_stats(Engine &E, const QuantInput &in, double t_out) {
    E.stats.ms_saliency = E.ms_saliency;
    E.stats.ms_upload = in.ms_upload;
    E.stats.ms_download = now_ms() - t_out;
    E.stats.ms_total += E.ms_saliency + in.ms_upload + E.stats.ms_download;
}

// host-buffer entry: upload, run, download + widen
static void run_host(Engine &E, size_t width, size_t height, const double *data, const double *weights, double tile_size,
                     size_t K, const patolette__QuantizationOptions *opt, double *palette, size_t *palette_map, bool rows = false,
                     void *d_map_out = nullptr) {
    // d_map_out: leave the narrow index map (u8 for K <= 256, else u32) in HBM there instead of widening it into palette_map
    const size_t N = width * height;
    const double t_start = now_ms();
    WsGuard wg(&E.stream, &E.stream2);
    const int me = map_elem_for(K);
    if (!opt->palette_only && !d_map_out) E.dmap.reserve(N * (size_t)me);
    const QuantInput in = quant_input(E, t_start, Pixels{data, nullptr, 3, rows}, false, true, 1, width, height, weights, tile_size, K, opt);
    std::vector<double> pal(3 * K);
    run_device(E, width, height, in.px, in.d_w, K, opt, pal.data(), d_map_out ? d_map_out : (void *)E.dmap.p, me);
    const double t_out = now_ms();
    if (!opt->palette_only && !d_map_out && map_touched(opt->dither, width, height)) download_map_widened(E, E.dmap.p, me, N, palette_map);
    std::memcpy(palette, pal.data(), 3 * K * sizeof(double));
    quant_stats(E, in, t_out);
}

// the device's index map (elements of me: 1 or 4 bytes) into a host buffer with elements of map_elem_out (1, 2, 4 or 8)
static void download_map(const void *d_map, int me, size_t N, void *map_out, int map_elem_out) {
    if (map_elem_out == me) { HIP_CHECK(hipMemcpy(map_out, d_map, N * (size_t)me, hipMemcpyDeviceToHost)); return; }
    std::vector<unsigned char> tmp(N * (size_t)me);
    HIP_CHECK(hipMemcpy(tmp.data(), d_map, tmp.size(), hipMemcpyDeviceToHost));
    given_elems_out(tmp.data(), me, map_out, map_elem_out, 0, N);
}

static HipError named_error(const char *name, const char *text) { return HipError(std::string(name) + ": " + text); }
static const char *const kBadDeviceMapElem = "patolette_amd: device map_elem_bytes must be 1 for K <= 256, else 4";

// Where the 8-bit entries' index map (elements of map_elem_for(K8) bytes) lands: in the caller's buffer when that is device memory, else
// in E.dmap; null when no map-derived output is wanted (the map kernels are then skipped).  Reserves that place and what u8_outputs
// takes of the workspace: the caller does this before it enqueues anything.
static void *u8_map_place(Engine &E, size_t N, size_t K8, bool want, void *map_out, int map_elem_out, bool map_on_device,
                          const unsigned char *quant_out, bool quant_on_device) {
    if (!want) return nullptr;
    if (quant_out) { E.pal8.reserve(3 * K8); if (!quant_on_device) E.quant8.reserve(3 * N); }
    if (map_out && map_on_device) {
        if (map_elem_out != map_elem_for(K8)) throw HipError(kBadDeviceMapElem);
        return map_out;
    }
    E.dmap.reserve(N * (size_t)map_elem_for(K8));
    return E.dmap.p;
}

// The 8-bit entries' output stage, from the map at d_map (u8_map_place) and the K8 palette rows' bytes p8: quantized = p8[map] made on the
// device and copied out unless `on_device`; the map downloaded, and widened or narrowed to map_elem_out, where it is not in place already
static void u8_outputs(Engine &E, const void *d_map, size_t N, const unsigned char *p8, size_t K8, void *map_out, int map_elem_out,
                       unsigned char *quant_out, bool on_device) {
    hipStream_t s = E.stream;
    const int me = map_elem_for(K8);
    if (quant_out) {
        HIP_CHECK(hipMemcpyAsync(E.pal8.p, p8, 3 * K8, hipMemcpyHostToDevice, s));
        unsigned char *d_q = on_device ? quant_out : E.quant8.p;
        launch_reconstruct(d_map, me, N, E.pal8.p, (int)K8, d_q, s);
        if (!on_device) HIP_CHECK(hipMemcpyAsync(quant_out, d_q, 3 * N, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    if (map_out && d_map != map_out) download_map(d_map, me, N, map_out, map_elem_out);
    E.sync();
}

// The RGBA entries' counterpart (run_rgba, run_remap_rgba): where the kernel that writes the caller's map elements and RGBA words puts
// them -- the caller's buffers when those are device memory, else E.rgba_map and E.quant8 -- and whether the N pixels must be staged.
// Checks what the kernels ask of device buffers (`entry`: the caller's C entry, for the message) and reserves these places, with
// E.src8 for staged pixels: the caller has enqueued nothing yet.  want: a map-derived output is made at all.
struct RgbaOut { bool stage_px; void *d_map; unsigned char *d_q; };
static RgbaOut rgba_out_place(Engine &E, const char *entry, size_t N, bool on_device, const unsigned char *pixels, bool want, void *map_out,
                              int map_elem_out, unsigned char *quant_out) {
    auto aligned = [](const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
    if (on_device && ((map_out && !aligned(map_out, (size_t)map_elem_out)) || (quant_out && !aligned(quant_out, 4))))
        throw named_error(entry, "palette_map and quantized must be aligned to their element size");
    RgbaOut o{!on_device || !aligned(pixels, 4), nullptr, nullptr};   // the kernels read one 32-bit word per pixel
    if (o.stage_px) E.src8.reserve(4 * N);
    if (want && !on_device && map_out) E.rgba_map.reserve(N * (size_t)map_elem_out);
    if (want && !on_device && quant_out) E.quant8.reserve(4 * N);
    if (want && map_out) o.d_map = on_device ? map_out : (void *)E.rgba_map.p;
    if (want && quant_out) o.d_q = on_device ? quant_out : E.quant8.p;
    return o;
}
// ... and from there into the caller's buffers where those are host memory, behind one wait for everything the call has enqueued
static void rgba_copy_out(Engine &E, const RgbaOut &o, size_t N, void *map_out, int map_elem_out, unsigned char *quant_out) {
    if (o.d_map && o.d_map != map_out) HIP_CHECK(hipMemcpyAsync(map_out, o.d_map, N * (size_t)map_elem_out, hipMemcpyDeviceToHost, E.stream));
    if (o.d_q && o.d_q != quant_out) HIP_CHECK(hipMemcpyAsync(quant_out, o.d_q, 4 * N, hipMemcpyDeviceToHost, E.stream));
    E.sync();
}

// 8-bit adaptor around the path: interleaved u8 in; f64 palette, u8 palette, index map and
// reconstructed u8 image out.  `pixels`, `d_map_out`, `d_quant_out` are device pointers when `on_device`.
static void run_u8(Engine &E, size_t width, size_t height, const unsigned char *pixels, int channels, const double *weights,
                   double tile_size, size_t K, const patolette__QuantizationOptions *opt, double *palette, unsigned char *palette_u8,
                   void *map_out, int map_elem_out, unsigned char *quant_out, bool on_device, bool map_on_device = false,
                   const Frames *frames = nullptr) {
    // frames: the image is that stack (width x height = frames->width x frames->count * frames->height); weights, upload, map
    // download and reconstruction serve it as they serve one image
    const size_t N = width * height;
    const size_t fcount = frames ? frames->count : 1, fheight = frames ? frames->height : height;   // one image: a stack of one
    const double t_start = now_ms();
    WsGuard wg(&E.stream, &E.stream2);
    // what the output stage takes of the workspace, before anything is enqueued (its own reservations are then no-ops)
    void *d_map = u8_map_place(E, N, K, !opt->palette_only && (map_out || quant_out), map_out, map_elem_out, on_device || map_on_device,
                               quant_out, on_device);
    const QuantInput in = quant_input(E, t_start, Pixels{nullptr, pixels, channels}, on_device, !on_device, fcount, width, fheight, weights,
                                      tile_size, K, opt);
    std::vector<double> pal(3 * K);
    run_device(E, width, height, in.px, in.d_w, K, opt, pal.data(), d_map, map_elem_for(K), nullptr, frames);
    const double t_out = now_ms();
    std::vector<unsigned char> p8(3 * K);
    palette_to_u8(pal.data(), K, p8.data());
    if (palette) std::memcpy(palette, pal.data(), 3 * K * sizeof(double));
    if (palette_u8) std::memcpy(palette_u8, p8.data(), 3 * K);
    if (d_map && map_touched(opt->dither, width, fheight)) u8_outputs(E, d_map, N, p8.data(), K, map_out, map_elem_out, quant_out, on_device);
    quant_stats(E, in, t_out);
}

// The frame around a run over pixels or maps the caller gives (the remaps, frame deltas, measure, gif_lzw): construction takes the
// start time, points the workspace at the engine's streams and resets the statistics; lap() writes the named lap (the time since the
// lap before it, or the start); done() the total.  Nothing happens on the way out: a run that throws leaves E.stats as far as it got.
struct GivenRun {
    Engine &E;
    const double t_start;
    double t_lap;
    WsGuard wg;
    explicit GivenRun(Engine &e) : E(e), t_start(now_ms()), t_lap(t_start), wg(&e.stream, &e.stream2) { E.stats = patolette_amd__Stats{}; }
    void lap(double patolette_amd__Stats::*field) { const double t = now_ms(); E.stats.*field = t - t_lap; t_lap = t; }
    void done() { E.stats.ms_total = now_ms() - t_start; }
    // `count` words the kernels left at d, on the host once everything enqueued has run
    std::vector<unsigned long long> words(const unsigned long long *d, size_t count) {
        std::vector<unsigned long long> w(count);
        HIP_CHECK(hipMemcpyAsync(w.data(), d, count * sizeof(unsigned long long), hipMemcpyDeviceToHost, E.stream));
        E.sync();
        return w;
    }
};

// --------------------------------------------------------------------------------------------
// remap: 8-bit pixels onto a palette the caller gives (include/patolette_amd.h, patolette_amd_remap_u8)
// --------------------------------------------------------------------------------------------
// TESTS ONLY (patolette_amd_debug_remap_two_pass): every remap converts the image into f64 planes first
static std::atomic<int> g_remap_two_pass{0};

// pal: the palette's k rows, planar (k,3) f64 sRGB; p8: the bytes `quantized` is made of, me-indexed rows (K8 >= k of them: the palette as
// given, dropped rows included).  `pixels`, `map_out`, `quant_out` are device pointers when `on_device`.
// Nearest, two-pass: pixels -> ICtCp planes (k_convert_u8, whose statistics bound the grid) -> launch_nn_map.  Nearest, fused (where the
// LDS-table kernel runs): launch_nn_map_u8 converts in registers.  Dither, two-pass: pixels -> linear
// Rec2020 planes -> launch_dither.  Dither, fused (where the lane layout runs): launch_dither with the job's bytes gathers the
// bytes along the curve and converts them there; no f64 image is written.
// Ordered (mode kRemapOrdered, `spread`): launch_ordered_map shifts, converts and searches in one kernel; palette in ICtCp, no f64 image.
enum { kRemapNearest = 0, kRemapRiemersma = 1, kRemapOrdered = 2 };
// The remaps' 8-bit pixels into E.src8 (reserved), from the host or -- `on_device` -- from where the kernels cannot read them; waited for
static const unsigned char *remap_stage_pixels(Engine &E, const unsigned char *pixels, size_t bytes, bool on_device) {
    HIP_CHECK(hipMemcpyAsync(E.src8.p, pixels, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, E.stream));
    HIP_CHECK(hipStreamSynchronize(E.stream));
    return E.src8.p;
}
// The remaps' Riemersma walk over `frames` frames of 8-bit pixels (N in all) with the Rec2020 palette in E.dpal and in `pal`: fused, or
// through the planes in E.cvt, which the caller has reserved (3 * N) unless `fused`
static void remap_dither(Engine &E, const unsigned char *d_px, int channels, size_t frames, size_t width, size_t height, const std::vector<double> &pal,
                         size_t k, void *d_map, int me, bool fused, bool lanes) {
    const size_t N = frames * width * height;
    hipStream_t s = E.stream;
    DitherJob job;
    job.frames = frames; job.width = width; job.height = height;
    job.d_pal = E.dpal.p; job.h_pal = pal.data(); job.k = (int)k;
    job.out = d_map; job.elem_bytes = me;
    bool done = false;
    if (fused) {
        HIP_CHECK(hipStreamSynchronize(s));
        job.bytes = d_px; job.channels = channels;
        done = launch_dither(job, E.nn, s);
        // the lane walk's verification stalled beyond patolette_amd_debug_dither_solo_cap: the planes after all, for the wavefront layout
        if (!done) { HIP_CHECK(hipStreamSynchronize(s)); E.cvt.reserve(3 * N); }
    }
    if (!done) {
        launch_convert_u8(PAMD_SRGB_TO_REC2020, d_px, channels, E.cvt.p, N, nullptr, s);
        HIP_CHECK(hipStreamSynchronize(s));
        job.bytes = nullptr;
        job.planes = E.cvt.p; job.plane_stride = N; job.which = PAMD_COPY;
        job.layout = (lanes && !fused) ? 1 : 0;                               // (after a stalled lane walk: not the same walk again)
        launch_dither(job, E.nn, s);
    }
}

// Which way a remap of N pixels onto k rows goes.  walk_frames: the frames a Riemersma walk takes together (run_remap: all of them,
// hence the frames' layout rule; run_remap_rgba walks frame by frame: 1).  lanes: the walk's lane layout runs; fused: no f64 image is
// written -- otherwise the caller reserves remap_planes, what such a route takes of the workspace besides the palette and the map.
struct RemapRoute { bool lanes, fused; };
static RemapRoute remap_route(int mode, size_t walk_frames, size_t width, size_t height, size_t N, size_t k) {
    const bool dither = mode == kRemapRiemersma;
    const bool lanes = dither && (walk_frames > 1 ? dither_frames_lane_layout(walk_frames, width, height, (int)k) : dither_lane_layout(width, height, (int)k));
    return {lanes, mode == kRemapOrdered || (!g_remap_two_pass.load(std::memory_order_relaxed) && (dither ? lanes : nn_map_u8_applies(N, (int)k)))};
}
static void remap_planes(Engine &E, size_t N) { E.cvt.reserve(3 * N); E.cstats.reserve(1); E.h_cstats.reserve(1); }

// The remaps' maps without a walk, over `frames` frames of 8-bit pixels (N in all) with the ICtCp palette's k rows on their way into
// E.dpal: ordered; nearest, fused; or nearest through the planes in E.cvt (remap_planes)
static void remap_flat(Engine &E, const unsigned char *d_px, int channels, size_t frames, size_t width, size_t height, bool ordered, double spread,
                       bool fused, size_t k, void *d_map, int me) {
    const size_t N = frames * width * height;
    hipStream_t s = E.stream;
    if (ordered) {
        launch_ordered_map(d_px, channels, frames, width, height, spread, E.dpal.p, (int)k, d_map, me, s);
    } else if (fused) {
        HIP_CHECK(hipStreamSynchronize(s));                                       // (the map kernels' tables are reserved on an idle stream)
        launch_nn_map_u8(d_px, channels, N, E.dpal.p, (int)k, d_map, me, E.nn, s);
    } else {
        launch_convert_u8(PAMD_SRGB_TO_ICTCP, d_px, channels, E.cvt.p, N, E.cstats.p, s);
        const Bounds b = read_bounds(E, false);                                   // (waits: the map kernels' tables are reserved on an idle stream)
        launch_nn_map(E.cvt.p, N, N, E.dpal.p, (int)k, d_map, me, b.lo, b.hi, E.nn, s);
    }
}

static void run_remap(Engine &E, size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels, std::vector<double> pal,
                      size_t k, const std::vector<unsigned char> &p8, size_t K8, int mode, double spread, void *map_out, int map_elem_out,
                      unsigned char *quant_out, bool on_device) {
    const bool dither = mode == kRemapRiemersma;
    const size_t N = frames * width * height;
    GivenRun run(E);
    const int me = map_elem_for(K8);
    const RemapRoute route = remap_route(mode, frames, width, height, N, k);
    // the workspace, before anything is enqueued
    if (!on_device) E.src8.reserve(N * (size_t)channels);
    E.dpal.reserve(3 * k); E.h_pal.reserve(3 * k);
    void *d_map = u8_map_place(E, N, K8, map_out || quant_out, map_out, map_elem_out, on_device, quant_out, on_device);
    const bool want = d_map != nullptr;
    if (want && !route.fused) remap_planes(E, N);
    const unsigned char *d_px = on_device ? pixels : remap_stage_pixels(E, pixels, N * (size_t)channels, false);
    run.lap(&patolette_amd__Stats::ms_upload);
    // the palette into the space its map compares in (patolette.c:268-299 for colour space sRGB, resp. :300-324)
    palette_rows(pal, k, dither ? hm::color::srgb_to_rec2020 : hm::color::srgb_to_ictcp);
    E.map_palette = pal;
    if (want) {
        upload_palette(E, pal, k);
        if (!dither) remap_flat(E, d_px, channels, frames, width, height, mode == kRemapOrdered, spread, route.fused, k, d_map, me);
        else {
            remap_dither(E, d_px, channels, frames, width, height, pal, k, d_map, me, route.fused, route.lanes);
            add_dither_stats(E);
        }
        E.sync();
    }
    run.lap(&patolette_amd__Stats::ms_map);
    if (want && map_touched(dither, width, height)) u8_outputs(E, d_map, N, p8.data(), K8, map_out, map_elem_out, quant_out, on_device);
    run.lap(&patolette_amd__Stats::ms_download);
    run.done();
}

// --------------------------------------------------------------------------------------------
// remap with alpha: RGBA frames onto a palette the caller gives (include/patolette_amd.h, patolette_amd_remap_rgba_u8)
// --------------------------------------------------------------------------------------------
// The map half of the RGBA entry for one width x height frame of which M pixels (0 < M < n) are opaque, from 8-bit pixels and a GIVEN
// palette: compaction (with the offsets launch_alpha_count left at d_offsets), the opaque pixels' bytes into linear Rec2020 planes,
// the masked walk over the frame's curve, and the expansion into the caller's elements and RGBA words.  pal: the k opaque rows in
// linear Rec2020 (also in E.dpal); d_palw: rows RGBA words.  The caller has reserved E.rgba_cpos (n), E.rgba_rgb (3 n), E.cvt (3 n),
// E.dmap (n elements of me bytes) and the masked dither's tables.  (run_rgba's own map stage stays inside run_device: it walks the
// pipeline's working image, ICtCp -> Rec2020, and another conversion route would change its bits.)
static void rgba_masked_frame(Engine &E, const unsigned char *d_px, size_t width, size_t height, int thr, size_t M, const unsigned *d_offsets,
                              const std::vector<double> &pal, size_t k, unsigned off, const unsigned char *d_palw, size_t rows, int me, void *d_map,
                              int map_elem, unsigned char *d_quant) {
    const size_t n = width * height;
    hipStream_t s = E.stream;
    launch_alpha_compact(d_px, n, M, thr, d_offsets, nullptr, E.rgba_cpos.p, E.rgba_rgb.p, nullptr, s);
    launch_convert_u8(PAMD_SRGB_TO_REC2020, E.rgba_rgb.p, 3, E.cvt.p, M, nullptr, s);
    HIP_CHECK(hipStreamSynchronize(s));                               // (the dither launchers size their workspace before they enqueue)
    DitherJob job;
    job.planes = E.cvt.p; job.plane_stride = M; job.which = PAMD_COPY;
    job.width = width; job.height = height; job.cpos = E.rgba_cpos.p; job.opaque = M;
    job.d_pal = E.dpal.p; job.h_pal = pal.data(); job.k = (int)k;
    job.out = E.dmap.p; job.elem_bytes = me;
    launch_dither(job, E.nn, s);
    launch_rgba_expand(E.dmap.p, me, E.rgba_cpos.p, n, M, off, d_palw, (int)rows, d_map, map_elem, d_quant, s);
}

// pal: the k OPAQUE rows, planar (k,3) f64 sRGB; palw: one RGBA word per row of the palette as the maps number it (off + k rows: row 0
// the transparent entry's (0, 0, 0, 0) when off == 1; the others (pal8, 255)).
// `pixels`, `map_out`, `quant_out` are device pointers when `on_device`.
// Nearest and ordered: run_remap's mappers over all N pixels with channels = 4 and the opaque rows, into E.dmap; then k_rgba_stamp, one
// launch, writes the caller's elements and the RGBA words and raises the flag.  Riemersma: frame after frame -- every frame's opaque
// count first (one wait for all of them), then per frame nothing (M == 0), run_remap's walk (M == n) or rgba_masked_frame.
static void run_remap_rgba(Engine &E, size_t frames, size_t width, size_t height, const unsigned char *pixels, int thr, std::vector<double> pal, size_t k,
                           const std::vector<unsigned> &palw, unsigned off, int mode, double spread, void *map_out, int map_elem_out,
                           unsigned char *quant_out, bool on_device) {
    const bool dither = mode == kRemapRiemersma;
    const size_t n = width * height, N = frames * n, rows = off + k;
    hipStream_t s = E.stream;
    GivenRun run(E);
    const int me = map_elem_for(k);                                   // the mappers' elements: choices among the opaque rows
    const bool want = map_out || quant_out;
    const RemapRoute route = remap_route(mode, 1, width, height, N, k);
    const size_t tiles = compact_tiles(n);
    // the workspace, before anything is enqueued
    const RgbaOut out = rgba_out_place(E, "patolette_amd_remap_rgba_device", N, on_device, pixels, want, map_out, map_elem_out, quant_out);
    E.dpal.reserve(3 * k); E.h_pal.reserve(3 * k);
    E.pal8.reserve(4 * rows);
    E.rr_words.reserve(1 + frames); E.h_rr_words.reserve(1 + frames);
    if (want) {
        E.dmap.reserve((dither ? n : N) * (size_t)me);
        if (dither) { E.cvt.reserve(3 * n); E.rgba_cpos.reserve(n); E.rgba_rgb.reserve(3 * n); dither_mask_reserve(E.nn, n); }
        else if (!route.fused) remap_planes(E, N);
    }
    if (dither) E.rgba_cnt.reserve(frames * tiles);
    const unsigned char *d_px = out.stage_px ? remap_stage_pixels(E, pixels, 4 * N, on_device) : pixels;
    run.lap(&patolette_amd__Stats::ms_upload);
    palette_rows(pal, k, dither ? hm::color::srgb_to_rec2020 : hm::color::srgb_to_ictcp);   // as run_remap takes its palette
    E.map_palette = pal;
    unsigned *d_flag = E.rr_words.p, *h_words = E.h_rr_words.p;
    HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(unsigned), s));
    HIP_CHECK(hipMemcpyAsync(E.pal8.p, palw.data(), 4 * rows, hipMemcpyHostToDevice, s));
    const char *const kNoEntry = "patolette_amd_remap_rgba: a pixel is transparent (alpha < alpha_threshold) and the palette has no transparent entry "
                                 "(transparent_index -1)";
    if (!dither) {
        if (want) {
            upload_palette(E, pal, k);
            remap_flat(E, d_px, 4, frames, width, height, mode == kRemapOrdered, spread, route.fused, k, E.dmap.p, me);
        }
        launch_rgba_stamp(d_px, want ? E.dmap.p : nullptr, me, N, thr, off, E.pal8.p, rows, out.d_map, map_elem_out, out.d_q, d_flag, s);
        HIP_CHECK(hipMemcpyAsync(h_words, d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    } else {
        for (size_t f = 0; f < frames; f++)
            launch_alpha_count(d_px + 4 * n * f, n, thr, E.rgba_cnt.p + f * tiles, E.rr_words.p + 1 + f, s);
        HIP_CHECK(hipMemcpyAsync(h_words, E.rr_words.p, (1 + frames) * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));                           // every frame's opaque count, with one wait
        if (off == 0) for (size_t f = 0; f < frames; f++) if (h_words[1 + f] < n) throw HipError(kNoEntry);
        if (want) {
            upload_palette(E, pal, k);
            const size_t mb = (size_t)map_elem_out;
            for (size_t f = 0; f < frames; f++) {
                const size_t M = h_words[1 + f];
                const unsigned char *px_f = d_px + 4 * n * f;
                void *map_f = out.d_map ? (void *)((unsigned char *)out.d_map + n * f * mb) : nullptr;
                unsigned char *q_f = out.d_q ? out.d_q + 4 * n * f : nullptr;
                if (M == 0) {                                          // nothing to walk: element 0 and (0, 0, 0, 0) throughout
                    if (map_f) HIP_CHECK(hipMemsetAsync(map_f, 0, n * mb, s));
                    if (q_f) HIP_CHECK(hipMemsetAsync(q_f, 0, 4 * n, s));
                } else if (M == n) {                                   // no transparent pixel: the plain walk of run_remap
                    if (map_touched(true, width, height)) remap_dither(E, px_f, 4, 1, width, height, pal, k, E.dmap.p, me, route.fused, route.lanes);
                    else HIP_CHECK(hipMemsetAsync(E.dmap.p, 0, n * (size_t)me, s));       // (a 1x1 dither writes nothing: entry 0)
                    launch_rgba_expand(E.dmap.p, me, nullptr, n, n, off, E.pal8.p, (int)rows, map_f, map_elem_out, q_f, s);
                } else {
                    rgba_masked_frame(E, px_f, width, height, thr, M, E.rgba_cnt.p + f * tiles, pal, k, off, E.pal8.p, rows, me, map_f, map_elem_out,
                                      q_f);
                }
                if (M > 0 && map_touched(true, width, height)) add_dither_stats(E);   // the walks' counters, summed over the frames
            }
        }
        h_words[0] = 0;
    }
    E.sync();                                                         // (palw is the caller's local: the copy must have left the host)
    run.lap(&patolette_amd__Stats::ms_map);
    if (h_words[0] & 1) throw HipError(kNoEntry);
    rgba_copy_out(E, out, N, map_out, map_elem_out, quant_out);
    run.lap(&patolette_amd__Stats::ms_download);
    run.done();
}

// --------------------------------------------------------------------------------------------
// frame deltas: an animation's index maps with "as on screen" made transparent (include/patolette_amd.h, patolette_amd_frame_deltas)
// --------------------------------------------------------------------------------------------
// Host maps of N elements (eb bytes each; given.h: the 2- and 8-byte ones as the device's 4) up into E.dl_maps and, where `pixels` is
// given, the 8-bit pixels into E.src8.  Reserves both: the caller has enqueued nothing yet.  Waits for the copies.
// stage: the caller's, for the 2- and 8-byte host elements widened or narrowed (its pages are the caller's to use again, and to free
// outside what it times)
static void stage_given(Engine &E, const void *maps, int eb, int me, size_t N, GivenSkip skip, unsigned long long skip_index,
                        const unsigned char *pixels, int channels, std::vector<unsigned> &stage) {
    hipStream_t s = E.stream;
    E.dl_maps.reserve(N * (size_t)me);
    if (pixels) E.src8.reserve(N * (size_t)channels);
    if (eb != me) { stage.resize(N); given_elems_in(maps, eb, N, skip, skip_index, stage.data()); maps = stage.data(); }
    HIP_CHECK(hipMemcpyAsync(E.dl_maps.p, maps, N * (size_t)me, hipMemcpyHostToDevice, s));
    if (pixels) HIP_CHECK(hipMemcpyAsync(E.src8.p, pixels, N * (size_t)channels, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// The flavours of the frame deltas: plain maps (patolette_amd_frame_deltas), maps whose index 0 is the transparent entry
// (patolette_amd_frame_deltas_rgba), and plain maps with a colour table per frame (patolette_amd_frame_deltas_local).  delta.h lays
// out the words the kernels leave.
struct DeltaFlavour {
    const char *bad_element;       // what a raised flag says
    bool v_boxes;                  // per frame a second box, V (what vanishes in the next frame): 5 words a slot instead of 3, and a disposal
    bool first_full;               // frame 0 is the full first map whatever the kernels counted
    bool free_index;               // the caller's transparent index T, an index no entry uses, travels as given_transparent_on_device(T)
};
// Per-frame palettes: P tables of K rows as bytes, and the table of every frame (checked: each below P).  `shown` is then colours,
// 3 bytes a position, and a lossy run's `pal` holds all P K rows.
struct DeltaTables { size_t P, K; std::vector<unsigned char> p8; std::vector<int32_t> of; };
static const DeltaFlavour kPlainDeltas{"patolette_amd_frame_deltas: a map element is not below palette_rows, or names a dropped trailing (-1, -1, -1) row",
                                       false, true, true};
static const DeltaFlavour kRgbaDeltas{"patolette_amd_frame_deltas_rgba: a map element is not below palette_rows, or names a dropped trailing (-1, -1, -1) row",
                                      true, false, false};
static const DeltaFlavour kLocalDeltas{"patolette_amd_frame_deltas_local: a map element is not below palette_rows", false, true, true};

// maps: frames x width x height elements of `eb` bytes; rows: what every element must stay below (lossy: the used rows of pal, planar
// (rows,3) f64 sRGB; otherwise pal is empty and neither it nor the pixels are read).  T (plain maps) and loop (RGBA maps): the
// flavour's own argument.  `maps`, `pixels`, `delta_out`, `shown_out` are device pointers when `on_device`; rects, disposals (RGBA maps)
// and changed are host memory.  Every output may be null; delta_out may be maps.  tables: the per-frame palettes, or null.
static void run_frame_deltas(Engine &E, const DeltaFlavour &fl, bool on_device, size_t frames, size_t width, size_t height, const void *maps, int eb,
                             size_t rows, size_t T, int loop, const unsigned char *pixels, int channels, std::vector<double> pal, double tolerance,
                             void *delta_out, void *shown_out, int32_t *rects, int32_t *disposals, uint64_t *changed,
                             const DeltaTables *tables = nullptr) {
    const bool lossy = tolerance > 0.0;
    const size_t n = width * height, N = frames * n, cells = frames * (size_t)kDeltaSlots;
    const size_t pal_rows = tables ? tables->P * tables->K : rows, shown_bytes = N * (tables ? 3 : (size_t)given_device_elem(eb, on_device));
    hipStream_t s = E.stream;
    GivenRun run(E);
    const int me = given_device_elem(eb, on_device);
    const unsigned Td = given_transparent_on_device(T);
    // the workspace, before anything is enqueued
    const size_t words = fl.v_boxes ? frame_deltas_rgba_words(frames) : frame_deltas_words(frames);
    E.dl_words.reserve(words);
    if (!fl.v_boxes) E.dl_masks.reserve(frame_deltas_masks(frames, n));
    if (!on_device && shown_out) E.dl_shown.reserve(shown_bytes);
    else if (fl.v_boxes && !shown_out) E.dl_shown.reserve(n * (size_t)me);         // the canvas between the frames' launches
    if (lossy) { E.dpal.reserve(3 * pal_rows); E.h_pal.reserve(3 * pal_rows); }
    if (tables) E.dl_rows.reserve(pal_rows + frames);
    const void *d_maps = maps;
    void *d_delta = delta_out, *d_shown = shown_out;
    const unsigned char *d_px = pixels;
    std::vector<unsigned> stage;
    if (!on_device) {
        stage_given(E, maps, eb, me, N, GivenSkip{}, 0, lossy ? pixels : nullptr, channels, stage);
        if (lossy) d_px = E.src8.p;
        d_maps = E.dl_maps.p;
        d_delta = delta_out ? E.dl_maps.p : nullptr;                               // in place: the kernels allow it
        d_shown = shown_out ? E.dl_shown.p : nullptr;
    }
    run.lap(&patolette_amd__Stats::ms_upload);
    if (lossy) {
        palette_rows(pal, pal_rows, hm::color::srgb_to_ictcp);                     // as run_remap's nearest map takes its palette
        upload_palette(E, pal, pal_rows);
    }
    const double *d_pal = lossy ? E.dpal.p : nullptr;
    std::vector<unsigned> local;                                                   // (pageable: the copy has left the host when it returns)
    if (tables) {
        local = given_row_words(tables->p8, pal_rows);
        local.insert(local.end(), tables->of.begin(), tables->of.end());
        HIP_CHECK(hipMemcpyAsync(E.dl_rows.p, local.data(), local.size() * sizeof(unsigned), hipMemcpyHostToDevice, s));
        launch_frame_deltas_local((const unsigned char *)d_maps, frames, width, height, tables->K, tables->P, Td, lossy,
                                  reinterpret_cast<const int *>(E.dl_rows.p + pal_rows), E.dl_rows.p, d_px, channels, d_pal, tolerance * tolerance,
                                  (unsigned char *)d_delta, (unsigned char *)d_shown, E.dl_masks.p, E.dl_words.p, s);
    } else if (fl.v_boxes)
        launch_frame_deltas_rgba(d_maps, me, frames, width, height, rows, loop, lossy, d_px, channels, d_pal, tolerance * tolerance, d_delta, d_shown,
                                 d_shown ? nullptr : E.dl_shown.p, E.dl_words.p, s);
    else
        launch_frame_deltas(d_maps, me, frames, width, height, rows, Td, lossy, d_px, channels, d_pal, tolerance * tolerance, d_delta, d_shown,
                            E.dl_masks.p, E.dl_words.p, s);
    const std::vector<unsigned long long> w = run.words(E.dl_words.p, words);
    run.lap(&patolette_amd__Stats::ms_map);
    if (w[words - 1] & 1) throw HipError(fl.bad_element);
    const unsigned *box = reinterpret_cast<const unsigned *>(w.data());             // C boxes, V boxes where the flavour has them, then the counts
    const unsigned long long *cnt = w.data() + cells * (fl.v_boxes ? 4 : 2);
    for (size_t f = 0; f < frames; f++) {
        const size_t at = f * (size_t)kDeltaSlots;
        const GivenFrameFold r = given_fold_frame(box + 4 * at, fl.v_boxes ? box + 4 * (cells + at) : nullptr, cnt + at, kDeltaSlots, width, height,
                                                  fl.first_full && f == 0);
        if (changed) changed[f] = r.count;
        if (disposals) disposals[f] = r.vanish ? 2 : 1;
        if (rects) std::memcpy(rects + 4 * f, r.rect, sizeof r.rect);
    }
    if (!on_device) {
        void *outs[2] = {delta_out, shown_out};
        const void *from[2] = {d_delta, d_shown};
        for (int o = 0; o < 2; o++) {
            if (!outs[o]) continue;
            if (tables && o == 1) { HIP_CHECK(hipMemcpy(outs[o], from[o], shown_bytes, hipMemcpyDeviceToHost)); continue; }   // colours
            if (eb == me) { HIP_CHECK(hipMemcpy(outs[o], from[o], N * (size_t)me, hipMemcpyDeviceToHost)); continue; }
            HIP_CHECK(hipMemcpy(stage.data(), from[o], N * sizeof(unsigned), hipMemcpyDeviceToHost));   // (stage_given sized it; Td becomes T)
            given_elems_out(stage.data(), me, outs[o], eb, 0, N, fl.free_index, Td, T);
        }
    }
    run.lap(&patolette_amd__Stats::ms_download);
    run.done();
}

// --------------------------------------------------------------------------------------------
// measure: a map's error per palette entry and frame (include/patolette_amd.h, patolette_amd_measure)
// --------------------------------------------------------------------------------------------
struct MeasureOut {                                // host memory, each may be null
    uint64_t *entry_count, *entry_sse; uint32_t *entry_max_se;          // K8 each
    uint64_t *frame_count, *frame_sse; uint32_t *frame_max_se;          // frames each
    double *frame_d_sum, *frame_d_max;                                  // frames each
};

// maps: frames x width x height elements of `eb` bytes; pal: the k used rows, planar (k,3) f64 sRGB; p8: the bytes of the K8 rows as
// given.  skip < 0: none.  `maps` and `pixels` are device pointers when `on_device`; the outputs are host memory.
static void run_measure(Engine &E, bool on_device, size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels,
                        const void *maps, int eb, std::vector<double> pal, size_t k, const std::vector<unsigned char> &p8, size_t K8,
                        long long skip, const MeasureOut &out) {
    const size_t n = width * height, N = frames * n;
    hipStream_t s = E.stream;
    GivenRun run(E);
    const int me = given_device_elem(eb, on_device);
    const bool with_d = out.frame_d_sum || out.frame_d_max;
    const GivenSkip sk = given_skip_on_device(skip, eb, me, on_device);
    // the workspace, before anything is enqueued
    const size_t words = measure_words(frames, k), from = measure_flag_word(k);
    E.ms_words.reserve(words);
    E.ms_tiles.reserve(measure_tile_count(frames, n));
    E.ms_p8.reserve(k);
    if (with_d) { E.dpal.reserve(3 * k); E.h_pal.reserve(3 * k); }
    const void *d_maps = maps;
    const unsigned char *d_px = pixels;
    std::vector<unsigned> stage;
    if (!on_device) {
        stage_given(E, maps, eb, me, N, sk, (unsigned long long)skip, pixels, channels, stage);
        d_maps = E.dl_maps.p;
        d_px = E.src8.p;
    }
    run.lap(&patolette_amd__Stats::ms_upload);
    const std::vector<unsigned> rows8 = given_row_words(p8, k);
    HIP_CHECK(hipMemcpyAsync(E.ms_p8.p, rows8.data(), k * sizeof(unsigned), hipMemcpyHostToDevice, s));
    if (with_d) {
        palette_rows(pal, k, hm::color::srgb_to_ictcp);                            // as run_remap's nearest map takes its palette
        upload_palette(E, pal, k);
    }
    launch_measure(d_maps, me, frames, n, d_px, channels, k, sk.on, sk.Sd, E.ms_p8.p, with_d ? E.dpal.p : nullptr, E.ms_words.p, E.ms_tiles.p, s);
    const std::vector<unsigned long long> w = run.words(E.ms_words.p + from, words - from);
    run.lap(&patolette_amd__Stats::ms_map);
    if (w[0] & 1)
        throw HipError("patolette_amd_measure: a map element is neither skip_index nor below palette_rows, or names a dropped trailing (-1, -1, -1) row");
    const unsigned long long *er = w.data() + 1, *fr = er + 3 * k;
    for (size_t i = 0; i < K8; i++) {                                              // (dropped rows: nothing names them)
        if (out.entry_count) out.entry_count[i] = i < k ? er[3 * i] : 0;
        if (out.entry_sse) out.entry_sse[i] = i < k ? er[3 * i + 1] : 0;
        if (out.entry_max_se) out.entry_max_se[i] = i < k ? (uint32_t)er[3 * i + 2] : 0;
    }
    for (size_t f = 0; f < frames; f++) {
        if (out.frame_count) out.frame_count[f] = fr[5 * f];
        if (out.frame_sse) out.frame_sse[f] = fr[5 * f + 1];
        if (out.frame_max_se) out.frame_max_se[f] = (uint32_t)fr[5 * f + 2];
        if (out.frame_d_sum) std::memcpy(out.frame_d_sum + f, fr + 5 * f + 3, sizeof(double));
        if (out.frame_d_max) std::memcpy(out.frame_d_max + f, fr + 5 * f + 4, sizeof(double));
    }
    run.lap(&patolette_amd__Stats::ms_download);
    run.done();
}

// --------------------------------------------------------------------------------------------
// gif_lzw: index maps LZW-compressed as a GIF's image data (include/patolette_amd.h, patolette_amd_gif_lzw)
// --------------------------------------------------------------------------------------------
// maps: frames x width x height one-byte elements, a device pointer when `on_device`; recs: the frames' rectangles with their first
// segments, frames + 1 records (lzw.h); seg: a segment's pixels; cap: the largest rectangle's area.  out, offsets: host memory.
// name: the entry's, ahead of what a failure says.  lossy: null for the exact coder (patolette_amd_gif_lzw), else the lossy one's table
// (host memory, checked) and `coded` -- null, or where the coded symbols go inside the rectangles: a device pointer when `on_device`.
struct LzwLossy { const unsigned char *near; unsigned char *coded; };
static void run_gif_lzw(Engine &E, const char *name, bool on_device, size_t frames, size_t width, size_t height, const unsigned char *maps,
                        const std::vector<LzwFrame> &recs, size_t seg, size_t cap, size_t bound, int m, const LzwLossy *lossy, unsigned char *out,
                        size_t capacity, uint64_t *offsets) {
    const size_t n = width * height, N = frames * n, S = recs[frames].seg0;
    hipStream_t s = E.stream;
    GivenRun run(E);
    const std::string who = std::string(name) + ": ";
    // the workspace, before anything is enqueued
    const size_t stride = lzw_stage_words(std::min(seg, cap)), words = lzw_words(frames), out_words = bound / 4 + 1;
    E.lz_frames.reserve(frames + 1);
    E.lz_stage.reserve(S * stride);
    E.lz_bits.reserve(S);
    E.lz_gbit.reserve(S + 1);
    E.lz_words.reserve(words);
    E.lz_out.reserve(out_words);
    unsigned char *d_coded = lossy ? lossy->coded : nullptr;
    std::vector<unsigned char> h_coded;                                    // host maps: the coded maps on their way to the rectangles
    if (lossy) {
        E.lz_near.reserve(kLzwNearBytes);
        if (!on_device && lossy->coded) { E.dl_shown.reserve(N); d_coded = E.dl_shown.p; h_coded.resize(N); }
    }
    const unsigned char *d_maps = maps;
    if (!on_device) {
        std::vector<unsigned> none;
        stage_given(E, maps, 1, 1, N, GivenSkip{}, 0, nullptr, 0, none);
        d_maps = E.dl_maps.p;
    }
    run.lap(&patolette_amd__Stats::ms_upload);
    HIP_CHECK(hipMemcpyAsync(E.lz_frames.p, recs.data(), (frames + 1) * sizeof(LzwFrame), hipMemcpyHostToDevice, s));
    if (lossy) {
        HIP_CHECK(hipMemcpyAsync(E.lz_near.p, lossy->near, kNearRow << m, hipMemcpyHostToDevice, s));   // the rows that are read
        launch_lzw_lossy(d_maps, frames, n, width, E.lz_frames.p, S, seg, stride, m, E.lz_near.p, d_coded, E.lz_stage.p, E.lz_bits.p, E.lz_gbit.p,
                         E.lz_words.p, E.lz_out.p, out_words, s);
    } else {
        launch_lzw(d_maps, frames, n, width, E.lz_frames.p, S, seg, stride, m, E.lz_stage.p, E.lz_bits.p, E.lz_gbit.p, E.lz_words.p, E.lz_out.p,
                   out_words, s);
    }
    const std::vector<unsigned long long> w = run.words(E.lz_words.p, words);
    run.lap(&patolette_amd__Stats::ms_map);
    if (w[0] & 1) throw HipError(who + "a map element inside a rectangle is not below 2^min_code_size");
    for (size_t f = 0; f <= frames; f++) offsets[f] = w[1 + f];
    const size_t total = (size_t)w[1 + frames];
    if (total > bound) throw HipError(who + "the streams exceed the stated bound (internal error)");
    if (total > capacity)
        throw HipError(who + "capacity is too small: offsets[frames] holds the bytes needed, nothing was copied");
    HIP_CHECK(hipMemcpy(out, E.lz_out.p, total, hipMemcpyDeviceToHost));
    if (!h_coded.empty()) {                                                // the rectangles' rows; nothing outside them is written
        HIP_CHECK(hipMemcpy(h_coded.data(), d_coded, N, hipMemcpyDeviceToHost));
        for (size_t f = 0; f < frames; f++) {
            const LzwFrame &F = recs[f];
            for (size_t y = 0; y < F.area / F.w; y++) {
                const size_t at = f * n + (F.y0 + y) * width + F.x0;
                std::memcpy(lossy->coded + at, h_coded.data() + at, F.w);
            }
        }
    }
    run.lap(&patolette_amd__Stats::ms_download);
    run.done();
}

// --------------------------------------------------------------------------------------------
// png_deflate: index maps deflated as an indexed PNG's image data (include/patolette_amd.h, patolette_amd_png_deflate)
// --------------------------------------------------------------------------------------------
// maps: frames x width x height one-byte elements, a device pointer when `on_device`; recs: the frames' rectangles with the FILTERED
// bytes as `area` and their first segments, frames + 1 records (lzw.h); bases: the frames' first bytes in the filtered streams, frames + 1;
// seg: a segment's filtered bytes; cap: the longest frame's.  out, offsets, adler: host memory.
static void run_png_deflate(Engine &E, bool on_device, size_t frames, size_t width, size_t height, const unsigned char *maps,
                            const std::vector<LzwFrame> &recs, const std::vector<unsigned long long> &bases, size_t seg, size_t cap, size_t bound,
                            unsigned char *out, size_t capacity, uint64_t *offsets, uint32_t *adler) {
    const size_t n = width * height, N = frames * n, S = recs[frames].seg0, stream_bytes = (size_t)bases[frames];
    hipStream_t s = E.stream;
    GivenRun run(E);
    const std::string who = "patolette_amd_png_deflate: ";
    // the workspace, before anything is enqueued
    const size_t longest = std::min(seg, cap), stride = deflate_stage_words(longest), tok_stride = deflate_token_stride(longest);
    const size_t words = deflate_words(frames, S), out_words = bound / 4 + 1;
    E.lz_frames.reserve(frames + 1);
    E.df_base.reserve(frames + 1);
    E.df_stream.reserve(stream_bytes + 2 * kDeflateStreamPad);             // (the streams start kDeflateStreamPad bytes in)
    E.df_tokens.reserve(S * tok_stride);
    E.lz_stage.reserve(S * stride);
    E.lz_bits.reserve(S);
    E.lz_gbit.reserve(S + 1);
    E.lz_words.reserve(words);
    E.lz_out.reserve(out_words);
    const unsigned char *d_maps = maps;
    if (!on_device) {
        std::vector<unsigned> none;
        stage_given(E, maps, 1, 1, N, GivenSkip{}, 0, nullptr, 0, none);
        d_maps = E.dl_maps.p;
    }
    run.lap(&patolette_amd__Stats::ms_upload);
    HIP_CHECK(hipMemcpyAsync(E.lz_frames.p, recs.data(), (frames + 1) * sizeof(LzwFrame), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(E.df_base.p, bases.data(), (frames + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    launch_deflate(d_maps, frames, n, width, E.lz_frames.p, E.df_base.p, stream_bytes, S, seg, tok_stride, stride, E.df_stream.p + kDeflateStreamPad, E.df_tokens.p,
                   E.lz_stage.p, E.lz_bits.p, E.lz_gbit.p, E.lz_words.p, E.lz_out.p, out_words, s);
    const std::vector<unsigned long long> w = run.words(E.lz_words.p, words);
    run.lap(&patolette_amd__Stats::ms_map);
    for (size_t f = 0; f <= frames; f++) offsets[f] = w[1 + f];
    const unsigned long long *sums = w.data() + frames + 2;                // a frame's Adler-32 from its segments' sums
    for (size_t f = 0; f < frames; f++) {
        Adler32 a;
        for (size_t k = recs[f].seg0; k < recs[f + 1].seg0; k++) {
            const size_t q0 = (k - recs[f].seg0) * seg;
            a.add(sums[2 * k], sums[2 * k + 1], std::min(seg, (size_t)recs[f].area - q0));
        }
        adler[f] = a.value();
    }
    const size_t total = (size_t)w[1 + frames];
    if (total > bound) throw HipError(who + "the streams exceed the stated bound (internal error)");
    if (total > capacity)
        throw HipError(who + "capacity is too small: offsets[frames] holds the bytes needed, nothing was copied");
    HIP_CHECK(hipMemcpy(out, E.lz_out.p, total, hipMemcpyDeviceToHost));
    run.lap(&patolette_amd__Stats::ms_download);
    run.done();
}

// The RGBA entry (include/patolette_amd.h, patolette_amd_rgba): the opaque pixels (alpha >= thr) are compacted in row-scan order and
// the path runs on them as an M x 1 image with one palette row less (row 0 is the transparent entry); the dither walks the full image's
// curve over them (DitherMask).  Every pixel opaque: the path runs on the image itself with the full palette, exactly as run_u8 does.
// One kernel then writes the full index map and the RGBA image.  `pixels`, `map_out`, `quant_out` are device pointers when `on_device`.
static void run_rgba(Engine &E, size_t width, size_t height, const unsigned char *pixels, int thr, const double *weights, double tile_size,
                     size_t K, const patolette__QuantizationOptions *opt, double *palette, unsigned char *palette_rgba, void *map_out,
                     int map_elem_out, unsigned char *quant_out, int *transparent_index, bool on_device) {
    const size_t N = width * height;
    hipStream_t s = E.stream;
    const double t_start = now_ms();
    WsGuard wg(&E.stream, &E.stream2);
    const bool weighted = weights || tile_size > 0.0;
    const bool want_map = !opt->palette_only && (map_out || quant_out);
    const int me = map_elem_for(K);                                  // the compact map (choices < K - 1 when masked)
    // everything the call can take of the workspace, before anything is enqueued (run_device's own preparation at M <= N pixels
    // is then a no-op, save for what it reserves behind a synchronisation)
    const RgbaOut out = rgba_out_place(E, "patolette_amd_rgba_device", N, on_device, pixels, want_map, map_out, map_elem_out, quant_out);
    E.rgba_cnt.reserve(compact_tiles(N) + 1); E.h_rgba_m.reserve(1);
    E.rgba_cpos.reserve(N); E.rgba_rgb.reserve(3 * N);
    if (weighted) E.rgba_w.reserve(N);
    E.pal8.reserve(4 * K);
    if (want_map) {
        E.dmap.reserve(N * (size_t)me);
        if (opt->dither) { E.aux.reserve(3 * N); dither_mask_reserve(E.nn, N); }
        else if (opt->color_space == patolette__CIELuv) E.aux.reserve(3 * N);
    }

    // upload (host images: converted behind the upload, as run_u8 -- kept if every pixel turns out opaque); behind it the count of the
    // opaque pixels (one small synchronisation); then the weights the binding derives (tile_size > 0): over the full image's RGB, as
    // run_u8 -- restricted to the opaque pixels below
    size_t M = 0;
    const QuantInput in = quant_input(E, t_start, Pixels{nullptr, pixels, 4}, on_device, out.stage_px, 1, width, height, weights, tile_size, K,
                                      opt, [&](const unsigned char *d_px) {
        unsigned *d_m = E.rgba_cnt.p + compact_tiles(N);
        launch_alpha_count(d_px, N, thr, E.rgba_cnt.p, d_m, s);
        HIP_CHECK(hipMemcpyAsync(E.h_rgba_m.p, d_m, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        M = E.h_rgba_m.p[0];
        if (M < N && M > 0 && K < 2) throw CodeError(-3, "Palette size should be greater than 0.");
        return M > 0;
    });
    const bool masked = M < N;
    if (transparent_index) *transparent_index = masked ? 0 : -1;

    const size_t Kq = masked ? K - 1 : K;                            // rows the path makes
    std::vector<double> pal(3 * std::max<size_t>(Kq, 1), -1.0);
    size_t len = 0;
    void *d_cmap = want_map ? (void *)E.dmap.p : nullptr;
    if (masked) {
        launch_alpha_compact(in.px.u8, N, M, thr, E.rgba_cnt.p, in.d_w, E.rgba_cpos.p, E.rgba_rgb.p, in.d_w ? E.rgba_w.p : nullptr, s);
        HIP_CHECK(hipStreamSynchronize(s));                           // (run_device sizes its workspace before it enqueues)
    }
    if (M > 0) {
        if (!masked) {
            run_device(E, width, height, in.px, in.d_w, K, opt, pal.data(), d_cmap, me);
        } else {
            const DitherMask mask{width, height, E.rgba_cpos.p};
            run_device(E, M, 1, Pixels{nullptr, E.rgba_rgb.p, 3}, in.d_w ? E.rgba_w.p : nullptr, Kq, opt, pal.data(), d_cmap, me, &mask);
        }
        len = E.stats.n_clusters;
    } else {
        E.stats = patolette_amd__Stats{};
    }
    const double t_out = now_ms();

    // palettes: row 0 the transparent entry when masked; unused rows -1 / (0, 0, 0, 0)
    const size_t off = masked ? 1 : 0;
    std::vector<unsigned char> p8(3 * std::max<size_t>(Kq, 1)), prgba(4 * K, 0);
    if (Kq > 0) palette_to_u8(pal.data(), Kq, p8.data());
    for (size_t i = 0; i < len; i++) {
        for (int c = 0; c < 3; c++) prgba[4 * (off + i) + c] = p8[3 * i + c];
        prgba[4 * (off + i) + 3] = 255;
    }
    if (palette) write_palette(palette, K, off, pal, Kq);
    if (palette_rgba) std::memcpy(palette_rgba, prgba.data(), 4 * K);

    if (want_map) {
        if (!masked && !map_touched(opt->dither, width, height))
            HIP_CHECK(hipMemsetAsync(E.dmap.p, 0, N * (size_t)me, s));        // (a 1x1 dither wrote nothing: entry 0)
        HIP_CHECK(hipMemcpyAsync(E.pal8.p, prgba.data(), 4 * K, hipMemcpyHostToDevice, s));
        launch_rgba_expand(d_cmap, me, masked ? E.rgba_cpos.p : nullptr, N, M, (unsigned)off, E.pal8.p, (int)K, out.d_map, map_elem_out, out.d_q, s);
        rgba_copy_out(E, out, N, map_out, map_elem_out, quant_out);   // (prgba is a local: the copy must have left the host)
    }
    quant_stats(E, in, t_out);
}

// --------------------------------------------------------------------------------------------
// ColorHistogram: an exact colour histogram in memory the caller owns (include/patolette_amd.h; the table: hist.h)
// --------------------------------------------------------------------------------------------
using HistWord = unsigned long long;

// `bytes` of device memory on the host, once everything enqueued has run
static void hist_read(Engine &E, void *dst, const void *d_src, size_t bytes) {
    HIP_CHECK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, E.stream));
    E.sync();
}
static const char *const kHistOverflow = "overflow: a weight sum passed 2^64 units; only a clear makes the histogram usable again";

// what every call but clear asks first: the table is a cleared one of this mode, and no sum in it has overflowed
static void hist_check(Engine &E, const char *name, const HistWord *d_hist, bool weighted) {
    HistWord h[2] = {0, 0};
    hist_read(E, h, d_hist, sizeof h);
    if (h[1] != kHistMagic + (weighted ? 1u : 0u)) throw named_error(name, "the memory is not a cleared histogram of this mode");
    if (h[0] & 1) throw named_error(name, kHistOverflow);
}

static void run_hist_clear(Engine &E, HistWord *d_hist, bool weighted) {
    const HistWord head[2] = {0, kHistMagic + (weighted ? 1u : 0u)};
    HIP_CHECK(hipMemsetAsync(d_hist, 0, hist_words(weighted) * sizeof(HistWord), E.stream));
    HIP_CHECK(hipMemcpyAsync(d_hist, head, sizeof head, hipMemcpyHostToDevice, E.stream));
    E.sync();                                                         // (head is a local: the copy must have left the host)
}

// pixels: frames x width x height x channels bytes; thr: -1, or the alpha below which a pixel enters nothing; weights: frames x
// width x height values or null -- then, in a weighted table, every frame's saliency weights.  `pixels` and `weights` are device
// pointers when `on_device`.  Everything that can refuse the add runs before k_hist_add is enqueued.
static void run_hist_add(Engine &E, const char *name, bool on_device, HistWord *d_hist, bool weighted, size_t frames, size_t width, size_t height,
                         const unsigned char *pixels, int channels, int thr, const double *weights, double tile_size) {
    const size_t N = frames * width * height;
    hipStream_t s = E.stream;
    GivenRun run(E);
    const bool derive = weighted && !weights;
    // the workspace, before anything is enqueued
    E.hs_words.reserve(4);
    if (weighted) E.hs_units.reserve(N);
    if (derive) { E.wsal.reserve(N); saliency_reserve(E.sal, width, height); }
    if (!on_device) { E.src8.reserve(N * (size_t)channels); if (weights) E.wsrc.reserve(N); }
    hist_check(E, name, d_hist, weighted);
    const unsigned char *d_px = pixels;
    const double *d_w = weights;
    if (!on_device) {
        HIP_CHECK(hipMemcpyAsync(E.src8.p, pixels, N * (size_t)channels, hipMemcpyHostToDevice, s));
        d_px = E.src8.p;
        if (weights) { HIP_CHECK(hipMemcpyAsync(E.wsrc.p, weights, N * sizeof(double), hipMemcpyHostToDevice, s)); d_w = E.wsrc.p; }
        HIP_CHECK(hipStreamSynchronize(s));
    }
    run.lap(&patolette_amd__Stats::ms_upload);
    E.ms_saliency = 0.0;
    if (derive) d_w = derive_weights(E, nullptr, d_px, channels, width, height, tile_size, frames);   // (all frames first; -5, -6, -7)
    E.stats.ms_saliency = E.ms_saliency;
    if (weighted) {
        HIP_CHECK(hipMemsetAsync(E.hs_words.p, 0, sizeof(HistWord), s));
        launch_hist_units(d_w, N, E.hs_units.p, reinterpret_cast<unsigned *>(E.hs_words.p), s);
        HistWord bad = 0;
        hist_read(E, &bad, E.hs_words.p, sizeof bad);
        if (bad & 1) throw named_error(name, "a weight is not finite or lies outside [0, 2^20]; nothing was added");
    }
    launch_hist_add(d_hist, weighted, d_px, channels, thr, N, weighted ? E.hs_units.p : nullptr, s);
    HistWord flags = 0;
    hist_read(E, &flags, d_hist, sizeof flags);
    run.lap(&patolette_amd__Stats::ms_map);
    if (flags & 1) throw named_error(name, kHistOverflow);
    run.done();
}

static void run_hist_merge(Engine &E, HistWord *d_hist, const HistWord *d_other, bool weighted) {
    static const char *const name = "patolette_amd_hist_merge";
    GivenRun run(E);
    hist_check(E, name, d_hist, weighted);
    hist_check(E, name, d_other, weighted);
    launch_hist_merge(d_hist, d_other, weighted, E.stream);
    HistWord flags = 0;
    hist_read(E, &flags, d_hist, sizeof flags);
    run.lap(&patolette_amd__Stats::ms_map);
    if (flags & 1) throw named_error(name, kHistOverflow);
    run.done();
}

static void run_hist_totals(Engine &E, const HistWord *d_hist, bool weighted, uint64_t *pixels, uint64_t *colors) {
    GivenRun run(E);
    E.hs_words.reserve(4);
    hist_check(E, "patolette_amd_hist_totals", d_hist, weighted);
    launch_hist_totals(d_hist, E.hs_words.p + 1, E.stream);
    HistWord t[2] = {0, 0};
    hist_read(E, t, E.hs_words.p + 1, sizeof t);
    if (pixels) *pixels = t[0];
    if (colors) *colors = t[1];
    run.lap(&patolette_amd__Stats::ms_map);
    run.done();
}

// The bins with count > 0 (`positive`: and weight > 0) compacted in key order into E.hs_rgb, E.hs_w and -- with want_counts --
// E.hs_counts; returns their number.  Nothing is enqueued when it returns.
static size_t hist_compact(Engine &E, const HistWord *d_hist, bool weighted, bool positive, bool want_counts, size_t capacity, const char *name) {
    hipStream_t s = E.stream;
    const size_t nt = compact_tiles(kHistBins);
    E.hs_tiles.reserve(nt + 1);
    launch_hist_export_count(d_hist, weighted, positive, E.hs_tiles.p, E.hs_tiles.p + nt, s);
    unsigned total = 0;
    hist_read(E, &total, E.hs_tiles.p + nt, sizeof total);
    const size_t M = total;
    if (M > capacity) throw named_error(name, "capacity is smaller than the number of colours (patolette_amd_hist_totals tells it)");
    if (M == 0) return 0;
    E.hs_rgb.reserve(3 * M); E.hs_w.reserve(M);
    if (want_counts) E.hs_counts.reserve(M);
    launch_hist_export_write(d_hist, weighted, positive, E.hs_tiles.p, E.hs_rgb.p, want_counts ? E.hs_counts.p : nullptr, E.hs_w.p, s);
    E.sync();
    return M;
}

static void run_hist_export(Engine &E, const HistWord *d_hist, bool weighted, size_t capacity, unsigned char *colors, uint64_t *counts,
                            double *weights) {
    static const char *const name = "patolette_amd_hist_export";
    GivenRun run(E);
    hist_check(E, name, d_hist, weighted);
    const size_t M = hist_compact(E, d_hist, weighted, false, counts != nullptr, capacity, name);
    run.lap(&patolette_amd__Stats::ms_map);
    if (M && colors) HIP_CHECK(hipMemcpy(colors, E.hs_rgb.p, 3 * M, hipMemcpyDeviceToHost));
    if (M && counts) HIP_CHECK(hipMemcpy(counts, E.hs_counts.p, M * sizeof(HistWord), hipMemcpyDeviceToHost));
    if (M && weights) HIP_CHECK(hipMemcpy(weights, E.hs_w.p, M * sizeof(double), hipMemcpyDeviceToHost));
    run.lap(&patolette_amd__Stats::ms_download);
    run.done();
}

// The palette of K rows from the colours with a weight above 0 (M' of them): the colours themselves while M' <= K, else what
// patolette_amd_u8_device returns for them as a 1 x M' image with those weights -- run_u8 itself, on the rows where they lie in HBM.
static void run_hist_palette(Engine &E, const HistWord *d_hist, bool weighted, size_t K, const patolette__QuantizationOptions *opt,
                             double *palette, unsigned char *palette_u8) {
    static const char *const name = "patolette_amd_hist_palette";
    GivenRun run(E);
    hist_check(E, name, d_hist, weighted);
    const size_t M = hist_compact(E, d_hist, weighted, true, false, kHistBins, name);
    run.lap(&patolette_amd__Stats::ms_map);
    if (M == 0) throw named_error(name, "the histogram holds no colour with a weight above 0");
    if (M > K) {                                                       // (the statistics are then run_u8's own: it resets them)
        patolette__QuantizationOptions o = *opt;
        o.dither = false; o.palette_only = false;
        run_u8(E, M, 1, E.hs_rgb.p, 3, E.hs_w.p, 0.0, K, &o, palette, palette_u8, nullptr, 1, nullptr, true, false, nullptr);
        return;
    }
    std::vector<unsigned char> rows(3 * M);
    HIP_CHECK(hipMemcpy(rows.data(), E.hs_rgb.p, 3 * M, hipMemcpyDeviceToHost));
    if (palette) {
        for (size_t j = 0; j < 3 * K; j++) palette[j] = -1.0;                                     // unused rows as run_device fills them
        for (int c = 0; c < 3; c++) for (size_t i = 0; i < M; i++) palette[K * (size_t)c + i] = (double)rows[3 * i + c] / 255.0;
    }
    if (palette_u8) {
        std::memset(palette_u8, 0, 3 * K);
        std::memcpy(palette_u8, rows.data(), 3 * M);
    }
    run.lap(&patolette_amd__Stats::ms_download);
    run.done();
}

static int validate_u8(size_t K, int channels, const void *map_out, int map_elem) {
    if (channels != 3 && channels != 4) return -1;
    if (map_out) {
        if (map_elem != 1 && map_elem != 2 && map_elem != 4 && map_elem != 8) return -1;
        if (map_elem == 1 && K > 256) return -1;
        if (map_elem == 2 && K > 65536) return -1;
    }
    return 0;
}

}  // namespace pamd

// ============================================================================================
// C ABI
// ============================================================================================
using namespace pamd;

static const char *kMessages[9] = {                                        // patolette.c:32-38, then the additive codes
    "Quantization successful.", "Internal quantization error.", "Image dimensions should be greater than 0.",
    "Palette size should be greater than 0.", "Image dimensions are too big.",
    "Saliency weights: image shape not supported (needs more than 3 pixels per side, at least 100 pixels, and a "
    "border band that fits).",
    "Saliency weights: a border band has a singular colour covariance.",
    "Saliency weights: the saliency map is degenerate (one of its normalising maxima is 0 or not finite, as for a constant "
    "channel mean); the reference's weights are NaN for this image.",
    nullptr};

static int comm_ok(const patolette_amd__Comm *comm) {
    return comm && comm->allreduce_sum && comm->size >= 1 && comm->rank >= 0 && comm->rank < comm->size;
}
static int slice_args_ok(size_t total_pixels, size_t slice_begin, size_t slice_pixels, const void *slice_data,
                         const patolette__QuantizationOptions *options, const void *slice_map) {
    return slice_pixels > 0 && slice_begin <= total_pixels && slice_pixels <= total_pixels - slice_begin && slice_data &&
           (options->palette_only || slice_map);
}
// Runs body(E) on the calling thread's engine, initialised.  Returns 0, or what a body that returns an int returns; a CodeError's own
// code (its message recorded, nothing printed); or -1 for any other failure (its message recorded for patolette_amd_last_error, and printed)
template <typename F>
static int guarded(F body) {
    try {
        Engine &E = engine();
        E.init();
        if constexpr (std::is_void_v<decltype(body(E))>) { body(E); return 0; }
        else return body(E);
    } catch (const CodeError &ex) {
        engine().last_error = ex.what();
        return ex.code;
    } catch (const std::exception &ex) {
        engine().last_error = ex.what();
        fprintf(stderr, "patolette: %s\n", ex.what());
        return -1;
    }
}
// An unusable argument, found before any engine is initialised (no device is needed to be told so): recorded, printed, the code set
static void fail_args(int *exit_code, int code, const char *msg) {
    try { engine().last_error = msg; } catch (...) {}
    fprintf(stderr, "%s\n", msg);
    *exit_code = code;
}
// The palette-given entries' arguments: fail() reports "<name>: <text>" through fail_args and returns false, as do the checks they share
struct ArgCheck {
    const char *name;
    int *exit_code;
    bool fail(int code, const char *text) const { fail_args(exit_code, code, (std::string(name) + ": " + text).c_str()); return false; }
    // frames of width x height: validate()'s codes with nothing recorded, then the cap on the pixels in all -- validate()'s own for one
    // image, or what the Riemersma walk of a remap numbers
    bool shape(size_t frames, size_t width, size_t height, bool dither = false) const {
        *exit_code = frames == 0 ? -2 : validate(width, height, 1);
        if (*exit_code != 0) return false;
        if (frames <= (dither ? kDitherFramesMaxPixels : (size_t)40000 * 40000) / (width * height)) return true;   // (n <= 1.6e9: no overflow before this)
        return fail(-4, dither ? "frames * width * height exceeds 2^31 pixels (the dither numbers pixels with 32 bits)" : "frames * width * height is too big");
    }
    bool map_elem_bytes(bool on_device, int eb) const {
        return (on_device ? (eb != 1 && eb != 4) : (eb != 1 && eb != 2 && eb != 4 && eb != 8))
                   ? fail(-1, "map_elem_bytes must be 1, 2, 4 or 8 (device maps: 1 or 4)") : true;
    }
    bool rows(size_t palette_rows, const char *text = "palette_rows must lie in [1, 2^31]") const {
        return palette_rows < 1 || palette_rows > ((size_t)1 << 31) ? fail(-1, text) : true;
    }
    bool one_of(const double *palette, const unsigned char *palette_u8, const char *text = "pass exactly one of palette and palette_u8") const {
        return (palette != nullptr) == (palette_u8 != nullptr) ? fail(-1, text) : true;
    }
    bool palette(const double *palette, const unsigned char *palette_u8, size_t palette_rows, bool want_bytes, GivenPalette &out) const {
        const GivenPaletteError e = given_palette(palette, palette_u8, palette_rows, want_bytes, out);
        return e == kGivenPaletteAllFill ? fail(-1, "every palette row is the unused-row fill (-1, -1, -1)")
             : e == kGivenPaletteNotFinite ? fail(-1, "the palette holds a value that is not finite") : true;
    }
    // what the frame deltas' lossy mode reads, up to the palette's parse (the caller's: RGBA maps prepare row 0 first)
    bool lossy(int channels, const unsigned char *pixels, const double *palette, const unsigned char *palette_u8) const {
        if (channels != 3 && channels != 4) return fail(-1, "channels must be 3 or 4");
        if (!pixels) return fail(-1, "a tolerance above 0 needs the frames' pixels");
        return one_of(palette, palette_u8, "a tolerance above 0 needs exactly one of palette and palette_u8");
    }
};

// runs `body` on the calling thread's engine with the slice description attached
// args_ok: this rank's arguments passed slice_args_ok.  A rank that returned early on bad arguments would leave its peers
// waiting in the first collective for ever, so the verdicts are summed over the group first and every rank fails together.
template <typename F>
static void slice_entry(size_t total_pixels, size_t slice_begin, const patolette_amd__Comm *comm, bool args_ok, int *exit_code, F body) {
    Shard sh;
    sh.total = total_pixels; sh.begin = slice_begin; sh.comm = *comm;
    Engine *Ep = nullptr;
    *exit_code = guarded([&](Engine &E) {
        Ep = &E;
        E.shard = &sh;
        int bad = args_ok ? 0 : 1;
        comm_sum_host(E, &bad, 1, 2);
        if (bad) throw HipError(args_ok ? "patolette_amd_slice: another rank of the group passed unusable arguments"
                                        : "patolette_amd_slice: unusable arguments (empty slice, slice outside the image, missing buffer)");
        body(E);
    });
    if (Ep) Ep->shard = nullptr;
}

// one f64 image in host memory, planar or (`rows`) row-major: validate()'s codes, then run_host
static void host_entry(bool rows, size_t width, size_t height, const double *data, const double *weights, double tile_size, size_t palette_size,
                       const patolette__QuantizationOptions *options, double *palette, size_t *palette_map, int *exit_code) {
    *exit_code = validate(width, height, palette_size);
    if (*exit_code != 0) return;
    *exit_code = guarded([&](Engine &E) { run_host(E, width, height, data, weights, tile_size, palette_size, options, palette, palette_map, rows); });
}
// run_device for an entry whose image is device memory: the caller's palette is written only when the run has succeeded
static void device_entry_run(Engine &E, size_t width, size_t height, const double *d_data, const double *d_weights, size_t palette_size,
                             const patolette__QuantizationOptions *options, double *palette, void *d_map, int map_elem_bytes) {
    std::vector<double> pal(3 * palette_size);
    run_device(E, width, height, Pixels{d_data, nullptr, 3}, d_weights, palette_size, options, pal.data(), d_map, map_elem_bytes);
    std::memcpy(palette, pal.data(), 3 * palette_size * sizeof(double));
}

extern "C" {

void patolette(size_t width, size_t height, const double *data, const double *weights, size_t palette_size,
               const patolette__QuantizationOptions *options, double *palette, size_t *palette_map, int *exit_code) {
    host_entry(false, width, height, data, weights, 0.0, palette_size, options, palette, palette_map, exit_code);
}

void patolette_amd_quantize(size_t width, size_t height, const double *data, const double *weights, double tile_size,
                            size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                            size_t *palette_map, int *exit_code) {
    host_entry(false, width, height, data, weights, tile_size, palette_size, options, palette, palette_map, exit_code);
}

void patolette_amd_quantize_rows(size_t width, size_t height, const double *rows, const double *weights, double tile_size,
                                 size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                                 size_t *palette_map, int *exit_code) {
    host_entry(true, width, height, rows, weights, tile_size, palette_size, options, palette, palette_map, exit_code);
}

void patolette_amd_slice(size_t total_pixels, size_t slice_begin, size_t slice_pixels, const double *slice_data,
                         const double *slice_weights, size_t palette_size, const patolette__QuantizationOptions *options,
                         const patolette_amd__Comm *comm, double *palette, size_t *slice_map, int *exit_code) {
    *exit_code = validate(total_pixels, 1, palette_size);
    if (*exit_code != 0) return;
    if (!comm_ok(comm)) { *exit_code = -1; return; }              // (validate() above is the same on every rank)
    slice_entry(total_pixels, slice_begin, comm, slice_args_ok(total_pixels, slice_begin, slice_pixels, slice_data, options, slice_map),
                exit_code, [&](Engine &E) {
        run_host(E, slice_pixels, 1, slice_data, slice_weights, 0.0, palette_size, options, palette, slice_map);
    });
}

void patolette_amd_slice_device(size_t total_pixels, size_t slice_begin, size_t slice_pixels, const double *d_slice_data,
                                const double *d_slice_weights, size_t palette_size, const patolette__QuantizationOptions *options,
                                const patolette_amd__Comm *comm, double *palette, void *d_slice_map, int map_elem_bytes,
                                int *exit_code) {
    *exit_code = validate(total_pixels, 1, palette_size);
    if (*exit_code != 0) return;
    if (!comm_ok(comm)) { *exit_code = -1; return; }
    slice_entry(total_pixels, slice_begin, comm, slice_args_ok(total_pixels, slice_begin, slice_pixels, d_slice_data, options, d_slice_map),
                exit_code, [&](Engine &E) {
        device_entry_run(E, slice_pixels, 1, d_slice_data, d_slice_weights, palette_size, options, palette, d_slice_map, map_elem_bytes);
    });
}

int patolette_amd_set_invariant_sums(int on) {
    const int before = invariant_default() ? 1 : 0;
    tl_invariant = on != 0 ? 1 : 0;
    EngineHolder &h = holder();
    if (h.e) h.e->invariant = on != 0;                // the engine already serving this thread; later ones copy tl_invariant
    return before;
}

int patolette_amd_set_subsample_cache(int on) {
    dither_order_cache(on != 0);             // the other size-only table kept between calls: the dither's curve order (map.hip)
    return g_perm_cache.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
}

int patolette_amd_set_kmeans_update(int mode) {
    const int before = km_update_order_free() ? 1 : 0;
    g_km_update.store(mode != 0 ? 1 : 0, std::memory_order_relaxed);
    return before;
}

int patolette_amd_saliency_weights(size_t width, size_t height, const double *data, double tile_size, double *weights_out) {
    const size_t N = width * height;
    if (N == 0) return kSalBadShape;
    const int rc = guarded([&](Engine &E) {
        E.src.reserve(3 * N);
        HIP_CHECK(hipMemcpyAsync(E.src.p, data, 3 * N * sizeof(double), hipMemcpyHostToDevice, E.stream));
        const double *d_w = derive_weights(E, E.src.p, nullptr, 3, width, height, tile_size);
        HIP_CHECK(hipMemcpy(weights_out, d_w, N * sizeof(double), hipMemcpyDeviceToHost));
    });
    return rc == -5 ? kSalBadShape : rc == -6 ? kSalSingular : rc == -7 ? kSalDegenerate : rc;   // (derive_weights' codes)
}

int patolette_amd_mbd(size_t rows, size_t cols, const float *img, int iters, float *out) {
    return guarded([&](Engine &E) {
        const int rc = mbd_device(E.sal, img, rows, cols, iters, out, E.stream);
        if (ktimer().enabled) ktimer().collect();
        return rc;
    });
}

const char *get_patolette_exit_code_info_message(int exit_code) {
    if (exit_code > 0 || exit_code < -7) return nullptr;
    return kMessages[-1 * exit_code];
}

patolette__QuantizationOptions *patolette_create_default_options(void) {   // patolette.c:107-119
    patolette__QuantizationOptions *o = (patolette__QuantizationOptions *)malloc(sizeof *o);
    o->dither = true; o->palette_only = false; o->color_space = patolette__ICtCp;
    o->kmeans_niter = 32; o->kmeans_max_samples = 512 * 512; o->verbose = false;
    return o;
}

int patolette_amd_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}
int patolette_amd_set_device(int ordinal) {
    if (hipSetDevice(ordinal) != hipSuccess) return -1;
    EngineHolder &h = holder();
    if (h.e && h.e->stream && h.e->device != ordinal) { pool_release(h.e); h.e = nullptr; }   // bound to another GPU: swap engines
    if (!h.e) h.e = pool_acquire(ordinal, invariant_default());
    h.e->device = ordinal;
    return 0;
}
void patolette_amd_release_workspace(void) {
    // this thread's engine and every idle pooled one: streams destroyed, device and pinned buffers freed; the next call
    // allocates afresh.  Engines in use by other threads (a batch in flight) are not touched.
    EngineHolder &h = holder();
    std::vector<Engine *> victims;
    if (h.e) { victims.push_back(h.e); h.e = nullptr; }
    { std::lock_guard<std::mutex> lk(g_pool_mu); victims.insert(victims.end(), g_pool.begin(), g_pool.end()); g_pool.clear(); }
    int cur = -1;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;      // ~Engine selects the engine's GPU: put the caller's back
    for (Engine *e : victims) delete e;
    if (have_cur) (void)hipSetDevice(cur);
}
const char *patolette_amd_last_error(void) { return engine().last_error.c_str(); }
void *patolette_amd_malloc(size_t bytes) { void *p = nullptr; if (hipMalloc(&p, bytes) != hipSuccess) return nullptr; return p; }
void patolette_amd_free(void *p) { if (p) (void)hipFree(p); }
int patolette_amd_memcpy_h2d(void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1; }
int patolette_amd_memcpy_d2h(void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
int patolette_amd_synchronize(void) { return hipDeviceSynchronize() == hipSuccess ? 0 : -1; }
int patolette_amd_fill_image(double *d, size_t n, uint64_t seed) {
    return guarded([&](Engine &E) { launch_fill_image(d, n, seed, E.stream); E.sync(); });
}
int patolette_amd_fill_weights(double *d, size_t n, uint64_t seed) {
    return guarded([&](Engine &E) { launch_fill_weights(d, n, seed, E.stream); E.sync(); });
}

void patolette_amd_device(size_t width, size_t height, const double *d_data, const double *d_weights, size_t palette_size,
                          const patolette__QuantizationOptions *options, double *palette, void *d_palette_map,
                          int map_elem_bytes, int *exit_code) {
    *exit_code = validate(width, height, palette_size);
    if (*exit_code != 0) return;
    *exit_code = guarded([&](Engine &E) {
        device_entry_run(E, width, height, d_data, d_weights, palette_size, options, palette, d_palette_map, map_elem_bytes);
    });
}

// F frames of one size, one palette (include/patolette_amd.h): the path on the stack of frames, the dither frame by frame.  The image
// entries (patolette_amd_u8*) are the case of one frame; bad_u8_args: the caller's text for what validate_u8 rejects
static void frames_entry(bool on_device, size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels,
                         const double *weights, double tile_size, size_t palette_size, const patolette__QuantizationOptions *options,
                         double *palette, unsigned char *palette_u8, void *palette_map, int map_elem_bytes, unsigned char *quantized,
                         const char *bad_u8_args, int *exit_code) {
    *exit_code = frames == 0 ? -2 : validate(width, height, palette_size);
    if (*exit_code != 0) return;
    const size_t n = width * height;
    if (frames > kDitherFramesMaxPixels / n)                        // (n <= 1.6e9: no overflow before this, and never with one frame)
        return fail_args(exit_code, -4, "patolette_amd_frames: frames * width * height exceeds 2^31 pixels");
    if (validate_u8(palette_size, channels, palette_map, map_elem_bytes) != 0) return fail_args(exit_code, -1, bad_u8_args);
    *exit_code = guarded([&](Engine &E) {
        const Frames fr{frames, width, height};
        run_u8(E, width, frames * height, pixels, channels, weights, tile_size, palette_size, options, palette, palette_u8, palette_map,
               map_elem_bytes, quantized, on_device, false, frames > 1 ? &fr : nullptr);      // (one frame: the image itself)
    });
}
static const char *const kBadFramesArgs = "patolette_amd_frames: bad channels / map_elem_bytes";
static const char *const kBadU8Args = "patolette_amd: bad channels / map_elem_bytes for the u8 entry point";

// 8-bit pixels onto the caller's palette (include/patolette_amd.h): the arguments, then run_remap
static void remap_entry(bool on_device, size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels, const double *palette,
                        const unsigned char *palette_u8, size_t palette_rows, int mode, double spread, void *palette_map, int map_elem_bytes,
                        unsigned char *quantized, int *exit_code) {
    // mode: kRemapNearest, kRemapRiemersma, or kRemapOrdered with its `spread` (the ordered map counts pixels as the nearest one does)
    const bool dither = mode == kRemapRiemersma;
    const ArgCheck arg{"patolette_amd_remap", exit_code};
    if (!arg.shape(frames, width, height, dither)) return;
    if (!arg.one_of(palette, palette_u8)) return;
    if (!arg.rows(palette_rows, "the palette needs at least one row")) return;
    if (validate_u8(palette_rows, channels, palette_map, map_elem_bytes) != 0)
        return (void)arg.fail(-1, "bad channels / map_elem_bytes (1, 2, 4 or 8, able to hold palette_rows - 1)");
    if (!pixels) return (void)arg.fail(-1, "no pixels");
    GivenPalette g;                                                        // with the bytes `quantized` is made of
    if (!arg.palette(palette, palette_u8, palette_rows, true, g)) return;
    if (mode == kRemapOrdered && !(std::isfinite(spread) && spread >= 0.0)) return (void)arg.fail(-1, "spread must be finite and not negative");
    *exit_code = guarded([&](Engine &E) {
        run_remap(E, frames, width, height, pixels, channels, std::move(g.pal), g.k, g.p8, palette_rows, mode, spread, palette_map, map_elem_bytes,
                  quantized, on_device);
    });
}

// RGBA pixels onto the caller's palette (include/patolette_amd.h): the arguments, then run_remap_rgba
static void remap_rgba_entry(bool on_device, size_t frames, size_t width, size_t height, const unsigned char *pixels, int alpha_threshold,
                             const double *palette, const unsigned char *palette_u8, size_t palette_rows, int transparent_index, int mode,
                             double spread, void *palette_map, int map_elem_bytes, unsigned char *quantized, int *exit_code) {
    const bool dither = mode == kRemapRiemersma;
    const ArgCheck arg{"patolette_amd_remap_rgba", exit_code};
    if (!arg.shape(frames, width, height, dither)) return;
    if (mode != kRemapNearest && mode != kRemapRiemersma && mode != kRemapOrdered) return (void)arg.fail(-1, "mode must be 0 (nearest), 1 (Riemersma) or 2 (ordered)");
    if (alpha_threshold < 0 || alpha_threshold > 256) return (void)arg.fail(-1, "alpha_threshold must lie in [0, 256]");
    if (transparent_index != -1 && transparent_index != 0) return (void)arg.fail(-1, "transparent_index must be -1 (none) or 0 (row 0)");
    if (!arg.one_of(palette, palette_u8)) return;
    if (!arg.rows(palette_rows, "the palette needs at least one row")) return;
    if (validate_u8(palette_rows, 4, palette_map, map_elem_bytes) != 0)
        return (void)arg.fail(-1, "bad map_elem_bytes (1, 2, 4 or 8, able to hold palette_rows - 1)");
    if (!pixels) return (void)arg.fail(-1, "no pixels");
    GivenPalette g;                                                        // with the bytes `quantized` is made of
    if (!arg.palette(palette, palette_u8, palette_rows, true, g)) return;
    const size_t off = transparent_index == 0 ? 1 : 0;
    if (g.k <= off) return (void)arg.fail(-1, "no opaque palette row remains beside the transparent entry");
    if (mode == kRemapOrdered && !(std::isfinite(spread) && spread >= 0.0)) return (void)arg.fail(-1, "spread must be finite and not negative");
    // the opaque rows, and every used row's RGBA word
    const size_t k = g.k - off;
    std::vector<double> pal(3 * k);
    for (int c = 0; c < 3; c++) for (size_t i = 0; i < k; i++) pal[(size_t)c * k + i] = g.pal[(size_t)c * g.k + off + i];
    const std::vector<unsigned> palw = given_row_words(g.p8, g.k, off, 0xFF000000u);
    *exit_code = guarded([&](Engine &E) {
        run_remap_rgba(E, frames, width, height, pixels, alpha_threshold, std::move(pal), k, palw, (unsigned)off, mode, spread, palette_map,
                       map_elem_bytes, quantized, on_device);
    });
}

// an animation's maps made deltas (include/patolette_amd.h): the arguments, then run_frame_deltas
static void frame_deltas_entry(bool on_device, size_t frames, size_t width, size_t height, const void *palette_maps, int map_elem_bytes,
                               size_t palette_rows, size_t transparent_index, const unsigned char *pixels, int channels, const double *palette,
                               const unsigned char *palette_u8, double tolerance, void *delta_maps, void *shown_maps, int32_t *rects,
                               uint64_t *changed, int *exit_code) {
    const ArgCheck arg{"patolette_amd_frame_deltas", exit_code};
    if (!arg.shape(frames, width, height)) return;
    const int eb = map_elem_bytes;
    if (!arg.map_elem_bytes(on_device, eb)) return;
    if (!palette_maps) return (void)arg.fail(-1, "no maps");
    if (!arg.rows(palette_rows)) return;
    if (transparent_index < palette_rows) return (void)arg.fail(-1, "transparent_index must be at least palette_rows (an index no entry uses)");
    if (eb < 8 && (transparent_index >> (8 * eb)) != 0)
        return (void)arg.fail(-1, "transparent_index does not fit an element of map_elem_bytes: no index is free for it -- make the palette with "
                                  "one row less, or pass wider elements");
    if (!(std::isfinite(tolerance) && tolerance >= 0.0)) return (void)arg.fail(-1, "tolerance must be finite and not negative");
    GivenPalette g;
    g.k = palette_rows;
    if (tolerance > 0.0) {                                                            // the lossy mode reads pixels and one palette
        if (!arg.lossy(channels, pixels, palette, palette_u8)) return;
        if (!arg.palette(palette, palette_u8, palette_rows, false, g)) return;
    }
    *exit_code = guarded([&](Engine &E) {
        run_frame_deltas(E, kPlainDeltas, on_device, frames, width, height, palette_maps, eb, g.k, transparent_index, 0, pixels, channels,
                         std::move(g.pal), tolerance, delta_maps, shown_maps, rects, nullptr, changed);
    });
}

// the deltas of maps whose index 0 is the transparent entry (include/patolette_amd.h): the arguments, then run_frame_deltas
static void frame_deltas_rgba_entry(bool on_device, size_t frames, size_t width, size_t height, const void *palette_maps, int map_elem_bytes,
                                    size_t palette_rows, const unsigned char *pixels, int channels, const double *palette,
                                    const unsigned char *palette_u8, double tolerance, int loop, void *delta_maps, void *shown_maps, int32_t *rects,
                                    int32_t *disposals, uint64_t *changed, int *exit_code) {
    const ArgCheck arg{"patolette_amd_frame_deltas_rgba", exit_code};
    if (!arg.shape(frames, width, height)) return;
    const int eb = map_elem_bytes;
    if (!arg.map_elem_bytes(on_device, eb)) return;
    if (!palette_maps) return (void)arg.fail(-1, "no maps");
    if (!arg.rows(palette_rows)) return;
    if (!(std::isfinite(tolerance) && tolerance >= 0.0)) return (void)arg.fail(-1, "tolerance must be finite and not negative");
    if (loop != 0 && loop != 1) return (void)arg.fail(-1, "loop must be 0 or 1");
    GivenPalette g;
    g.k = palette_rows;
    if (tolerance > 0.0) {                                                            // the lossy mode reads pixels and one palette
        if (!arg.lossy(channels, pixels, palette, palette_u8)) return;
        std::vector<double> opaque;                                                   // row 0 is the transparent entry: its colour is never read
        if (palette) {
            opaque.assign(palette, palette + 3 * palette_rows);
            for (int c = 0; c < 3; c++) opaque[(size_t)c * palette_rows] = 0.0;
        }
        if (!arg.palette(palette ? opaque.data() : nullptr, palette_u8, palette_rows, false, g)) return;
    }
    *exit_code = guarded([&](Engine &E) {
        run_frame_deltas(E, kRgbaDeltas, on_device, frames, width, height, palette_maps, eb, g.k, 0, loop, pixels, channels, std::move(g.pal), tolerance,
                         delta_maps, shown_maps, rects, disposals, changed);
    });
}

// the deltas of maps with a colour table per frame (include/patolette_amd.h): the arguments, then run_frame_deltas
static void frame_deltas_local_entry(bool on_device, size_t frames, size_t width, size_t height, const void *palette_maps,
                                     const unsigned char *palettes_u8, size_t palette_count, size_t palette_rows, const int32_t *palette_of,
                                     size_t transparent_index, const unsigned char *pixels, int channels, double tolerance, void *delta_maps,
                                     unsigned char *shown_rgb, int32_t *rects, uint64_t *changed, int *exit_code) {
    const ArgCheck arg{"patolette_amd_frame_deltas_local", exit_code};
    if (!arg.shape(frames, width, height)) return;
    if (!palette_maps) return (void)arg.fail(-1, "no maps");
    if (palette_rows < 1 || palette_rows > 255) return (void)arg.fail(-1, "palette_rows must lie in [1, 255]: a GIF table of 256 rows leaves no free index");
    if (palette_count < 1 || palette_count > 65536) return (void)arg.fail(-1, "palette_count must lie in [1, 65536]");
    if (transparent_index < palette_rows || transparent_index > 255)
        return (void)arg.fail(-1, "transparent_index must lie in [palette_rows, 255] (an index no table uses, in a one-byte element)");
    if (!palettes_u8) return (void)arg.fail(-1, "no palettes");
    if (!palette_of && palette_count != frames) return (void)arg.fail(-1, "without palette_of every frame has its own table: palette_count must equal frames");
    if (!(std::isfinite(tolerance) && tolerance >= 0.0)) return (void)arg.fail(-1, "tolerance must be finite and not negative");
    DeltaTables t{palette_count, palette_rows, {}, std::vector<int32_t>(frames)};
    for (size_t f = 0; f < frames; f++) {
        t.of[f] = palette_of ? palette_of[f] : (int32_t)f;
        if (t.of[f] < 0 || (size_t)t.of[f] >= palette_count) return (void)arg.fail(-1, "a palette_of value does not lie in [0, palette_count)");
    }
    GivenPalette g;                                                                   // all P K rows as one byte palette
    if (tolerance > 0.0) {
        if (channels != 3 && channels != 4) return (void)arg.fail(-1, "channels must be 3 or 4");
        if (!pixels) return (void)arg.fail(-1, "a tolerance above 0 needs the frames' pixels");
    }
    given_palette(nullptr, palettes_u8, palette_count * palette_rows, true, g);        // (bytes: nothing to reject)
    if (!(tolerance > 0.0)) g.pal.clear();
    t.p8 = std::move(g.p8);
    *exit_code = guarded([&](Engine &E) {
        run_frame_deltas(E, kLocalDeltas, on_device, frames, width, height, palette_maps, 1, palette_rows, transparent_index, 0, pixels, channels,
                         std::move(g.pal), tolerance, delta_maps, shown_rgb, rects, nullptr, changed, &t);
    });
}

// a map's error per entry and frame (include/patolette_amd.h): the arguments, then run_measure
static void measure_entry(bool on_device, size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels,
                          const void *palette_maps, int map_elem_bytes, const double *palette, const unsigned char *palette_u8, size_t palette_rows,
                          long long skip_index, const MeasureOut &out, int *exit_code) {
    const ArgCheck arg{"patolette_amd_measure", exit_code};
    if (!arg.shape(frames, width, height)) return;
    const int eb = map_elem_bytes;
    if (channels != 3 && channels != 4) return (void)arg.fail(-1, "channels must be 3 or 4");
    if (!arg.map_elem_bytes(on_device, eb)) return;
    if (!pixels) return (void)arg.fail(-1, "no pixels");
    if (!palette_maps) return (void)arg.fail(-1, "no maps");
    if (!arg.one_of(palette, palette_u8)) return;
    if (!arg.rows(palette_rows)) return;
    if (skip_index < -1) return (void)arg.fail(-1, "skip_index must be -1 (none) or an index");
    GivenPalette g;                                                        // with the bytes the integer part compares with
    if (!arg.palette(palette, palette_u8, palette_rows, true, g)) return;
    *exit_code = guarded([&](Engine &E) {
        run_measure(E, on_device, frames, width, height, pixels, channels, palette_maps, eb, std::move(g.pal), g.k, g.p8, palette_rows, skip_index, out);
    });
}

// index maps LZW-compressed (include/patolette_amd.h), by the exact coder or -- `lossy` -- the lossy one: the arguments, then run_gif_lzw
static void gif_lzw_entry(const char *name, bool on_device, size_t frames, size_t width, size_t height, const unsigned char *maps,
                          const int32_t *rects, int min_code_size, size_t segment, const LzwLossy *lossy, unsigned char *out, size_t capacity,
                          uint64_t *offsets, int *exit_code) {
    const ArgCheck arg{name, exit_code};
    if (!arg.shape(frames, width, height)) return;
    if (!maps) return (void)arg.fail(-1, "no maps");
    if (!offsets) return (void)arg.fail(-1, "no offsets");
    if (!out && capacity > 0) return (void)arg.fail(-1, "no out");
    if (min_code_size < 2 || min_code_size > 8) return (void)arg.fail(-1, "min_code_size must lie in [2, 8]");
    if (segment > kLzwSegmentMax) return (void)arg.fail(-1, "segment must be 0 (the default) or lie in [1, 2^24]");
    if (lossy) {
        if (!lossy->near) return (void)arg.fail(-1, "no near: the table of patolette_amd_gif_neighbours, or any 4096 bytes of its layout");
        const NearError e = near_check(lossy->near, min_code_size);
        if (e == kNearCount) return (void)arg.fail(-1, "near: a row below 2^min_code_size has a count above 15");
        if (e == kNearCandidate) return (void)arg.fail(-1, "near: a candidate of a row below 2^min_code_size is not below 2^min_code_size");
        const size_t N = frames * width * height;
        const uintptr_t a = (uintptr_t)maps, b = (uintptr_t)lossy->coded;
        if (lossy->coded && a < b + N && b < a + N) return (void)arg.fail(-1, "coded must not overlap maps");
    }
    const size_t seg = segment ? segment : kLzwSegment;
    std::vector<LzwFrame> recs;
    try { recs.resize(frames + 1); } catch (const std::bad_alloc &) { return (void)arg.fail(-1, "no memory for the frames' table"); }
    size_t S = 0, cap = 0, bound = 0;                                      // (S <= frames * width * height <= 1.6e9: 31 bits)
    for (size_t f = 0; f < frames; f++) {
        long long x0 = 0, y0 = 0, w = (long long)width, h = (long long)height;
        if (rects) { x0 = rects[4 * f]; y0 = rects[4 * f + 1]; w = rects[4 * f + 2]; h = rects[4 * f + 3]; }
        if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || x0 + w > (long long)width || y0 + h > (long long)height)
            return (void)arg.fail(-1, "every rectangle must lie inside the frame and have w, h >= 1");
        const size_t area = (size_t)w * (size_t)h, nseg = ceil_div(area, seg);
        recs[f] = LzwFrame{(unsigned)x0, (unsigned)y0, (unsigned)w, (unsigned)area, (unsigned)S};
        S += nseg;
        cap = std::max(cap, area);
        bound += lzw_frame_bound(area, nseg);
    }
    recs[frames] = LzwFrame{0, 0, 0, 0, (unsigned)S};
    *exit_code = guarded([&](Engine &E) {
        run_gif_lzw(E, name, on_device, frames, width, height, maps, recs, seg, cap, bound, min_code_size, lossy, out, capacity, offsets);
    });
}

// index maps deflated as PNG image data (include/patolette_amd.h): the arguments, then run_png_deflate
static void png_deflate_entry(bool on_device, size_t frames, size_t width, size_t height, const unsigned char *maps, const int32_t *rects,
                              size_t segment, unsigned char *out, size_t capacity, uint64_t *offsets, uint32_t *adler, int *exit_code) {
    const ArgCheck arg{"patolette_amd_png_deflate", exit_code};
    if (!arg.shape(frames, width, height)) return;
    if (!maps) return (void)arg.fail(-1, "no maps");
    if (!offsets) return (void)arg.fail(-1, "no offsets");
    if (!adler) return (void)arg.fail(-1, "no adler");
    if (!out && capacity > 0) return (void)arg.fail(-1, "no out");
    if (segment > kDeflateSegmentMax) return (void)arg.fail(-1, "segment must be 0 (the default) or lie in [1, 32768]");
    const size_t seg = segment ? segment : kDeflateSegment;
    std::vector<LzwFrame> recs;
    std::vector<unsigned long long> bases;
    try { recs.resize(frames + 1); bases.resize(frames + 1); } catch (const std::bad_alloc &) { return (void)arg.fail(-1, "no memory for the frames' table"); }
    size_t S = 0, cap = 0, bound = 0, at = 0;                              // (S <= 2 * frames * width * height <= 3.2e9: checked at the launch)
    for (size_t f = 0; f < frames; f++) {
        long long x0 = 0, y0 = 0, w = (long long)width, h = (long long)height;
        if (rects) { x0 = rects[4 * f]; y0 = rects[4 * f + 1]; w = rects[4 * f + 2]; h = rects[4 * f + 3]; }
        if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || x0 + w > (long long)width || y0 + h > (long long)height)
            return (void)arg.fail(-1, "every rectangle must lie inside the frame and have w, h >= 1");
        const size_t flen = deflate_filtered((size_t)w, (size_t)h), nseg = ceil_div(flen, seg);   // (flen <= 2 * 1.6e9: 32 bits)
        recs[f] = LzwFrame{(unsigned)x0, (unsigned)y0, (unsigned)w, (unsigned)flen, (unsigned)S};
        bases[f] = at;
        at += flen;
        S += nseg;
        cap = std::max(cap, flen);
        bound += deflate_frame_bound(flen, nseg);
    }
    if (S >> 31) return (void)arg.fail(-4, "frames * width * height is too big for this segment");
    recs[frames] = LzwFrame{0, 0, 0, 0, (unsigned)S};
    bases[frames] = at;
    *exit_code = guarded([&](Engine &E) {
        run_png_deflate(E, on_device, frames, width, height, maps, recs, bases, seg, cap, bound, out, capacity, offsets, adler);
    });
}

// the lossy coder's table for a palette (include/patolette_amd.h): host code from end to end -- no engine, no device
static void gif_neighbours_entry(const double *palette, const unsigned char *palette_u8, size_t palette_rows, int transparent_index, double tolerance,
                                 int max_neighbours, unsigned char *near_out, int *exit_code) {
    const ArgCheck arg{"patolette_amd_gif_neighbours", exit_code};
    if (!arg.one_of(palette, palette_u8)) return;
    if (palette_rows < 1 || palette_rows > kNearRows) return (void)arg.fail(-1, "palette_rows must lie in [1, 256]");
    if (transparent_index < -1 || transparent_index > 255) return (void)arg.fail(-1, "transparent_index must be -1 (none) or lie in [0, 255]");
    if (!(std::isfinite(tolerance) && tolerance >= 0.0)) return (void)arg.fail(-1, "tolerance must be finite and not negative");
    if (max_neighbours < 0 || max_neighbours > (int)kNearMost) return (void)arg.fail(-1, "max_neighbours must lie in [0, 15]");
    if (!near_out) return (void)arg.fail(-1, "no near_out");
    try {
        GivenPalette g;
        if (!arg.palette(palette, palette_u8, palette_rows, false, g)) return;
        near_build(std::move(g.pal), g.k, transparent_index, tolerance, (size_t)max_neighbours, near_out);
        *exit_code = 0;
    } catch (const std::bad_alloc &) { arg.fail(-1, "no memory for the palette"); }
}

static void rgba_entry(bool on_device, size_t width, size_t height, const unsigned char *pixels, int alpha_threshold, const double *weights,
                       double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                       unsigned char *palette_rgba, void *palette_map, int map_elem_bytes, unsigned char *quantized, int *transparent_index,
                       int *exit_code) {
    *exit_code = validate(width, height, palette_size);
    if (*exit_code != 0) return;
    if (alpha_threshold < 0 || alpha_threshold > 256) return fail_args(exit_code, -1, "patolette_amd_rgba: alpha_threshold must lie in [0, 256]");
    if (validate_u8(palette_size, 4, palette_map, map_elem_bytes) != 0)
        return fail_args(exit_code, -1, "patolette_amd_rgba: map_elem_bytes must be 1, 2, 4 or 8 and able to hold palette_size - 1");
    *exit_code = guarded([&](Engine &E) {
        run_rgba(E, width, height, pixels, alpha_threshold, weights, tile_size, palette_size, options, palette, palette_rgba, palette_map,
                 map_elem_bytes, quantized, transparent_index, on_device);
    });
}

void patolette_amd_rgba(size_t width, size_t height, const unsigned char *pixels, int alpha_threshold, const double *weights, double tile_size,
                        size_t palette_size, const patolette__QuantizationOptions *options, double *palette, unsigned char *palette_rgba,
                        void *palette_map, int map_elem_bytes, unsigned char *quantized, int *transparent_index, int *exit_code) {
    rgba_entry(false, width, height, pixels, alpha_threshold, weights, tile_size, palette_size, options, palette, palette_rgba, palette_map,
               map_elem_bytes, quantized, transparent_index, exit_code);
}

void patolette_amd_rgba_device(size_t width, size_t height, const unsigned char *d_pixels, int alpha_threshold, const double *d_weights,
                               double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                               unsigned char *palette_rgba, void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized,
                               int *transparent_index, int *exit_code) {
    rgba_entry(true, width, height, d_pixels, alpha_threshold, d_weights, tile_size, palette_size, options, palette, palette_rgba,
               d_palette_map, map_elem_bytes, d_quantized, transparent_index, exit_code);
}

void patolette_amd_remap_u8(size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels, const double *palette,
                            const unsigned char *palette_u8, size_t palette_rows, int dither, void *palette_map, int map_elem_bytes,
                            unsigned char *quantized, int *exit_code) {
    remap_entry(false, frames, width, height, pixels, channels, palette, palette_u8, palette_rows, dither ? kRemapRiemersma : kRemapNearest, 0.0,
                palette_map, map_elem_bytes, quantized, exit_code);
}

void patolette_amd_remap_u8_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int channels, const double *palette,
                                   const unsigned char *palette_u8, size_t palette_rows, int dither, void *d_palette_map, int map_elem_bytes,
                                   unsigned char *d_quantized, int *exit_code) {
    remap_entry(true, frames, width, height, d_pixels, channels, palette, palette_u8, palette_rows, dither ? kRemapRiemersma : kRemapNearest, 0.0,
                d_palette_map, map_elem_bytes, d_quantized, exit_code);
}

void patolette_amd_remap_ordered_u8(size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels, const double *palette,
                                    const unsigned char *palette_u8, size_t palette_rows, double spread, void *palette_map, int map_elem_bytes,
                                    unsigned char *quantized, int *exit_code) {
    remap_entry(false, frames, width, height, pixels, channels, palette, palette_u8, palette_rows, kRemapOrdered, spread, palette_map,
                map_elem_bytes, quantized, exit_code);
}

void patolette_amd_remap_ordered_u8_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int channels,
                                           const double *palette, const unsigned char *palette_u8, size_t palette_rows, double spread,
                                           void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized, int *exit_code) {
    remap_entry(true, frames, width, height, d_pixels, channels, palette, palette_u8, palette_rows, kRemapOrdered, spread, d_palette_map,
                map_elem_bytes, d_quantized, exit_code);
}

int patolette_amd_debug_remap_two_pass(int on) { return g_remap_two_pass.exchange(on ? 1 : 0); }

void patolette_amd_remap_rgba_u8(size_t frames, size_t width, size_t height, const unsigned char *pixels, int alpha_threshold,
                                 const double *palette, const unsigned char *palette_u8, size_t palette_rows, int transparent_index, int mode,
                                 double spread, void *palette_map, int map_elem_bytes, unsigned char *quantized, int *exit_code) {
    remap_rgba_entry(false, frames, width, height, pixels, alpha_threshold, palette, palette_u8, palette_rows, transparent_index, mode, spread,
                     palette_map, map_elem_bytes, quantized, exit_code);
}

void patolette_amd_remap_rgba_u8_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int alpha_threshold,
                                        const double *palette, const unsigned char *palette_u8, size_t palette_rows, int transparent_index,
                                        int mode, double spread, void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized,
                                        int *exit_code) {
    remap_rgba_entry(true, frames, width, height, d_pixels, alpha_threshold, palette, palette_u8, palette_rows, transparent_index, mode, spread,
                     d_palette_map, map_elem_bytes, d_quantized, exit_code);
}

int patolette_amd_debug_rgba_stamp_quad(int mode) { return rgba_stamp_debug_quad(mode); }

int patolette_amd_debug_delta_quad(int mode) { return delta_debug_quad(mode); }
int patolette_amd_debug_delta_local_tables(int mode) { return delta_debug_local_tables(mode); }
int patolette_amd_debug_delta_local_route(void) { return delta_local_route(); }

void patolette_amd_frame_deltas_local(size_t frames, size_t width, size_t height, const unsigned char *palette_maps,
                                      const unsigned char *palettes_u8, size_t palette_count, size_t palette_rows, const int32_t *palette_of,
                                      size_t transparent_index, const unsigned char *pixels, int channels, double tolerance,
                                      unsigned char *delta_maps, unsigned char *shown_rgb, int32_t *rects, uint64_t *changed, int *exit_code) {
    frame_deltas_local_entry(false, frames, width, height, palette_maps, palettes_u8, palette_count, palette_rows, palette_of, transparent_index,
                             pixels, channels, tolerance, delta_maps, shown_rgb, rects, changed, exit_code);
}
void patolette_amd_frame_deltas_local_device(size_t frames, size_t width, size_t height, const unsigned char *d_palette_maps,
                                             const unsigned char *palettes_u8, size_t palette_count, size_t palette_rows,
                                             const int32_t *palette_of, size_t transparent_index, const unsigned char *d_pixels, int channels,
                                             double tolerance, unsigned char *d_delta_maps, unsigned char *d_shown_rgb, int32_t *rects,
                                             uint64_t *changed, int *exit_code) {
    frame_deltas_local_entry(true, frames, width, height, d_palette_maps, palettes_u8, palette_count, palette_rows, palette_of, transparent_index,
                             d_pixels, channels, tolerance, d_delta_maps, d_shown_rgb, rects, changed, exit_code);
}

void patolette_amd_frame_deltas(size_t frames, size_t width, size_t height, const void *palette_maps, int map_elem_bytes, size_t palette_rows,
                                size_t transparent_index, const unsigned char *pixels, int channels, const double *palette,
                                const unsigned char *palette_u8, double tolerance, void *delta_maps, void *shown_maps, int32_t *rects,
                                uint64_t *changed, int *exit_code) {
    frame_deltas_entry(false, frames, width, height, palette_maps, map_elem_bytes, palette_rows, transparent_index, pixels, channels, palette,
                       palette_u8, tolerance, delta_maps, shown_maps, rects, changed, exit_code);
}

void patolette_amd_frame_deltas_device(size_t frames, size_t width, size_t height, const void *d_palette_maps, int map_elem_bytes,
                                       size_t palette_rows, size_t transparent_index, const unsigned char *d_pixels, int channels,
                                       const double *palette, const unsigned char *palette_u8, double tolerance, void *d_delta_maps,
                                       void *d_shown_maps, int32_t *rects, uint64_t *changed, int *exit_code) {
    frame_deltas_entry(true, frames, width, height, d_palette_maps, map_elem_bytes, palette_rows, transparent_index, d_pixels, channels, palette,
                       palette_u8, tolerance, d_delta_maps, d_shown_maps, rects, changed, exit_code);
}

void patolette_amd_frame_deltas_rgba(size_t frames, size_t width, size_t height, const void *palette_maps, int map_elem_bytes,
                                     size_t palette_rows, const unsigned char *pixels, int channels, const double *palette,
                                     const unsigned char *palette_u8, double tolerance, int loop, void *delta_maps, void *shown_maps,
                                     int32_t *rects, int32_t *disposals, uint64_t *changed, int *exit_code) {
    frame_deltas_rgba_entry(false, frames, width, height, palette_maps, map_elem_bytes, palette_rows, pixels, channels, palette, palette_u8,
                            tolerance, loop, delta_maps, shown_maps, rects, disposals, changed, exit_code);
}

void patolette_amd_frame_deltas_rgba_device(size_t frames, size_t width, size_t height, const void *d_palette_maps, int map_elem_bytes,
                                            size_t palette_rows, const unsigned char *d_pixels, int channels, const double *palette,
                                            const unsigned char *palette_u8, double tolerance, int loop, void *d_delta_maps,
                                            void *d_shown_maps, int32_t *rects, int32_t *disposals, uint64_t *changed, int *exit_code) {
    frame_deltas_rgba_entry(true, frames, width, height, d_palette_maps, map_elem_bytes, palette_rows, d_pixels, channels, palette, palette_u8,
                            tolerance, loop, d_delta_maps, d_shown_maps, rects, disposals, changed, exit_code);
}

void patolette_amd_measure(size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels, const void *palette_maps,
                           int map_elem_bytes, const double *palette, const unsigned char *palette_u8, size_t palette_rows, long long skip_index,
                           uint64_t *entry_count, uint64_t *entry_sse, uint32_t *entry_max_se, uint64_t *frame_count, uint64_t *frame_sse,
                           uint32_t *frame_max_se, double *frame_d_sum, double *frame_d_max, int *exit_code) {
    measure_entry(false, frames, width, height, pixels, channels, palette_maps, map_elem_bytes, palette, palette_u8, palette_rows, skip_index,
                  MeasureOut{entry_count, entry_sse, entry_max_se, frame_count, frame_sse, frame_max_se, frame_d_sum, frame_d_max}, exit_code);
}

void patolette_amd_measure_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int channels,
                                  const void *d_palette_maps, int map_elem_bytes, const double *palette, const unsigned char *palette_u8,
                                  size_t palette_rows, long long skip_index, uint64_t *entry_count, uint64_t *entry_sse, uint32_t *entry_max_se,
                                  uint64_t *frame_count, uint64_t *frame_sse, uint32_t *frame_max_se, double *frame_d_sum, double *frame_d_max,
                                  int *exit_code) {
    measure_entry(true, frames, width, height, d_pixels, channels, d_palette_maps, map_elem_bytes, palette, palette_u8, palette_rows, skip_index,
                  MeasureOut{entry_count, entry_sse, entry_max_se, frame_count, frame_sse, frame_max_se, frame_d_sum, frame_d_max}, exit_code);
}

void patolette_amd_gif_lzw(size_t frames, size_t width, size_t height, const unsigned char *maps, const int32_t *rects, int min_code_size,
                           size_t segment, unsigned char *out, size_t capacity, uint64_t *offsets, int *exit_code) {
    gif_lzw_entry("patolette_amd_gif_lzw", false, frames, width, height, maps, rects, min_code_size, segment, nullptr, out, capacity, offsets, exit_code);
}

void patolette_amd_gif_lzw_device(size_t frames, size_t width, size_t height, const unsigned char *d_maps, const int32_t *rects, int min_code_size,
                                  size_t segment, unsigned char *out, size_t capacity, uint64_t *offsets, int *exit_code) {
    gif_lzw_entry("patolette_amd_gif_lzw", true, frames, width, height, d_maps, rects, min_code_size, segment, nullptr, out, capacity, offsets, exit_code);
}

void patolette_amd_png_deflate(size_t frames, size_t width, size_t height, const unsigned char *maps, const int32_t *rects, size_t segment,
                               unsigned char *out, size_t capacity, uint64_t *offsets, uint32_t *adler, int *exit_code) {
    png_deflate_entry(false, frames, width, height, maps, rects, segment, out, capacity, offsets, adler, exit_code);
}

void patolette_amd_png_deflate_device(size_t frames, size_t width, size_t height, const unsigned char *d_maps, const int32_t *rects, size_t segment,
                                      unsigned char *out, size_t capacity, uint64_t *offsets, uint32_t *adler, int *exit_code) {
    png_deflate_entry(true, frames, width, height, d_maps, rects, segment, out, capacity, offsets, adler, exit_code);
}

// tests: the host's block for a token list (deflate_codes.h, write_block); no device, no engine
int patolette_amd_debug_deflate_block(const uint32_t *tokens, size_t count, int final_block, unsigned char *out, size_t capacity, uint64_t *bits) {
    if (!bits || (count && !tokens)) return -1;
    *bits = 0;
    for (size_t i = 0; i < count; i++) {                                // literals below 256; a match's unused bits clear, its length within 258
        const uint32_t t = tokens[i];
        if (dc::tok_is_match(t) ? (t & 0x7f008000u) != 0 || dc::tok_len(t) > dc::kMaxMatch : t > 255u) return -1;
    }
#if defined(__HIP_DEVICE_COMPILE__)                                     // (write_block exists in the host's pass alone)
    return -1;
#else
    dc::BitWriter bw;
    *bits = dc::write_block(tokens, count, final_block != 0, bw);
    if (!out || bw.bytes.size() > capacity) return -1;
    if (!bw.bytes.empty()) std::memcpy(out, bw.bytes.data(), bw.bytes.size());
    return 0;
#endif
}

void patolette_amd_gif_lzw_lossy(size_t frames, size_t width, size_t height, const unsigned char *maps, const int32_t *rects, int min_code_size,
                                 size_t segment, const unsigned char *near, unsigned char *coded, unsigned char *out, size_t capacity,
                                 uint64_t *offsets, int *exit_code) {
    const LzwLossy lossy{near, coded};
    gif_lzw_entry("patolette_amd_gif_lzw_lossy", false, frames, width, height, maps, rects, min_code_size, segment, &lossy, out, capacity, offsets,
                  exit_code);
}

void patolette_amd_gif_lzw_lossy_device(size_t frames, size_t width, size_t height, const unsigned char *d_maps, const int32_t *rects,
                                        int min_code_size, size_t segment, const unsigned char *near, unsigned char *d_coded, unsigned char *out,
                                        size_t capacity, uint64_t *offsets, int *exit_code) {
    const LzwLossy lossy{near, d_coded};
    gif_lzw_entry("patolette_amd_gif_lzw_lossy", true, frames, width, height, d_maps, rects, min_code_size, segment, &lossy, out, capacity, offsets,
                  exit_code);
}

void patolette_amd_gif_neighbours(const double *palette, const unsigned char *palette_u8, size_t palette_rows, int transparent_index,
                                  double tolerance, int max_neighbours, unsigned char *near_out, int *exit_code) {
    gif_neighbours_entry(palette, palette_u8, palette_rows, transparent_index, tolerance, max_neighbours, near_out, exit_code);
}

void patolette_amd_frames_u8(size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels, const double *weights,
                             double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                             unsigned char *palette_u8, void *palette_map, int map_elem_bytes, unsigned char *quantized, int *exit_code) {
    frames_entry(false, frames, width, height, pixels, channels, weights, tile_size, palette_size, options, palette, palette_u8, palette_map,
                 map_elem_bytes, quantized, kBadFramesArgs, exit_code);
}

void patolette_amd_frames_u8_device(size_t frames, size_t width, size_t height, const unsigned char *d_pixels, int channels,
                                    const double *d_weights, double tile_size, size_t palette_size,
                                    const patolette__QuantizationOptions *options, double *palette, unsigned char *palette_u8,
                                    void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized, int *exit_code) {
    frames_entry(true, frames, width, height, d_pixels, channels, d_weights, tile_size, palette_size, options, palette, palette_u8,
                 d_palette_map, map_elem_bytes, d_quantized, kBadFramesArgs, exit_code);
}

void patolette_amd_u8(size_t width, size_t height, const unsigned char *pixels, int channels, const double *weights,
                      double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                      unsigned char *palette_u8, void *palette_map, int map_elem_bytes, unsigned char *quantized, int *exit_code) {
    frames_entry(false, 1, width, height, pixels, channels, weights, tile_size, palette_size, options, palette, palette_u8, palette_map,
                 map_elem_bytes, quantized, kBadU8Args, exit_code);
}

void patolette_amd_u8_device(size_t width, size_t height, const unsigned char *d_pixels, int channels, const double *d_weights,
                             double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *palette,
                             unsigned char *palette_u8, void *d_palette_map, int map_elem_bytes, unsigned char *d_quantized,
                             int *exit_code) {
    frames_entry(true, 1, width, height, d_pixels, channels, d_weights, tile_size, palette_size, options, palette, palette_u8,
                 d_palette_map, map_elem_bytes, d_quantized, kBadU8Args, exit_code);
}

// ---- ColorHistogram (include/patolette_amd.h): the arguments, then the run_hist_* above
size_t patolette_amd_hist_bytes(int weighted) { return hist_words(weighted != 0) * sizeof(HistWord); }

int patolette_amd_hist_clear(void *d_hist, int weighted) {
    int code = 0;
    if (!d_hist) { ArgCheck{"patolette_amd_hist_clear", &code}.fail(-1, "no histogram"); return code; }
    return guarded([&](Engine &E) { run_hist_clear(E, (HistWord *)d_hist, weighted != 0); });
}

static void hist_add_entry(bool on_device, void *d_hist, int weighted, size_t frames, size_t width, size_t height, const unsigned char *pixels,
                           int channels, int alpha_threshold, const double *weights, double tile_size, int *exit_code) {
    static const char *const name = "patolette_amd_hist_add";
    const ArgCheck arg{name, exit_code};
    if (!arg.shape(frames, width, height)) return;
    if (!d_hist) return (void)arg.fail(-1, "no histogram");
    if (!pixels) return (void)arg.fail(-1, "no pixels");
    if (channels != 3 && channels != 4) return (void)arg.fail(-1, "channels must be 3 or 4");
    if (alpha_threshold < -1 || alpha_threshold > 255) return (void)arg.fail(-1, "alpha_threshold must be -1 (none) or lie in [0, 255]");
    if (alpha_threshold >= 0 && channels != 4) return (void)arg.fail(-1, "an alpha_threshold needs pixels of 4 channels");
    const bool derive = !weights && tile_size > 0.0;
    if (weighted && !weights && !derive) return (void)arg.fail(-1, "a weighted histogram needs weights, or a tile_size above 0 to derive them");
    if (!weighted && (weights || derive)) return (void)arg.fail(-1, "an unweighted histogram takes neither weights nor a tile_size above 0");
    *exit_code = guarded([&](Engine &E) {
        run_hist_add(E, name, on_device, (HistWord *)d_hist, weighted != 0, frames, width, height, pixels, channels, alpha_threshold, weights, tile_size);
    });
}

void patolette_amd_hist_add_u8(void *d_hist, int weighted, size_t frames, size_t width, size_t height, const unsigned char *pixels, int channels,
                               int alpha_threshold, const double *weights, double tile_size, int *exit_code) {
    hist_add_entry(false, d_hist, weighted, frames, width, height, pixels, channels, alpha_threshold, weights, tile_size, exit_code);
}

void patolette_amd_hist_add_u8_device(void *d_hist, int weighted, size_t frames, size_t width, size_t height, const unsigned char *d_pixels,
                                      int channels, int alpha_threshold, const double *d_weights, double tile_size, int *exit_code) {
    hist_add_entry(true, d_hist, weighted, frames, width, height, d_pixels, channels, alpha_threshold, d_weights, tile_size, exit_code);
}

int patolette_amd_hist_merge(void *d_hist, const void *d_other, int weighted) {
    int code = 0;
    const ArgCheck arg{"patolette_amd_hist_merge", &code};
    if (!d_hist || !d_other) { arg.fail(-1, "no histogram"); return code; }
    if (d_hist == d_other) { arg.fail(-1, "a histogram cannot be merged into itself"); return code; }
    return guarded([&](Engine &E) { run_hist_merge(E, (HistWord *)d_hist, (const HistWord *)d_other, weighted != 0); });
}

void patolette_amd_hist_totals(const void *d_hist, int weighted, uint64_t *pixels, uint64_t *colors, int *exit_code) {
    if (!d_hist) return (void)ArgCheck{"patolette_amd_hist_totals", exit_code}.fail(-1, "no histogram");
    *exit_code = guarded([&](Engine &E) { run_hist_totals(E, (const HistWord *)d_hist, weighted != 0, pixels, colors); });
}

void patolette_amd_hist_export(const void *d_hist, int weighted, size_t capacity, unsigned char *colors, uint64_t *counts, double *weights,
                               int *exit_code) {
    if (!d_hist) return (void)ArgCheck{"patolette_amd_hist_export", exit_code}.fail(-1, "no histogram");
    *exit_code = guarded([&](Engine &E) { run_hist_export(E, (const HistWord *)d_hist, weighted != 0, capacity, colors, counts, weights); });
}

void patolette_amd_hist_palette(const void *d_hist, int weighted, size_t palette_size, const patolette__QuantizationOptions *options,
                                double *palette, unsigned char *palette_u8, int *exit_code) {
    const ArgCheck arg{"patolette_amd_hist_palette", exit_code};
    if (!d_hist) return (void)arg.fail(-1, "no histogram");
    if (!options) return (void)arg.fail(-1, "no options");
    *exit_code = validate(1, 1, palette_size);
    if (*exit_code != 0) return;
    *exit_code = guarded([&](Engine &E) { run_hist_palette(E, (const HistWord *)d_hist, weighted != 0, palette_size, options, palette, palette_u8); });
}

// Independent images: up to six are in flight at once, each on its own engine (HIP stream + workspace) driven by
// its own host thread, so the upload / host-side split-loop work of one image overlaps the kernels of another.
// Engines are pooled per device and reused across calls.

// run item(E, i) for i in [0, count) on pooled engines, `workers` of them in flight
static void batch_run(size_t count, size_t width, size_t height, const patolette__QuantizationOptions *options, int *exit_codes,
                      const std::function<void(Engine &, size_t)> &item) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { for (size_t i = 0; i < count; i++) exit_codes[i] = -1; return; }
    if (engine().device >= 0) device = engine().device;
    // Images in flight: six keep the GPU busy through the host round trips between an image's split rounds (device-resident
    // 4096^2 images, one MI355X: 2960 Mpx/s one at a time, 3330 / 3410 / 3740 / 3990 / 3880 with 2 / 3 / 4 / 6 / 8 in flight).  The
    // Riemersma dither fills the GPU by itself since it is cut into runs (map.hip DitherSeg), so dithered batches keep the same
    // number in flight.  Bounded by the free HBM: an engine's workspace is ~170 bytes per pixel.
    const size_t base_flight = getenv("PAMD_BATCH_FLIGHT") ? std::max<size_t>(1, (size_t)atoll(getenv("PAMD_BATCH_FLIGHT"))) : 6;
    size_t workers = std::min<size_t>(count, base_flight);
    if (count > 1) {
        size_t free_b = 0, total_b = 0;
        (void)hipSetDevice(device);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t per_engine = (size_t)(170.0 * (double)width * (double)height) + ((size_t)64 << 20);
            size_t idle = 0;                                     // pooled engines whose workspace already covers this image size
            {
                std::lock_guard<std::mutex> lk(g_pool_mu);
                for (Engine *e : g_pool) if (e->device == device && e->cvt.cap >= 3 * width * height) idle++;
            }
            const size_t fit = idle + free_b / 2 / per_engine;   // leave half of what is free alone
            workers = std::min<size_t>(count, std::max<size_t>(1, std::min<size_t>(fit, base_flight)));
        }
    }
    std::atomic<size_t> next{0};
    const bool invariant = invariant_default();
    auto work = [&]() {
        Engine *E = nullptr;
        try {
            (void)hipSetDevice(device);
            E = pool_acquire(device, invariant);                 // the CALLER's setting (this may be a helper thread)
            E->init();
        } catch (const std::exception &ex) {
            fprintf(stderr, "patolette: %s\n", ex.what());
            for (size_t i; (i = next.fetch_add(1)) < count;) exit_codes[i] = -1;
            if (E) pool_release(E);
            return;
        }
        for (size_t i; (i = next.fetch_add(1)) < count;) {
            try {
                item(*E, i);
                exit_codes[i] = 0;
            } catch (const CodeError &ex) {
                exit_codes[i] = ex.code;
            } catch (const std::exception &ex) {
                fprintf(stderr, "patolette: %s\n", ex.what());
                exit_codes[i] = -1;
            }
        }
        pool_release(E);
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < workers; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

static void batch_impl(bool rows, size_t count, size_t width, size_t height, const double *const *data, const double *const *weights,
                       double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *const *palettes,
                       size_t *const *palette_maps, int *exit_codes) {
    const int v = validate(width, height, palette_size);
    if (v != 0) { for (size_t i = 0; i < count; i++) exit_codes[i] = v; return; }
    batch_run(count, width, height, options, exit_codes, [&](Engine &E, size_t i) {
        run_host(E, width, height, data[i], weights ? weights[i] : nullptr, tile_size, palette_size, options, palettes[i],
                 palette_maps ? palette_maps[i] : nullptr, rows);
    });
}

void patolette_amd_batch_u8(size_t count, size_t width, size_t height, const unsigned char *const *pixels, int channels,
                            const double *const *weights, double tile_size, size_t palette_size,
                            const patolette__QuantizationOptions *options, double *const *palettes, unsigned char *const *palettes_u8,
                            void *const *palette_maps, int map_elem_bytes, unsigned char *const *quantized, int *exit_codes) {
    int v = validate(width, height, palette_size);
    if (v == 0 && validate_u8(palette_size, channels, palette_maps ? (const void *)palette_maps : nullptr, map_elem_bytes) != 0)
        fail_args(&v, -1, kBadU8Args);
    if (v != 0) { for (size_t i = 0; i < count; i++) exit_codes[i] = v; return; }
    batch_run(count, width, height, options, exit_codes, [&](Engine &E, size_t i) {
        run_u8(E, width, height, pixels[i], channels, weights ? weights[i] : nullptr, tile_size, palette_size, options, palettes[i],
               palettes_u8 ? palettes_u8[i] : nullptr, palette_maps ? palette_maps[i] : nullptr, map_elem_bytes,
               quantized ? quantized[i] : nullptr, false);
    });
}

void patolette_amd_batch_dmap(size_t count, size_t width, size_t height, const void *const *images, int pixel_format,
                              const double *const *weights, double tile_size, size_t palette_size,
                              const patolette__QuantizationOptions *options, double *const *palettes, void *d_palette_maps,
                              int map_elem_bytes, int *exit_codes) {
    int v = validate(width, height, palette_size);
    if (v == 0 && pixel_format != 0 && pixel_format != 1 && pixel_format != 3 && pixel_format != 4) v = -1;
    if (v == 0 && d_palette_maps && map_elem_bytes != map_elem_for(palette_size)) fail_args(&v, -1, kBadDeviceMapElem);
    if (v != 0) { for (size_t i = 0; i < count; i++) exit_codes[i] = v; return; }
    const size_t N = width * height;
    batch_run(count, width, height, options, exit_codes, [&](Engine &E, size_t i) {
        void *d_map = d_palette_maps ? (void *)((unsigned char *)d_palette_maps + i * N * (size_t)map_elem_bytes) : nullptr;
        const double *w = weights ? weights[i] : nullptr;
        if (pixel_format <= 1)
            run_host(E, width, height, (const double *)images[i], w, tile_size, palette_size, options, palettes[i], nullptr,
                     pixel_format == 1, d_map);
        else
            run_u8(E, width, height, (const unsigned char *)images[i], pixel_format, w, tile_size, palette_size, options, palettes[i],
                   nullptr, d_map, map_elem_bytes, nullptr, false, true);
    });
}

int patolette_amd_principal_axis(const double cov6[6], double axis[3]) {
    return hm::principal_axis(cov6, axis) ? 0 : -1;
}
int patolette_amd_subsample_indices(size_t n, size_t take, int32_t *out) {
    if (!out || take > n) return -1;
    hm::rand_perm_prefix(n, take, 1234u, out);                              // host code: needs no device
    return 0;
}
int patolette_amd_eigen_sym3_device(const double *a_colmajor, size_t count, double *w, double *z, int *info) {
    try {
        if (!count) return 0;
        DevBuf<double> da, dw, dz; DevBuf<int> di;
        da.reserve(9 * count); dw.reserve(3 * count); dz.reserve(9 * count); di.reserve(count);
        HIP_CHECK(hipMemcpy(da.p, a_colmajor, 9 * count * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_eigen_batch, (unsigned)((count + 63) / 64), 64, 0, nullptr, da.p, count, dw.p, dz.p, di.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(w, dw.p, 3 * count * sizeof(double), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(z, dz.p, 9 * count * sizeof(double), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(info, di.p, count * sizeof(int), hipMemcpyDeviceToHost));
        return 0;
    } catch (const std::exception &e) { engine().last_error = e.what(); return -1; }
}
// The global quantiser from a moment table the caller gives, on either route (tests only).  Scratch buffers throughout; the DP state
// starts as 0xFF bytes, so that an entry a route reads without having written it cannot pass for the reference's initial value.
int patolette_amd_debug_gq_table(const double *table, const uint32_t *counts, int weighted, size_t palette_size, int route, int *kbase, int *error,
                                 int *cuts, unsigned char *bucket_table, uint64_t *begin, uint64_t *n, double *sw, double *mean,
                                 uint64_t *prefix_w0, double *prefix, int *cut_table) {
    if (!table || !counts || !kbase || !error || !cuts || !bucket_table || !begin || !n || !sw || !mean || palette_size < 1 || (route != 0 && route != 1))
        return -1;
    return guarded([&](Engine &E) -> int {
        hipStream_t s = E.stream;
        const size_t hs = (size_t)(weighted ? 14 : 10) * 2 * kBuckets;
        DevBuf<double> d_hist; DevBuf<unsigned int> d_hcount; DevBuf<GqDpDev> d_g;
        d_hist.reserve(hs); d_hcount.reserve(kBuckets); d_g.reserve(1);
        HIP_CHECK(hipMemcpyAsync(d_hist.p, table, hs * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_hcount.p, counts, kBuckets * sizeof(unsigned int), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d_g.p, 0xFF, sizeof(GqDpDev), s));
        auto h_g = std::make_unique<GqDpDev>();
        *kbase = 0; *error = 0;
        for (int j = 0; j < 14; j++) cuts[j] = 0;
        for (int j = 0; j < kGqMaxK; j++) { begin[j] = 0; n[j] = 0; sw[j] = 0; for (int q = 0; q < 3; q++) mean[3 * j + q] = 0; }
        std::memset(bucket_table, 0, kBuckets);
        if (prefix_w0) std::memset(prefix_w0, 0, 2 * (kBuckets + 1) * sizeof(uint64_t));
        if (prefix) std::memset(prefix, 0, 14 * (kBuckets + 1) * sizeof(double));
        if (route == 0) {
            launch_gq_dp(d_hist.p, d_hcount.p, (int)std::min<size_t>(palette_size, kGqMaxK), d_g.p, s);
            HIP_CHECK(hipMemcpyAsync(h_g.get(), d_g.p, sizeof(GqDpDev), hipMemcpyDeviceToHost, s));
            E.sync();
            GqDecision D;
            auto cm = std::make_unique<hm::CellMoments>();
            const bool ok = gq_host_decide(table, counts, weighted != 0, palette_size, h_g->cut, D, cm.get());
            if (prefix_w0) for (int i = 0; i <= kBuckets; i++) { prefix_w0[i] = cm->w0[i]; prefix_w0[kBuckets + 1 + i] = h_g->w0[i]; }
            if (prefix) {                                            // rows 0..9 the host's own chains, 10..13 k_gq_prefix's (what the DP read)
                for (int r = 0; r < 3; r++) std::memcpy(prefix + (size_t)r * (kBuckets + 1), cm->w1[r], sizeof(cm->w1[r]));
                std::memcpy(prefix + (size_t)3 * (kBuckets + 1), cm->w2, sizeof(cm->w2));
                for (int q = 0; q < 6; q++) std::memcpy(prefix + (size_t)(4 + q) * (kBuckets + 1), cm->wrs[q], sizeof(cm->wrs[q]));
                for (int r = 0; r < 3; r++) std::memcpy(prefix + (size_t)(10 + r) * (kBuckets + 1), h_g->w1[r], sizeof(h_g->w1[r]));
                std::memcpy(prefix + (size_t)13 * (kBuckets + 1), h_g->w2, sizeof(h_g->w2));
            }
            if (cut_table) std::memcpy(cut_table, h_g->cut, sizeof(h_g->cut));
            if (!ok) { *error = 1; return 0; }
            *kbase = D.kbase;
            for (int j = 0; j <= D.kbase && j < 14; j++) cuts[j] = (int)D.cuts[j];
            std::memcpy(bucket_table, D.lut.data(), kBuckets);
            for (int j = 0; j < D.kbase; j++) {
                begin[j] = D.base[j].begin; n[j] = D.base[j].n; sw[j] = D.base[j].sw;
                for (int q = 0; q < 3; q++) mean[3 * j + q] = D.base[j].mean[q];
            }
            return 0;
        }
        DevBuf<NodeDev> d_nodes; DevBuf<unsigned char> d_lut; DevBuf<GqOut> d_out; DevBuf<GqPrefixes> d_pre;
        d_nodes.reserve(1 + kGqMaxK); d_lut.reserve(kBuckets); d_out.reserve(2); d_pre.reserve(1);
        HIP_CHECK(hipMemsetAsync(d_nodes.p, 0, (1 + kGqMaxK) * sizeof(NodeDev), s));
        HIP_CHECK(hipMemsetAsync(d_out.p, 0, 2 * sizeof(GqOut), s));
        hipLaunchKernelGGL(k_gq_control, 1, 1024, 0, s, (const double *)d_hist.p, (const unsigned int *)d_hcount.p, d_g.p, (int)std::min<size_t>(palette_size, (size_t)1 << 30),
                           weighted ? 1 : 0, d_nodes.p, 1, d_lut.p, d_out.p, d_out.p + 1, (prefix_w0 || prefix) ? d_pre.p : (GqPrefixes *)nullptr);
        HIP_CHECK(hipGetLastError());
        GqOut o;
        std::vector<NodeDev> h_nodes(1 + kGqMaxK);
        auto h_pre = std::make_unique<GqPrefixes>();
        HIP_CHECK(hipMemcpyAsync(&o, d_out.p, sizeof(GqOut), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_nodes.data(), d_nodes.p, (1 + kGqMaxK) * sizeof(NodeDev), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(bucket_table, d_lut.p, kBuckets, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_g.get(), d_g.p, sizeof(GqDpDev), hipMemcpyDeviceToHost, s));
        if (prefix_w0 || prefix) HIP_CHECK(hipMemcpyAsync(h_pre.get(), d_pre.p, sizeof(GqPrefixes), hipMemcpyDeviceToHost, s));
        E.sync();
        if (prefix_w0) std::memcpy(prefix_w0, h_pre->w0, sizeof(h_pre->w0));
        if (prefix) std::memcpy(prefix, h_pre->t, sizeof(h_pre->t));
        if (cut_table) std::memcpy(cut_table, h_g->cut, sizeof(h_g->cut));
        if (o.error) { *error = 1; std::memset(bucket_table, 0, kBuckets); return 0; }
        *kbase = o.kbase;
        for (int j = 0; j <= o.kbase && j < 14; j++) cuts[j] = o.cuts[j];
        for (int j = 0; j < o.kbase; j++) {
            const NodeDev &c = h_nodes[1 + j];
            begin[j] = c.begin; n[j] = c.n; sw[j] = c.sw;
            for (int q = 0; q < 3; q++) mean[3 * j + q] = c.mean[q];
        }
        return 0;
    });
}
int patolette_amd_eigen_sym3(const double a_colmajor[9], double w[3], double z[9]) {
    std::memcpy(z, a_colmajor, 9 * sizeof(double));
    return hm::eigen_sym3(z, w);                                           // LAPACK info: 0 = converged
}

void patolette_amd_batch(size_t count, size_t width, size_t height, const double *const *data, const double *const *weights,
                         double tile_size, size_t palette_size, const patolette__QuantizationOptions *options, double *const *palettes,
                         size_t *const *palette_maps, int *exit_codes) {
    batch_impl(false, count, width, height, data, weights, tile_size, palette_size, options, palettes, palette_maps, exit_codes);
}
void patolette_amd_batch_rows(size_t count, size_t width, size_t height, const double *const *rows, const double *const *weights,
                              double tile_size, size_t palette_size, const patolette__QuantizationOptions *options,
                              double *const *palettes, size_t *const *palette_maps, int *exit_codes) {
    batch_impl(true, count, width, height, rows, weights, tile_size, palette_size, options, palettes, palette_maps, exit_codes);
}

static int pow_entry(const double *x, double y, double *out, size_t n, int mode) {
    return guarded([&](Engine &E) -> int {
        if (n == 0) return 0;
        if (mode < 0 || mode > 2) return -1;
        E.src.reserve(2 * n);
        HIP_CHECK(hipMemcpyAsync(E.src.p, x, n * sizeof(double), hipMemcpyHostToDevice, E.stream));
        launch_pow(E.src.p, y, E.src.p + n, n, E.stream, mode);
        HIP_CHECK(hipMemcpyAsync(out, E.src.p + n, n * sizeof(double), hipMemcpyDeviceToHost, E.stream));
        E.sync();
        return 0;
    });
}
int patolette_amd_pow(const double *x, double y, double *out, size_t n) { return pow_entry(x, y, out, n, 2); }
int patolette_amd_debug_pow(const double *x, double y, double *out, size_t n, int mode) { return pow_entry(x, y, out, n, mode); }

int patolette_amd_debug_convert(int which, const double *planar, const unsigned char *bytes, int channels, double *out, size_t n, int general) {
    return guarded([&](Engine &E) -> int {
        if (n == 0) return 0;
        if ((planar == nullptr) == (bytes == nullptr) || (bytes && (channels < 3 || channels > 4))) return -1;
        E.src.reserve(3 * n); E.aux.reserve(3 * n);
        if (planar) {
            HIP_CHECK(hipMemcpy(E.src.p, planar, 3 * n * sizeof(double), hipMemcpyHostToDevice));
            launch_convert(which, E.src.p, E.aux.p, n, nullptr, E.stream, BinK{0.0, 0.0}, BinK{0.0, 0.0}, 0, n, true, general != 0);
        } else {
            HIP_CHECK(hipMemcpy(E.src.p, bytes, n * (size_t)channels, hipMemcpyHostToDevice));
            launch_convert_u8(which, reinterpret_cast<const unsigned char *>(E.src.p), channels, E.aux.p, n, nullptr, E.stream, BinK{0.0, 0.0},
                              BinK{0.0, 0.0}, 0, n, true, general != 0);
        }
        E.sync();
        HIP_CHECK(hipMemcpy(out, E.aux.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    });
}

int patolette_amd_convert(int which, double *planar, size_t n) {
    return guarded([&](Engine &E) -> int {
        if (n == 0) return 0;
        E.src.reserve(3 * n); E.aux.reserve(3 * n);
        HIP_CHECK(hipMemcpy(E.src.p, planar, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        launch_convert(which, E.src.p, E.aux.p, n, nullptr, E.stream);
        E.sync();
        HIP_CHECK(hipMemcpy(planar, E.aux.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    });
}

int patolette_amd_quantize_clusters(const double *colors, const double *weights, size_t n, size_t K, double *centers, size_t *n_clusters) {
    return guarded([&](Engine &E) -> int {
        if (n == 0 || K == 0) return -1;
        const bool weighted = weights != nullptr;
        E.src.reserve(3 * n);
        E.cvt.reserve((weighted ? 4 : 3) * n);
        E.cstats.reserve(1);
        HIP_CHECK(hipMemcpy(E.src.p, colors, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        launch_convert(PAMD_COPY, E.src.p, E.cvt.p, n, E.cstats.p, E.stream);
        if (weighted) {
            HIP_CHECK(hipMemcpyAsync(E.cvt.p + 3 * n, weights, n * sizeof(double), hipMemcpyHostToDevice, E.stream));
            launch_weight_stats(E.cvt.p + 3 * n, n, E.cstats.p, E.stream);
        }
        Bounds b = read_bounds(E, weighted);
        E.stats = patolette_amd__Stats{};
        std::vector<double> pal;
        size_t len = 0;
        if (quantize_clusters(E, n, K, weighted, b, pal, len) != 0) return -1;
        for (size_t j = 0; j < 3 * K; j++) centers[j] = NAN;
        for (int j = 0; j < 3; j++) for (size_t i = 0; i < len; i++) centers[(size_t)j * K + i] = pal[(size_t)j * len + i];
        *n_clusters = len;
        return 0;
    });
}

int patolette_amd_kmeans_refine(const double *colors, const double *weights, size_t n, double *centers_io, size_t k, int niter, size_t max_samples) {
    return guarded([&](Engine &E) -> int {
        const bool weighted = weights != nullptr;
        E.cvt.reserve((weighted ? 4 : 3) * n);
        HIP_CHECK(hipMemcpy(E.cvt.p, colors, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        if (weighted) HIP_CHECK(hipMemcpy(E.cvt.p + 3 * n, weights, n * sizeof(double), hipMemcpyHostToDevice));
        std::vector<double> pal(centers_io, centers_io + 3 * k);
        bool nonfinite = false;                                     // Clustering.cpp:295-304 over every colour value as f32
        double bx = 0, bw = 1, min_w = 0;
        for (size_t i = 0; i < 3 * n && !nonfinite; i++) { nonfinite = !(std::fabs(colors[i]) < 0x1.ffffffp127); bx = std::max(bx, std::fabs(colors[i])); }
        bool bad_w = false;                                         // as f32: the finite domain of kmeans_refine
        if (!nonfinite && weighted) for (size_t i = 0; i < n; i++) {
            const float wf = (float)weights[i];
            bw = std::max(bw, std::fabs(weights[i]));
            if (!(wf >= 0.f) || !std::isfinite(wf)) bad_w = true;
            else if (wf > 0.f && (min_w == 0 || (double)wf < min_w)) min_w = (double)wf;
        }
        kmeans_refine(E, n, weighted, pal, k, niter, max_samples, nonfinite, 0, bx, bw, min_w, bad_w);
        std::memcpy(centers_io, pal.data(), 3 * k * sizeof(double));
        return 0;
    });
}

int patolette_amd_debug_km_route(void) { return holder().e ? holder().e->km.route : 0; }

int patolette_amd_debug_nn_route(int route) { return nn_debug_route(route); }

int patolette_amd_debug_nn_map_elem(const double *colors, size_t n, const double *palette, size_t k, int map_elem_bytes, int misalign, void *map) {
    return guarded([&](Engine &E) -> int {
        const int eb = map_elem_bytes;
        if ((eb != 1 && eb != 4 && eb != 8) || (eb == 1 && k > 256) || k == 0 || (misalign != 0 && (misalign != 1 || eb != 1)))
            throw HipError("patolette_amd_debug_nn_map_elem: elements of 1 (up to 256 rows), 4 or 8 bytes; misalign 0, or 1 with 1-byte elements");
        if (n == 0) return 0;
        E.src.reserve(3 * n); E.dpal.reserve(3 * k); E.dmap.reserve(n * (size_t)eb + 1);
        HIP_CHECK(hipMemcpy(E.src.p, colors, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(E.dpal.p, palette, 3 * k * sizeof(double), hipMemcpyHostToDevice));
        launch_nn_map(E.src.p, n, n, E.dpal.p, (int)k, E.dmap.p + misalign, eb, nullptr, nullptr, E.nn, E.stream);
        E.sync();
        HIP_CHECK(hipMemcpy(map, E.dmap.p + misalign, n * (size_t)eb, hipMemcpyDeviceToHost));
        return 0;
    });
}

int patolette_amd_nn_map(const double *colors, size_t n, const double *palette, size_t k, size_t *map) {
    return guarded([&](Engine &E) -> int {
        if (n == 0) return 0;
        E.src.reserve(3 * n); E.dpal.reserve(3 * k); E.dmap.reserve(n * 4);
        HIP_CHECK(hipMemcpy(E.src.p, colors, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(E.dpal.p, palette, 3 * k * sizeof(double), hipMemcpyHostToDevice));
        launch_nn_map(E.src.p, n, n, E.dpal.p, (int)k, E.dmap.p, 4, nullptr, nullptr, E.nn, E.stream);
        E.sync();
        download_map(E.dmap.p, 4, n, map, 8);
        return 0;
    });
}

int patolette_amd_dither(const double *colors, size_t width, size_t height, const double *palette, size_t k, size_t *map) {
    return guarded([&](Engine &E) -> int {
        const size_t n = width * height;
        if (n == 0) return 0;
        E.src.reserve(3 * n); E.dpal.reserve(3 * k); E.dmap.reserve(n * 4);
        HIP_CHECK(hipMemcpy(E.src.p, colors, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(E.dpal.p, palette, 3 * k * sizeof(double), hipMemcpyHostToDevice));
        DitherJob job;
        job.planes = E.src.p; job.plane_stride = n; job.which = PAMD_COPY;
        job.width = width; job.height = height;
        job.d_pal = E.dpal.p; job.h_pal = palette; job.k = (int)k;
        job.out = E.dmap.p; job.elem_bytes = 4;
        launch_dither(job, E.nn, E.stream);
        E.stats = patolette_amd__Stats{};                           // (a call of its own: nothing of the one before it stays)
        add_dither_stats(E);
        E.sync();
        if (map_touched(true, width, height)) download_map(E.dmap.p, 4, n, map, 8);
        return 0;
    });
}

int patolette_amd_debug_fault(int which) { return g_debug_fault.exchange(which); }
int patolette_amd_debug_workspace(int flags) { return g_debug_ws.exchange(flags & (kWsPoison | kWsCount | kWsLog)); }
unsigned long long patolette_amd_debug_late_growths(void) { return g_late_growths.load(); }
int patolette_amd_set_split_loop(int mode) { return g_lq_device.exchange(mode < 0 || mode > 2 ? 2 : mode); }
int patolette_amd_set_global_quantiser(int on_device) { return g_gq_device.exchange(on_device ? 1 : 0); }
void patolette_amd_dither_config(int segments, int warm) { dither_config(segments, warm); }
void patolette_amd_dither_layout(int lanes) { dither_layout(lanes); }
int patolette_amd_debug_dither_solo_cap(int cap) { return dither_solo_cap(cap); }
int patolette_amd_debug_dither_stall_passes(int n) { return dither_stall_passes(n); }
int patolette_amd_dither_layout_in_use(size_t width, size_t height, size_t k) { return dither_lane_layout(width, height, (int)k) ? 1 : 0; }
int patolette_amd_debug_dither_lane_tables(double *geom30, float *amb3, unsigned char *tables, size_t capacity) {
    return guarded([&](Engine &E) -> int { return dither_lane_tables(E.nn, geom30, amb3, tables, capacity, E.stream); });
}
void patolette_amd_last_stats(patolette_amd__Stats *out) { *out = engine().stats; }
size_t patolette_amd_last_split_trace(patolette_amd__SplitTrace *hdr, patolette_amd__SplitRecord *recs, size_t capacity) {
    Engine &E = engine();
    try { materialise_trace(E); } catch (const std::exception &e) { E.last_error = e.what(); E.trace.clear(); }
    if (hdr) *hdr = E.trace_hdr;
    if (recs) std::memcpy(recs, E.trace.data(), sizeof *recs * std::min(capacity, E.trace.size()));
    return E.trace.size();
}
size_t patolette_amd_last_cluster_centers(double *out, size_t capacity_rows) {
    Engine &E = engine();
    const size_t len = E.cluster_centers.size() / 3;
    if (out && len <= capacity_rows)
        for (int j = 0; j < 3; j++) for (size_t i = 0; i < len; i++) out[(size_t)j * capacity_rows + i] = E.cluster_centers[(size_t)j * len + i];
    return len;
}
size_t patolette_amd_last_map_palette(double *out, size_t capacity_rows) {
    const std::vector<double> &mp = engine().map_palette;
    const size_t len = mp.size() / 3;
    if (out && capacity_rows >= len)
        for (int j = 0; j < 3; j++) for (size_t i = 0; i < len; i++) out[(size_t)j * capacity_rows + i] = mp[(size_t)j * len + i];
    return len;
}

void patolette_amd_profile_enable(int on) {
    KernelTimer &t = ktimer();
    if (engine().stream) (void)hipStreamSynchronize(engine().stream);
    t.reset();
    t.enabled = on != 0;
}
void patolette_amd_profile_only(const char *kernel_name) { ktimer().only = kernel_name ? kernel_name : ""; ktimer().only_seen = 0; }
void patolette_amd_profile_sample(int period) { ktimer().sample_period = period > 1 ? (unsigned)period : 1u; }
int patolette_amd_profile_count(void) { return (int)ktimer().names.size(); }
int patolette_amd_profile_get(int i, char *name64, double *total_ms, size_t *launches, double *total_bytes) {
    KernelTimer &t = ktimer();
    if (i < 0 || i >= (int)t.names.size()) return -1;
    snprintf(name64, 64, "%s", t.names[i].c_str());
    *total_ms = t.total_ms[i];
    *launches = t.launches[i];
    *total_bytes = t.total_bytes[i];
    return 0;
}

}  // extern "C"
