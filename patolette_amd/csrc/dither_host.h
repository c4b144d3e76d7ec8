// dither_host.h -- the host arithmetic of the Riemersma dither's drivers (map.hip): the queue weights, what the lane walk can take, the
// layout rule, the two cuts of the curve into runs, the lane layout's search geometry with the margins of its f32 first pass, and
// the stall rule of the two verification loops: each once, as plain functions of their arguments (the knob snapshot and the number
// of compute units are passed in).  Host code only (no HIP header): tests/dither_host_check.cpp runs it under sanitizers and
// tests/test_dither_host.py holds it to tests/dither_ref.py bit for bit.  The plain structs the kernels take by value and the
// host fills here (NNGrid, DitherWeights) live here too.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace pamd {

struct NNGrid {
    double lo[3], cw[3], inv[3];             // cell (i,j,k) spans lo + i*cw .. lo + (i+1)*cw
    int G;
};

struct DitherWeights { double w[16]; };

constexpr double kRw = 0.51254268114958, kGw = 0.8234075540095561, kBw = 0.2435159132377184;   // riemersma.c:38-42

struct DitherConfig { int segments = 0, warm = -1, lanes = -1; };    // 0 / -1 = chosen by launch_dither

// the sixteen weights of the error queue (riemersma.c: a geometric ramp from 1/16 to 1)
inline DitherWeights dither_weights() {
    DitherWeights wts;
    const double m = std::exp(std::log(16.0) / (16.0 - 1));
    double v = 1;
    for (int i = 0; i < 16; i++) { wts.w[i] = v / 16.0; v *= m; }
    return wts;
}
// what the lane walk itself can take, whatever the knobs say: a run of 64 pixels in every frame, one tile row per 8 runs (grid.y),
// the pruned search's palette sizes
inline bool dither_lanes_possible(size_t frames, size_t n, int k) { return frames > 0 && n >= 64 && frames <= (size_t)8 * 65535 && k >= 8 && k <= 256; }

// One lane per run where the pruned search applies (8 <= K <= 256) and the image is large: the lane layout needs ~10^5 runs of a few
// hundred pixels to fill the GPU and pays a gather, an un-permute and a repair round of fixed cost -- 2048^2: 2.3 ms against 1.6 ms
// for one wavefront per run, 4096^2: 2.7 ms, 8192^2: 4.8 against 15.6 ms.  dither_layout(1) asks for it from 65 536 pixels on.
inline bool dither_lane_rule(const DitherConfig &cfg, size_t npix, int k) {
    if (!(k >= 8 && k <= 256) || cfg.segments == 1 || cfg.lanes == 0) return false;
    return cfg.lanes > 0 ? npix >= 65536 : npix >= ((size_t)1 << 23);
}

// The lane layout's cut of npix pixels (frames * nframe of them, or a masked image's opaque ones with frames == 1) into S runs of at
// most Lmax pixels.  fruns: 0, or with frames > 1 the runs per frame -- one cut with the same number of runs in every frame, so that
// run boundaries fall on the frame starts (t(f S / frames) = f nframe exactly)
struct DitherLaneCut { size_t S; unsigned Lmax, fruns, warm; };
inline DitherLaneCut dither_lane_cut(int segments, int warm, int cus, size_t npix, size_t nframe, size_t frames) {
    DitherLaneCut c{};
    // runs: eight wavefronts of 64 per CU (two per SIMD), none shorter than 256 pixels unless asked for
    size_t S = segments > 0 ? (size_t)segments : std::min<size_t>((size_t)cus * 8 * 64, npix / 256);
    S = std::max<size_t>(1, std::min(std::min(S, npix / 64), (size_t)8 * 65535));    // (a tile row per 8 runs: grid.y)
    if (frames > 1) {                                               // the same limits, per frame (dither_lanes_possible: they leave one run at least)
        const size_t per = segments > 0 ? ((size_t)segments + frames - 1) / frames : std::min<size_t>((size_t)cus * 8 * 64, npix / 256) / frames;
        c.fruns = (unsigned)std::max<size_t>(1, std::min(std::min(per, nframe / 64), (size_t)8 * 65535 / frames));
        S = frames * c.fruns;
    }
    c.S = S; c.Lmax = (unsigned)((npix + S - 1) / S);
    // warm-up: 256 pixels.  With a repair pass that costs a tenth of a millisecond (one wavefront per listed run) the 2-6 % of the
    // boundaries that 256 steps do not settle are cheaper than 256 more steps for every run (8192^2: noise 3.65 -> 3.28 ms,
    // scene 6.0 -> 5.4, gradients + 2 % noise 5.36 -> 5.27; 384 lies between)
    c.warm = (unsigned)std::min<size_t>(warm >= 0 ? (size_t)warm : 256, npix / S);     // (the warm-up of a run is the end of its predecessor)
    return c;
}

// The lane layout's search geometry, from the palette on the host (planar (k,3), linear Rec2020) alone.
// The grid of the exact-pruning records: the weighted palette's bounding box, half its extent wider on every side -- error diffusion
// pushes queries beyond the palette's hull; what still falls outside takes the wider grids: 1.5 extents around the palette's box with
// the first grid's number of cells, 4 extents with 32 across.
struct DitherLaneGeometry {
    std::vector<double> wp;                  // the palette scaled by the float-cast weights, planar (k,3)
    NNGrid g, gw[2];
    double hi[3], whi[2][3];                 // the grids' upper corners
    float amb, amb_p, amb_x;                 // margins of the f32 first pass: inside the first grid; outside, amb_p + amb_x |x - lo|^2
};
inline DitherLaneGeometry dither_lane_geometry(const double *h_pal, int k, size_t npix) {
    DitherLaneGeometry a;
    std::vector<double> &wp = a.wp;
    wp.resize(3 * (size_t)k);
    const double fw[3] = {(double)(float)kRw, (double)(float)kGw, (double)(float)kBw};
    NNGrid &g = a.g, *gw = a.gw;
    g.G = npix >= ((size_t)1 << 20) ? 64 : 32;
    for (int c = 0; c < 3; c++) {
        double lo = INFINITY, hi = -INFINITY;
        for (int j = 0; j < k; j++) { const double v = h_pal[(size_t)c * k + j] * fw[c]; wp[(size_t)c * k + j] = v; lo = std::min(lo, v); hi = std::max(hi, v); }
        double r = hi - lo;
        if (!(r > 0) || !std::isfinite(r)) r = 0;
        const double m = 0.5 * r + 1e-3;
        g.lo[c] = lo - m;
        const double Rg = r + 2 * m;
        g.cw[c] = Rg / g.G;
        g.inv[c] = g.G / Rg;
        a.hi[c] = g.lo[c] + Rg;
        for (int lv = 0; lv < 2; lv++) {
            gw[lv].G = lv == 0 ? g.G : 32;
            const double mo = (lv == 0 ? 1.5 : 4.0) * r + (lv == 0 ? 5e-3 : 1e-2), Ro = r + 2 * mo;
            gw[lv].lo[c] = lo - mo;
            gw[lv].cw[c] = Ro / gw[lv].G;
            gw[lv].inv[c] = gw[lv].G / Ro;
            a.whi[lv][c] = gw[lv].lo[c] + Ro;
        }
    }
    // margin of the f32 first pass (the table comment above k_nn_map_mid): 2.5 E, E = 2^-24 (9 max |p - lo|^2 + 5 |hi - lo|^2) (1 + 1e-3)
    double wmax = 0.0, r2 = 0.0;
    for (int j = 0; j < k; j++) {
        double d = 0.0;
        for (int c = 0; c < 3; c++) { const double t = wp[(size_t)c * k + j] - g.lo[c]; d += t * t; }
        wmax = std::max(wmax, d);
    }
    for (int c = 0; c < 3; c++) { const double t = a.hi[c] - g.lo[c]; r2 += t * t; }
    const double M = 2.5 * 1.001 * 0x1.0p-24 * (9.0 * wmax + 5.0 * r2);
    a.amb = (float)M;
    if ((double)a.amb < M) a.amb = std::nextafter(a.amb, INFINITY);
    if (!(M < 3.0e38)) a.amb = INFINITY;
    // outside the grid the query's own |x - lo|^2 stands where |hi - lo|^2 did (evaluated in f32: 1e-6 relative, inside the 1e-3)
    const double Mp = 2.5 * 1.002 * 0x1.0p-24 * 9.0 * wmax, Mx = 2.5 * 1.002 * 0x1.0p-24 * 5.0;
    a.amb_p = std::nextafter((float)Mp, INFINITY); a.amb_x = std::nextafter((float)Mx, INFINITY);
    if (!(Mp < 3.0e38)) a.amb_p = INFINITY;
    return a;
}

// The wavefront layout's cut.  Runs: two wavefronts per SIMD fill the issue slots of the chip (one chain alone uses ~2/3 of its
// SIMD's); never shorter than the warm-up -- below that the speculative steps outnumber the useful ones.
struct DitherWaveCut { size_t S; unsigned warm; };
inline DitherWaveCut dither_wave_cut(const DitherConfig &cfg, int cus, size_t npix, size_t width, size_t height) {
    DitherWaveCut c{};
    c.warm = cfg.warm >= 0 ? (unsigned)cfg.warm : 1024u;
    size_t S = cfg.segments > 0 ? (size_t)cfg.segments : (size_t)cus * 8;
    if (cfg.segments <= 0) S = std::min(S, npix / std::max<size_t>(c.warm, 256));
    S = std::min(S, npix / 128);                                 // every run after the first has its sixteen predecessors
    if (std::max(width, height) < 16) S = 1;
    if (S < 1) S = 1;
    c.S = S;
    return c;
}

// The verification loops' stall rule: a pass that leaves `n` things to do "made no progress" when n has not dropped by an eighth (one
// at least) of the pass before; step() returns how many such passes came in a row.  reset(): after the loop has acted on a stall.
struct DitherStall {
    unsigned prev = 0xFFFFFFFFu;
    int stalled = 0;
    int step(unsigned n) {
        stalled = (prev != 0xFFFFFFFFu && n + std::max(1u, prev / 8) >= prev) ? stalled + 1 : 0;
        prev = n;
        return stalled;
    }
    void reset() { stalled = 0; prev = 0xFFFFFFFFu; }
};

}  // namespace pamd
