// dither_host_check.cpp -- the dither drivers' host arithmetic (csrc/dither_host.h) over cases read from a file, results printed as
// integers and hex floats, one line per case.  Host code only: test_dither_host.py writes the cases, builds this with
// -fsanitize=address,undefined and compares the lines with tests/dither_ref.py.  The palette of a case sits in a heap block of
// exactly 3 k doubles, so a read past it is caught.
//   geom K NPIX v[3 K]      -> lo[3] hi[3] inv[3] cw[3] G per grid (three grids), amb amb_p amb_x, then the weighted palette
//   lanecut SEGMENTS WARM CUS NPIX NFRAME FRAMES -> S Lmax fruns warm
//   wavecut SEGMENTS WARM CUS NPIX WIDTH HEIGHT  -> S warm
//   rule SEGMENTS LANES NPIX K -> 0 / 1        possible FRAMES N K -> 0 / 1
//   weights -> the sixteen queue weights         stall N n[N] -> the stall count after every pass
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "dither_host.h"

using namespace pamd;

namespace {
FILE *in;
bool word(char *buf) { return fscanf(in, "%63s", buf) == 1; }
long long integer() { char b[64]; if (!word(b)) exit(2); return strtoll(b, nullptr, 10); }
double real() { char b[64]; if (!word(b)) exit(2); return strtod(b, nullptr); }   // (hex floats, inf, nan)

void geom() {
    const int k = (int)integer();
    const size_t npix = (size_t)integer();
    std::unique_ptr<double[]> pal(new double[3 * (size_t)k]);
    for (size_t i = 0; i < 3 * (size_t)k; i++) pal[i] = real();
    const DitherLaneGeometry a = dither_lane_geometry(pal.get(), k, npix);
    if (a.wp.size() != 3 * (size_t)k) exit(3);
    for (int lv = 0; lv < 3; lv++) {
        const NNGrid &g = lv == 0 ? a.g : a.gw[lv - 1];
        const double *hi = lv == 0 ? a.hi : a.whi[lv - 1];
        for (int c = 0; c < 3; c++) printf("%a ", g.lo[c]);
        for (int c = 0; c < 3; c++) printf("%a ", hi[c]);
        for (int c = 0; c < 3; c++) printf("%a ", g.inv[c]);
        for (int c = 0; c < 3; c++) printf("%a ", g.cw[c]);
        printf("%d ", g.G);
    }
    printf("%a %a %a", (double)a.amb, (double)a.amb_p, (double)a.amb_x);
    for (double v : a.wp) printf(" %a", v);
    printf("\n");
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) return 2;
    char op[64];
    long cases = 0;
    while (word(op)) {
        cases++;
        if (!strcmp(op, "geom")) geom();
        else if (!strcmp(op, "lanecut")) {
            const int segments = (int)integer(), warm = (int)integer(), cus = (int)integer();
            const size_t npix = (size_t)integer(), nframe = (size_t)integer(), frames = (size_t)integer();
            const DitherLaneCut c = dither_lane_cut(segments, warm, cus, npix, nframe, frames);
            printf("%zu %u %u %u\n", c.S, c.Lmax, c.fruns, c.warm);
        } else if (!strcmp(op, "wavecut")) {
            DitherConfig cfg;
            cfg.segments = (int)integer(); cfg.warm = (int)integer();
            const int cus = (int)integer();
            const size_t npix = (size_t)integer(), width = (size_t)integer(), height = (size_t)integer();
            const DitherWaveCut c = dither_wave_cut(cfg, cus, npix, width, height);
            printf("%zu %u\n", c.S, c.warm);
        } else if (!strcmp(op, "rule")) {
            DitherConfig cfg;
            cfg.segments = (int)integer(); cfg.lanes = (int)integer();
            const size_t npix = (size_t)integer();
            printf("%d\n", dither_lane_rule(cfg, npix, (int)integer()) ? 1 : 0);
        } else if (!strcmp(op, "possible")) {
            const size_t frames = (size_t)integer(), n = (size_t)integer();
            printf("%d\n", dither_lanes_possible(frames, n, (int)integer()) ? 1 : 0);
        } else if (!strcmp(op, "weights")) {
            const DitherWeights w = dither_weights();
            for (int i = 0; i < 16; i++) printf("%a%c", w.w[i], i == 15 ? '\n' : ' ');
        } else if (!strcmp(op, "stall")) {
            DitherStall st;
            const long n = (long)integer();
            for (long i = 0; i < n; i++) printf("%d%c", st.step((unsigned)integer()), i == n - 1 ? '\n' : ' ');
            st.reset();
            if (st.step(0) != 0) return 3;
        } else return 2;
    }
    fclose(in);
    fprintf(stderr, "dither_host_check: %ld cases\n", cases);
    return 0;
}
