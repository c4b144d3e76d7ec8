// lzw_near.h -- the lossy LZW coder's table of near colours (include/patolette_amd.h: patolette_amd_gif_neighbours builds it,
// patolette_amd_gif_lzw_lossy reads it): its layout, the check the coder makes of it and its builder, each once.  Host code only (no
// HIP header), in the manner of given.h: tests/lzw_near_check.cpp runs it under sanitizers over buffers of exactly the documented sizes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

#include "given.h"
#include "host_math.h"

namespace pamd {

// 256 rows of 16 bytes: row s = the count (0 .. 15), then that many candidates for symbol s in order of preference; the rest of a
// row is not read, nor is a row at or above 2^m
constexpr size_t kNearRows = 256, kNearRow = 16, kNearMost = 15;

// What the coder reads of `near` at minimum code size m: every count must be <= 15 and every candidate below 2^m
enum NearError { kNearOk = 0, kNearCount, kNearCandidate };
inline NearError near_check(const unsigned char *near, int m) {
    const size_t rows = (size_t)1 << m;
    for (size_t s = 0; s < rows; s++) {
        const unsigned char *row = near + kNearRow * s;
        if (row[0] > kNearMost) return kNearCount;
        for (size_t j = 1; j <= row[0]; j++) if (row[j] >= rows) return kNearCandidate;
    }
    return kNearOk;
}

// The table of a palette.  pal: the k <= 256 used rows, planar (k,3) f64 sRGB (given_palette's); each goes through srgb_to_ictcp as
// run_frame_deltas prepares its palette, and D = (d0*d0 + d1*d1) + d2*d2 between two rows is the D of the frame_deltas contract
// (this file is compiled without contraction: no FMA).  Row s lists the other used rows e with D <= tolerance^2 by (D, e) ascending,
// cut to `most` <= 15; `transparent` (-1: none) is left out both as s and as e.  Rows at and above k are empty.  out: 4096 bytes, all written.
inline void near_build(std::vector<double> pal, size_t k, int transparent, double tolerance, size_t most, unsigned char *out) {
    for (size_t i = 0; i < k; i++) {
        double c[3] = {pal[i], pal[k + i], pal[2 * k + i]};
        hm::color::srgb_to_ictcp(c);
        pal[i] = c[0]; pal[k + i] = c[1]; pal[2 * k + i] = c[2];
    }
    const double t2 = tolerance * tolerance;
    std::fill(out, out + kNearRows * kNearRow, (unsigned char)0);
    std::vector<std::pair<double, size_t>> in;
    for (size_t s = 0; s < k; s++) {
        if ((long long)s == (long long)transparent) continue;
        in.clear();
        for (size_t e = 0; e < k; e++) {
            if (e == s || (long long)e == (long long)transparent) continue;
            const double d0 = pal[s] - pal[e], d1 = pal[k + s] - pal[k + e], d2 = pal[2 * k + s] - pal[2 * k + e];
            const double D = (d0 * d0 + d1 * d1) + d2 * d2;
            if (D <= t2) in.emplace_back(D, e);
        }
        std::sort(in.begin(), in.end());
        const size_t count = std::min(in.size(), most);
        unsigned char *row = out + kNearRow * s;
        row[0] = (unsigned char)count;
        for (size_t j = 0; j < count; j++) row[1 + j] = (unsigned char)in[j].second;
    }
}

}  // namespace pamd
