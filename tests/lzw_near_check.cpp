// lzw_near_check.cpp -- the lossy LZW coder's table rules (csrc/lzw_near.h) as a stand-alone program, for a sanitizer build: the
// check of a table at every minimum code size and the builder over palettes of 1 .. 256 rows, each compared with a restatement of the
// documented rule, in heap buffers of exactly the documented sizes (4096 bytes of table, of which the check may read 16 << m only).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lzw_near.h"

using namespace pamd;

namespace {
unsigned long long g_state = 88172645463325252ull;
unsigned rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (unsigned)(g_state >> 11); }
bool fail(const char *what, long a = 0, long b = 0) { fprintf(stderr, "lzw_near_check: %s (%ld, %ld)\n", what, a, b); return false; }

// the check reads the rows below 2^m and, of each, the count and that many bytes: the buffer ends there
bool check_rules() {
    long checked = 0;
    for (int m = 2; m <= 8; m++) {
        const size_t rows = (size_t)1 << m, bytes = kNearRow * rows;
        for (int round = 0; round < 200; round++) {
            std::unique_ptr<unsigned char[]> t(new unsigned char[bytes]);
            for (size_t s = 0; s < rows; s++) {
                t[kNearRow * s] = (unsigned char)(rnd() % 16);
                for (size_t j = 1; j < kNearRow; j++) t[kNearRow * s + j] = (unsigned char)(j <= t[kNearRow * s] ? rnd() % rows : 255);   // behind the count: not read
            }
            if (near_check(t.get(), m) != kNearOk) return fail("a good table was refused", m, round);
            const size_t s = rnd() % rows;
            unsigned char *row = t.get() + kNearRow * s;
            const unsigned char count = row[0];
            row[0] = (unsigned char)(16 + rnd() % 240);
            if (near_check(t.get(), m) != kNearCount) return fail("a count above 15 passed", m, round);
            row[0] = count;
            if (count > 0 && m < 8) {
                const size_t j = 1 + rnd() % count;
                row[j] = (unsigned char)(rows + rnd() % (256 - rows));
                if (near_check(t.get(), m) != kNearCandidate) return fail("a candidate at or above 2^m passed", m, round);
            }
            checked++;
        }
    }
    printf("lzw_near_check: %ld tables checked\n", checked);
    return true;
}

bool build_rules() {
    long built = 0;
    for (size_t k = 1; k <= 256; k += (k < 20 ? 1 : 59)) {
        for (int round = 0; round < 6; round++) {
            std::vector<double> pal(3 * k);
            for (size_t i = 0; i < k; i++)
                for (int c = 0; c < 3; c++) pal[(size_t)c * k + i] = (i % 3 == 2 && round % 2) ? pal[(size_t)c * k + i - 2] : (rnd() % 256) / 255.0;   // duplicates
            const int transparent = round < 2 ? -1 : (int)(rnd() % 256);
            const double tolerance = round == 0 ? 0.0 : 0.02 * (1 << round);
            const size_t most = round == 1 ? 0 : (round == 2 ? 1 : 15);
            std::unique_ptr<unsigned char[]> out(new unsigned char[kNearRows * kNearRow]);
            std::memset(out.get(), 0xEE, kNearRows * kNearRow);
            near_build(pal, k, transparent, tolerance, most, out.get());
            if (near_check(out.get(), 8) != kNearOk) return fail("the builder's table fails its own check", (long)k, round);
            std::vector<double> lab = pal;
            for (size_t i = 0; i < k; i++) {
                double c[3] = {lab[i], lab[k + i], lab[2 * k + i]};
                hm::color::srgb_to_ictcp(c);
                lab[i] = c[0]; lab[k + i] = c[1]; lab[2 * k + i] = c[2];
            }
            auto D = [&](size_t a, size_t b) {
                const double d0 = lab[a] - lab[b], d1 = lab[k + a] - lab[k + b], d2 = lab[2 * k + a] - lab[2 * k + b];
                return (d0 * d0 + d1 * d1) + d2 * d2;
            };
            for (size_t s = 0; s < kNearRows; s++) {
                const unsigned char *row = out.get() + kNearRow * s;
                for (size_t j = row[0] + 1; j < kNearRow; j++) if (row[j] != 0) return fail("a byte behind the count is not 0", (long)s, (long)j);
                if (s >= k || (int)s == transparent) { if (row[0] != 0) return fail("an unused or transparent row has candidates", (long)s, row[0]); continue; }
                size_t within = 0;
                for (size_t e = 0; e < k; e++) within += e != s && (int)e != transparent && D(s, e) <= tolerance * tolerance;
                if (row[0] != (within < most ? within : most)) return fail("a count", (long)s, row[0]);
                for (size_t j = 1; j <= row[0]; j++) {
                    const size_t e = row[j];
                    if (e >= k || e == s || (int)e == transparent || D(s, e) > tolerance * tolerance) return fail("a candidate that may not be one", (long)s, (long)e);
                    if (j > 1) {
                        const size_t b = row[j - 1];
                        if (D(s, b) > D(s, e) || (D(s, b) == D(s, e) && b >= e)) return fail("the order", (long)s, (long)j);
                    }
                }
                // nothing nearer was left out: every row ahead of the last candidate in (D, index) order is listed
                if (row[0] == most && most > 0 && within > most) {
                    const size_t last = row[row[0]];
                    size_t ahead = 0;
                    for (size_t e = 0; e < k; e++)
                        ahead += e != s && (int)e != transparent && (D(s, e) < D(s, last) || (D(s, e) == D(s, last) && e < last));
                    if (ahead != most - 1) return fail("a nearer row was left out", (long)s, (long)ahead);
                }
            }
            built++;
        }
    }
    printf("lzw_near_check: %ld tables built and found to follow the rule\n", built);
    return true;
}
}  // namespace

int main() { return check_rules() && build_rules() ? 0 : 1; }
