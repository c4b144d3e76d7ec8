// given_check.cpp -- the palette-given entries' host rules (csrc/given.h: the caller's palette, index elements in and out, the device's
// values of the transparent and skip indices, the frame deltas' slots folded into rectangle, count and disposal) against a per-element
// restatement of what the header documents.  Host code only:
// test_given_host.py builds this with -fsanitize=address,undefined and runs it.  Every buffer is on the heap at exactly the size the ABI
// documents, so a read or write past it is caught.  Exit status 0 and a line of counts: every case agreed, and every class occurred.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "given.h"

using namespace pamd;

namespace {
typedef unsigned long long u64;
constexpr u64 k32 = 0xFFFFFFFFull, kTwo32 = 1ull << 32, kBig = (1ull << 40) + 3;

struct Counts {
    long pal_u8 = 0, pal_f64 = 0, trailing[3] = {0, 0, 0}, all_fill = 0, middle_fill = 0, rows1 = 0, nan_used = 0, inf_used = 0, nan_trailing = 0,
         bytes_clipped = 0, no_bytes = 0;
    long in2 = 0, in8 = 0, in_skip_row = 0, in_skip_beyond = 0, in_collision = 0, in_saturated = 0, derived = 0;
    long out[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, out_subst = 0, out_mid_range = 0, out_empty = 0;
};

bool fail(const char *what, long a = 0, long b = 0) { fprintf(stderr, "given_check: %s (%ld, %ld)\n", what, a, b); return false; }

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {         // a heap block of exactly v.size() elements (none for an empty one)
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

// ---- the caller's palette ------------------------------------------------------------------------------------------------------
unsigned char byte_of(double v) {                              // clip(v * 255, 0, 255), truncated
    const double s = v * 255.0;
    if (s < 0.0) return 0;
    if (s > 255.0) return 255;
    return (unsigned char)std::floor(s);
}

bool check_u8_palette(size_t rows, Counts &c) {
    std::vector<unsigned char> rows8(3 * rows);
    for (size_t i = 0; i < rows8.size(); i++) rows8[i] = (unsigned char)(i * 37 + 11);
    if (rows > 1) { rows8[0] = 0; rows8[1] = 255; }
    const auto p = exact(rows8);
    for (int want = 0; want <= 1; want++) {
        GivenPalette g;
        if (given_palette(nullptr, p.get(), rows, want != 0, g) != kGivenPaletteOk) return fail("u8 palette refused", (long)rows);
        if (g.k != rows || g.pal.size() != 3 * rows) return fail("u8 palette: a row was dropped", (long)rows);
        for (size_t i = 0; i < rows; i++) for (int ch = 0; ch < 3; ch++)
            if (g.pal[(size_t)ch * rows + i] != (double)rows8[3 * i + ch] / 255.0) return fail("u8 palette: value", (long)i, ch);
        if (want ? g.p8 != rows8 : !g.p8.empty()) return fail("u8 palette: bytes", (long)rows, want);
        if (!want) c.no_bytes++;
    }
    c.pal_u8++;
    if (rows == 1) c.rows1++;
    return true;
}

// rows as (r, g, b) triples; what the header documents, restated: k = rows less the trailing triples that are exactly (-1, -1, -1);
// the used rows as given; a used row with a value that is not finite fails; the bytes are byte_of() of every row
bool check_f64_palette(const std::vector<double> &triples, Counts &c) {
    const size_t rows = triples.size() / 3;
    std::vector<double> planar(3 * rows);
    for (size_t i = 0; i < rows; i++) for (int ch = 0; ch < 3; ch++) planar[(size_t)ch * rows + i] = triples[3 * i + ch];
    const auto p = exact(planar);
    size_t k = rows;
    while (k > 0 && triples[3 * (k - 1)] == -1.0 && triples[3 * (k - 1) + 1] == -1.0 && triples[3 * (k - 1) + 2] == -1.0) k--;
    bool finite = true, nan = false, middle = false;
    for (size_t i = 0; i < 3 * k; i++) { if (!std::isfinite(triples[i])) finite = false; if (std::isnan(triples[i])) nan = true; }
    for (size_t i = 0; i + 1 < k; i++) if (triples[3 * i] == -1.0 && triples[3 * i + 1] == -1.0 && triples[3 * i + 2] == -1.0) middle = true;
    const GivenPaletteError expect = k == 0 ? kGivenPaletteAllFill : finite ? kGivenPaletteOk : kGivenPaletteNotFinite;
    for (int want = 0; want <= 1; want++) {
        GivenPalette g;
        const GivenPaletteError got = given_palette(p.get(), nullptr, rows, want != 0, g);
        if (got != expect) return fail("f64 palette: verdict", (long)got, (long)expect);
        if (got != kGivenPaletteOk) continue;
        if (g.k != k || g.pal.size() != 3 * k) return fail("f64 palette: used rows", (long)g.k, (long)k);
        for (size_t i = 0; i < k; i++) for (int ch = 0; ch < 3; ch++)
            if (g.pal[(size_t)ch * k + i] != triples[3 * i + ch]) return fail("f64 palette: value", (long)i, ch);
        if (!want) { if (!g.p8.empty()) return fail("f64 palette: bytes nobody asked for"); c.no_bytes++; continue; }
        if (g.p8.size() != 3 * rows) return fail("f64 palette: byte rows", (long)g.p8.size(), (long)rows);
        for (size_t i = 0; i < 3 * rows; i++) {
            if (g.p8[i] != byte_of(triples[i])) return fail("f64 palette: byte", (long)i, g.p8[i]);
            if (triples[i] < 0.0 || triples[i] > 1.0) c.bytes_clipped++;
        }
    }
    c.pal_f64++;
    if (expect == kGivenPaletteAllFill) c.all_fill++;
    else c.trailing[std::min<size_t>(rows - k, 2)]++;
    if (expect == kGivenPaletteNotFinite) {
        (nan ? c.nan_used : c.inf_used)++;
        if (k == rows && rows > 1 && triples[3 * (rows - 1)] == -1.0 && std::isnan(triples[3 * rows - 1])) c.nan_trailing++;
    }
    if (middle && expect == kGivenPaletteOk) c.middle_fill++;
    if (rows == 1) c.rows1++;
    return true;
}

bool check_palettes(Counts &c) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (size_t rows : {(size_t)1, (size_t)2, (size_t)16, (size_t)257}) if (!check_u8_palette(rows, c)) return false;
    const std::vector<double> F = {-1, -1, -1};
    auto cat = [](std::vector<std::vector<double>> parts) { std::vector<double> o; for (auto &q : parts) o.insert(o.end(), q.begin(), q.end()); return o; };
    const std::vector<double> A = {0.0, 0.5, 1.0}, B = {0.25, 0.999, 1.0 / 255.0}, O = {-0.5, 1.5, 256.0 / 255.0}, N1 = {-1, -1, 0.0}, Z = {-1e-9, 1.0 + 1e-9, -300.0};
    const std::vector<std::vector<double>> cases = {
        A, cat({A, B}), cat({A, B, O, Z}),                        // no fill row; values below 0 and above 1 in the bytes
        cat({A, F}), cat({A, B, F, F, F}), cat({A, F, F}),          // one and several trailing fill rows
        F, cat({F, F, F}),                                        // nothing but fill
        cat({A, F, B}), cat({F, A}), cat({A, F, B, F}),            // a fill row ahead of a used one stays
        cat({A, N1}), cat({N1}),                                  // nearly a fill row: used
        cat({A, {0.1, nan, 0.2}, B}), cat({{nan, 0, 0}}), cat({A, {0.1, 0.2, inf}}), cat({{-inf, 0, 0}, A, F}),   // not finite, in a used row
        // a dropped row is (-1, -1, -1) exactly and so holds neither: the nearest thing is a last row of -1, -1, NaN, which is a used row
        cat({A, {-1, -1, nan}}), cat({A, F, {-1, -1, nan}}),
    };
    for (const auto &t : cases) if (!check_f64_palette(t, c)) return false;
    return true;
}

// ---- the two derivations --------------------------------------------------------------------------------------------------------
bool check_derivations(Counts &c) {
    struct { u64 T; unsigned Td; } ts[] = {{16, 16}, {255, 255}, {k32, 0xFFFFFFFFu}, {kTwo32, 0xFFFFFFFFu}, {kBig, 0xFFFFFFFFu}};
    for (auto &t : ts) { if (given_transparent_on_device(t.T) != t.Td) return fail("transparent index on the device"); c.derived++; }
    struct { int eb; bool dev; int me; } es[] = {{1, false, 1}, {2, false, 4}, {4, false, 4}, {8, false, 4}, {1, true, 1}, {4, true, 4}};
    for (auto &e : es) { if (given_device_elem(e.eb, e.dev) != e.me) return fail("device element size", e.eb); c.derived++; }
    // an index names a position when it fits the caller's elements (and the device's, which are no wider); 8-byte host elements hold
    // any, and beyond 32 bits it saturates
    struct { long long skip; int eb; bool dev; bool on; unsigned Sd; } ss[] = {
        {-1, 1, false, false, 0}, {-1, 8, false, false, 0},
        {5, 1, false, true, 5}, {255, 1, false, true, 255}, {256, 1, false, false, 0}, {256, 1, true, false, 0},
        {5, 2, false, true, 5}, {65535, 2, false, true, 65535}, {65536, 2, false, false, 0},
        {70000, 4, false, true, 70000}, {(long long)k32, 4, true, true, 0xFFFFFFFFu}, {(long long)kTwo32, 4, false, false, 0}, {(long long)kTwo32, 4, true, false, 0},
        {5, 8, false, true, 5}, {(long long)k32, 8, false, true, 0xFFFFFFFFu}, {(long long)kTwo32, 8, false, true, 0xFFFFFFFFu}, {(long long)kBig, 8, false, true, 0xFFFFFFFFu},
    };
    for (auto &s : ss) {
        const GivenSkip g = given_skip_on_device(s.skip, s.eb, given_device_elem(s.eb, s.dev), s.dev);
        if (g.on != s.on || (s.on && g.Sd != s.Sd)) return fail("skip index on the device", (long)s.skip, s.eb);
        c.derived++;
    }
    return true;
}

// ---- inbound elements -----------------------------------------------------------------------------------------------------------
bool check_in(int eb, const std::vector<u64> &values, long long skip_index, Counts &c) {
    const size_t N = values.size();
    std::vector<unsigned short> v2(values.begin(), values.end());
    const auto p2 = exact(v2);
    const auto p8 = exact(values);
    const GivenSkip sk = given_skip_on_device(skip_index, eb, 4, false);
    std::unique_ptr<unsigned[]> dst(new unsigned[N]);
    given_elems_in(eb == 2 ? (const void *)p2.get() : (const void *)p8.get(), eb, N, sk, (u64)skip_index, dst.get());
    for (size_t i = 0; i < N; i++) {
        const u64 v = eb == 2 ? (u64)v2[i] : values[i];
        const bool is_skip = sk.on && skip_index >= 0 && v == (u64)skip_index;
        if (eb == 2) { if (dst[i] != v) return fail("inbound, 2 bytes: not the value", (long)i); continue; }
        if (is_skip) { if (dst[i] != sk.Sd) return fail("inbound: the skip index did not arrive as Sd", (long)i); c.in_skip_row += v <= k32; c.in_skip_beyond += v > k32; continue; }
        if (sk.on && dst[i] == sk.Sd) return fail("inbound: an element that is not the skip index arrived as Sd", (long)i);
        if (v <= k32 && !(sk.on && v == sk.Sd)) { if (dst[i] != v) return fail("inbound: a value that fits was changed", (long)i); continue; }
        if (dst[i] <= (1u << 31)) return fail("inbound: a value that fits no element became a row", (long)i);
        if (v > k32) c.in_saturated++; else c.in_collision++;
    }
    (eb == 2 ? c.in2 : c.in8)++;
    return true;
}

bool check_inbound(Counts &c) {
    const std::vector<u64> small = {0, 1, 5, 255, 256, 0xFFFF, 7}, wide = {0, 5, 0xFFFF, k32, kTwo32, kBig, 0xFFFFFFFEull, 1ull << 31, 5, kBig};
    for (long long skip : {-1LL, 5LL, 0xFFFFLL, 70000LL}) if (!check_in(2, small, skip, c)) return false;
    for (long long skip : {-1LL, 5LL, 0LL, (long long)k32, (long long)kTwo32, (long long)kBig, 9LL}) if (!check_in(8, wide, skip, c)) return false;
    if (!check_in(8, {}, 5, c) || !check_in(2, {}, -1, c)) return false;        // nothing to read
    return true;
}

// ---- outbound elements ----------------------------------------------------------------------------------------------------------
template <typename S, typename D>
bool check_out(size_t N, size_t lo, size_t hi, bool subst, unsigned Td, u64 T, Counts &c) {
    std::vector<S> srcv(N);
    for (size_t i = 0; i < N; i++) srcv[i] = (S)(i % 5 == 3 ? Td : (i * 2654435761u) >> (sizeof(S) == 1 ? 24 : i % 4 * 8));
    std::vector<D> before(N);
    for (size_t i = 0; i < N; i++) before[i] = (D)(0xA5A5A5A5A5A5A5A5ull + i);
    const auto src = exact(srcv);
    const auto dst = exact(before);
    given_elems_out(src.get(), (int)sizeof(S), dst.get(), (int)sizeof(D), lo, hi, subst, Td, T);
    for (size_t i = 0; i < N; i++) {
        const bool in = i >= lo && i < hi;
        const D want = !in ? before[i] : (subst && srcv[i] == (S)Td && (u64)srcv[i] == (u64)Td) ? (D)T : (D)srcv[i];
        if (dst[i] != want) return fail(in ? "outbound: element" : "outbound: an element outside the range was written", (long)i, (long)sizeof(D));
    }
    static const int slot[9] = {0, 0, 1, 0, 2, 0, 0, 0, 3};
    c.out[sizeof(S) == 4][slot[sizeof(D)]]++;
    if (subst) c.out_subst++;
    if (lo > 0 && hi < N && lo < hi) c.out_mid_range++;
    if (lo == hi) c.out_empty++;
    return true;
}

template <typename S>
bool check_out_from(Counts &c) {
    const size_t N = 37;
    const size_t ranges[][2] = {{0, N}, {5, 29}, {11, 11}, {N - 1, N}, {0, 1}};
    for (auto &r : ranges) {
        if (!check_out<S, unsigned char>(N, r[0], r[1], false, 0, 0, c) || !check_out<S, unsigned short>(N, r[0], r[1], false, 0, 0, c) ||
            !check_out<S, unsigned int>(N, r[0], r[1], false, 0, 0, c) || !check_out<S, u64>(N, r[0], r[1], false, 0, 0, c)) return false;
        // the transparent index: one that fits the elements comes back as itself, one beyond 32 bits from the saturated value
        if (!check_out<S, u64>(N, r[0], r[1], true, 200, 200, c) || !check_out<S, unsigned short>(N, r[0], r[1], true, 200, 200, c)) return false;
        if (sizeof(S) == 4 && (!check_out<S, u64>(N, r[0], r[1], true, 0xFFFFFFFFu, kBig, c) || !check_out<S, u64>(N, r[0], r[1], true, 0xFFFFFFFFu, k32, c) ||
                               !check_out<S, unsigned short>(N, r[0], r[1], true, 65535, 65535, c))) return false;
    }
    return check_out<S, u64>(0, 0, 0, false, 0, 0, c);
}

// ---- the frame deltas' words, folded ----------------------------------------------------------------------------------------------
// The kernels' words as csrc/delta.h lays them out, restated: per frame and slot a box of four unsigned (two words), for RGBA maps a
// second such box (V), then per frame and slot a count, then the flag word.
constexpr int kSlots = 32;
size_t words_plain(size_t frames) { return frames * kSlots * 3 + 1; }
size_t words_rgba(size_t frames) { return frames * kSlots * 5 + 1; }

struct Pos { unsigned x, y; int slot; };
struct FrameCase { std::vector<Pos> changed, vanish; };

// what include/patolette_amd.h says of a frame: the tight box of the changed and the vanishing positions as (x0, y0, w, h), (0, 0, 0, 0)
// when there is none; their number; disposal 2 iff something vanishes; frame 0 of plain maps is the full frame with n changed
bool check_fold(bool rgba, unsigned width, unsigned height, const std::vector<FrameCase> &frames, long &cases) {
    const size_t F = frames.size(), cells = F * kSlots, words = rgba ? words_rgba(F) : words_plain(F);
    std::unique_ptr<u64[]> w(new u64[words]);
    std::fill(w.get(), w.get() + words, 0ull);
    unsigned *box = reinterpret_cast<unsigned *>(w.get());
    u64 *cnt = w.get() + cells * (rgba ? 4 : 2);
    auto put = [&](size_t cell, const Pos &p) {                     // as the kernels keep a box: maxima over zero
        unsigned *b = box + 4 * cell;
        b[0] = std::max(b[0], width - p.x); b[1] = std::max(b[1], height - p.y); b[2] = std::max(b[2], p.x + 1); b[3] = std::max(b[3], p.y + 1);
    };
    for (size_t f = 0; f < F; f++) {
        for (const Pos &p : frames[f].changed) { put(f * kSlots + p.slot, p); cnt[f * kSlots + p.slot]++; }
        if (rgba) for (const Pos &p : frames[f].vanish) put(cells + f * kSlots + p.slot, p);
    }
    for (size_t f = 0; f < F; f++) {
        const GivenFrameFold got = given_fold_frame(box + 4 * f * kSlots, rgba ? box + 4 * (cells + f * kSlots) : nullptr, cnt + f * kSlots, kSlots,
                                                    width, height, !rgba && f == 0);
        std::vector<Pos> all = frames[f].changed;
        if (rgba) all.insert(all.end(), frames[f].vanish.begin(), frames[f].vanish.end());
        int want[4] = {0, 0, 0, 0};
        u64 count = frames[f].changed.size();
        if (!rgba && f == 0) { want[2] = (int)width; want[3] = (int)height; count = (u64)width * height; }
        else if (!all.empty()) {
            unsigned x0 = width, y0 = height, x1 = 0, y1 = 0;
            for (const Pos &p : all) { x0 = std::min(x0, p.x); y0 = std::min(y0, p.y); x1 = std::max(x1, p.x); y1 = std::max(y1, p.y); }
            want[0] = (int)x0; want[1] = (int)y0; want[2] = (int)(x1 - x0 + 1); want[3] = (int)(y1 - y0 + 1);
        }
        for (int a = 0; a < 4; a++) if (got.rect[a] != want[a]) return fail("fold: rectangle", (long)f, a);
        if (got.count != count) return fail("fold: count", (long)f, (long)got.count);
        if (got.vanish != (rgba && !frames[f].vanish.empty())) return fail("fold: vanish", (long)f);
        cases++;
    }
    return true;
}

bool check_folds(long &cases) {
    const unsigned W = 7, H = 5;
    const FrameCase empty{}, first{{{0, 0, 0}}, {}}, last{{{W - 1, H - 1, 31}}, {}};
    // every maximum in a slot of its own: x0 from slot 3, y0 from 9, x1 from 17, y1 from 30; two positions share a slot
    const FrameCase spread{{{1, 3, 3}, {4, 1, 9}, {5, 2, 17}, {2, 4, 30}, {3, 3, 30}}, {}};
    const FrameCase disjoint{{{0, 0, 1}, {1, 1, 2}}, {{5, 3, 1}, {6, 4, 7}}};          // C top left, V bottom right: the union, disposal 2
    const FrameCase only_v{{}, {{2, 2, 0}}};                                          // nothing changes, something vanishes: a rectangle still
    for (bool rgba : {false, true}) {
        // frame 0: the override for plain maps (whatever its cells hold), a frame like any other for RGBA maps
        if (!check_fold(rgba, W, H, {empty, empty, first, last, spread}, cases)) return false;
        if (!check_fold(rgba, W, H, {first, spread, empty}, cases)) return false;
        if (!check_fold(rgba, W, H, {disjoint, only_v, disjoint, empty}, cases)) return false;
        if (!check_fold(rgba, 1, 1, {first}, cases)) return false;                 // one frame of one pixel: cells of the last frame end at the counts
    }
    return true;
}
}  // namespace

int main() {
    Counts c;
    if (!check_palettes(c) || !check_derivations(c) || !check_inbound(c) || !check_out_from<unsigned char>(c) || !check_out_from<unsigned int>(c)) return 1;
    long folds = 0;
    if (!check_folds(folds)) return 1;
    printf("given_check: %ld frames folded from their slots agree\n", folds);
    long outs = 0;
    bool every_out = true;
    for (auto &row : c.out) for (long v : row) { outs += v; every_out = every_out && v > 0; }
    printf("given_check: %ld u8 and %ld f64 palettes agree (%ld / %ld / %ld with 0 / 1 / more trailing fill rows, %ld all fill, %ld with a fill row kept, "
           "%ld not finite); %ld derivations; %ld inbound maps (%ld skip indices, %ld saturated, %ld collisions); %ld outbound ranges\n",
           c.pal_u8, c.pal_f64, c.trailing[0], c.trailing[1], c.trailing[2], c.all_fill, c.middle_fill, c.nan_used + c.inf_used, c.derived,
           c.in2 + c.in8, c.in_skip_row + c.in_skip_beyond, c.in_saturated, c.in_collision, outs);
    // the cases the tables are made for did occur
    const bool every = c.pal_u8 && c.pal_f64 && c.trailing[0] && c.trailing[1] && c.trailing[2] && c.all_fill && c.middle_fill && c.rows1 >= 2 &&
                       c.nan_used && c.inf_used && c.nan_trailing && c.bytes_clipped && c.no_bytes && c.in2 && c.in8 && c.in_skip_row && c.in_skip_beyond &&
                       c.in_collision && c.in_saturated && c.derived && every_out && c.out_subst && c.out_mid_range && c.out_empty;
    if (!every) { fprintf(stderr, "given_check: a case is missing\n"); return 1; }
    return 0;
}
