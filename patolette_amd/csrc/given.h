// given.h -- what the caller gives the palette-given entries (remap, frame_deltas, measure; include/patolette_amd.h), what their index
// maps look like on either side of the link, and what the host makes of the frame deltas' slots: each rule once.  Host code only (no
// HIP header): tests/given_check.cpp runs it under sanitizers over buffers of exactly the sizes the ABI documents.  The device's side
// of the shared rules is given_device.h.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pamd {

// palette_u8 = clip(palette * 255, 0, 255) truncated (README.md:178-181); unused rows (-1) become 0.  palette: planar (K,3)
inline void palette_to_u8(const double *palette, size_t K, unsigned char *out) {
    for (size_t i = 0; i < K; i++)
        for (int c = 0; c < 3; c++) {
            double v = palette[K * (size_t)c + i] * 255.0;
            v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
            out[3 * i + c] = (unsigned char)v;
        }
}

// The caller's palette of `rows` rows, given as exactly one of `palette` (planar (rows,3) f64 sRGB) and `palette_u8` ((rows,3) bytes).
//   pal, k: the used rows, planar (k,3) f64 sRGB.  u8: every row, byte / 255.  f64: the rows as given without the trailing
//           (-1, -1, -1) ones, the reference's fill of unused rows (patolette.c:327-336); such a row ahead of a used one stays.
//   p8:     with want_bytes, the bytes of all `rows` rows (dropped ones included: a map element may not name them, `quantized` and the
//           outputs are still sized by them).  u8: the palette as given.  f64: palette_to_u8 of it.
// Fails when no row is left, or when a used row holds a value that is not finite.
enum GivenPaletteError { kGivenPaletteOk = 0, kGivenPaletteAllFill, kGivenPaletteNotFinite };
struct GivenPalette {
    std::vector<double> pal;
    size_t k = 0;
    std::vector<unsigned char> p8;
};
inline GivenPaletteError given_palette(const double *palette, const unsigned char *palette_u8, size_t rows, bool want_bytes, GivenPalette &out) {
    size_t k = rows;
    if (palette_u8) {
        out.pal.resize(3 * k);
        for (size_t i = 0; i < k; i++) for (int c = 0; c < 3; c++) out.pal[(size_t)c * k + i] = (double)palette_u8[3 * i + c] / 255.0;
        if (want_bytes) out.p8.assign(palette_u8, palette_u8 + 3 * rows);
    } else {
        auto row_is = [&](size_t i, double v) { return palette[i] == v && palette[rows + i] == v && palette[2 * rows + i] == v; };
        while (k > 0 && row_is(k - 1, -1.0)) k--;
        if (k == 0) return kGivenPaletteAllFill;
        out.pal.resize(3 * k);
        for (size_t i = 0; i < k; i++) for (int c = 0; c < 3; c++) {
            const double v = palette[rows * (size_t)c + i];
            if (!std::isfinite(v)) return kGivenPaletteNotFinite;
            out.pal[(size_t)c * k + i] = v;
        }
        if (want_bytes) { out.p8.resize(3 * rows); palette_to_u8(palette, rows, out.p8.data()); }
    }
    out.k = k;
    return kGivenPaletteOk;
}

// Rows first .. rows - 1 of p8 ((r, g, b) bytes) as one word each, r in the low byte, with `high` or-ed in (0xFF000000: the row's
// opaque RGBA word); the rows below `first` are 0
inline std::vector<unsigned> given_row_words(const std::vector<unsigned char> &p8, size_t rows, size_t first = 0, unsigned high = 0) {
    std::vector<unsigned> w(rows, 0u);
    for (size_t i = first; i < rows; i++) w[i] = (unsigned)p8[3 * i] | (unsigned)p8[3 * i + 1] << 8 | (unsigned)p8[3 * i + 2] << 16 | high;
    return w;
}

// An index map's elements: `eb` bytes each as the caller holds them, `me` on the device.  Device maps are used as they are; of host
// maps the 1- and 4-byte ones go up as they are, the 2- and 8-byte ones as 4-byte elements
inline int given_device_elem(int eb, bool on_device) { return (on_device || eb == 1) ? eb : 4; }

// frame_deltas' transparent index T on the device.  Only 8-byte host elements let T pass 32 bits; it then saturates, and stays above
// every row (rows <= 2^31)
inline unsigned given_transparent_on_device(unsigned long long T) { return T > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)T; }

// measure's skip index on the device: whether any element can be it, and its value Sd there.  skip < 0: none.  An index that does not
// fit the elements names no position; 8-byte host elements hold any, and one beyond 32 bits saturates as T does
struct GivenSkip { bool on = false; unsigned Sd = 0; };
inline GivenSkip given_skip_on_device(long long skip, int eb, int me, bool on_device) {
    GivenSkip s;
    if (skip < 0) return s;
    const unsigned long long v = (unsigned long long)skip;
    if (me == 1 || on_device || eb != 8) { s.on = (v >> (8 * (eb < me ? eb : me))) == 0; s.Sd = (unsigned)v; }
    else { s.on = true; s.Sd = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)v; }
    return s;
}

// Inbound: N host elements of eb = 2 or 8 bytes into the device's 4-byte ones.  2 bytes: the value.  8 bytes: the skip index itself
// (skip.on, `skip_index`) becomes skip.Sd; a value beyond 32 bits, or one that only collides with Sd, becomes `beyond`, which is above
// every row (rows <= 2^31) and is not Sd: it stays "not a row"; any other value is kept.  No skip (frame_deltas): GivenSkip{}
inline void given_elems_in(const void *src, int eb, size_t N, GivenSkip skip, unsigned long long skip_index, unsigned *dst) {
    if (eb == 2) { for (size_t i = 0; i < N; i++) dst[i] = ((const unsigned short *)src)[i]; return; }
    const unsigned long long *s = (const unsigned long long *)src;
    const unsigned beyond = skip.Sd == 0xFFFFFFFFu ? 0xFFFFFFFEu : 0xFFFFFFFFu;
    for (size_t i = 0; i < N; i++) {
        const unsigned long long v = s[i];
        dst[i] = (skip.on && v == skip_index) ? skip.Sd : (v > 0xFFFFFFFFull || (skip.on && v == skip.Sd) ? beyond : (unsigned)v);
    }
}

// Outbound: elements [lo, hi) of the device's map at src (me = 1 or 4 bytes each) into the same positions of dst, host elements of
// eb = 1, 2, 4 or 8 bytes: the value, cut to eb bytes.  With `subst`, a value equal to Td (given_transparent_on_device(T)) becomes T first
template <bool Subst, typename S, typename D>
inline void given_elems_out_loop(const S *src, D *dst, size_t lo, size_t hi, unsigned Td, unsigned long long T) {
    for (size_t i = lo; i < hi; i++) dst[i] = (Subst && src[i] == Td) ? (D)T : (D)src[i];
}
template <bool Subst, typename S>
inline void given_elems_out_to(const S *src, void *dst, int eb, size_t lo, size_t hi, unsigned Td, unsigned long long T) {
    switch (eb) {
        case 1: given_elems_out_loop<Subst>(src, (unsigned char *)dst, lo, hi, Td, T); break;
        case 2: given_elems_out_loop<Subst>(src, (unsigned short *)dst, lo, hi, Td, T); break;
        case 4: given_elems_out_loop<Subst>(src, (unsigned int *)dst, lo, hi, Td, T); break;
        default: given_elems_out_loop<Subst>(src, (unsigned long long *)dst, lo, hi, Td, T); break;
    }
}
inline void given_elems_out(const void *src, int me, void *dst, int eb, size_t lo, size_t hi, bool subst = false, unsigned Td = 0,
                            unsigned long long T = 0) {
    auto from = [&](auto *s) { subst ? given_elems_out_to<true>(s, dst, eb, lo, hi, Td, T) : given_elems_out_to<false>(s, dst, eb, lo, hi, Td, T); };
    if (me == 1) from((const unsigned char *)src); else from((const unsigned int *)src);
}

// What the frame-delta kernels leave for one frame, folded into what the caller gets.  A box arrives spread over `slots` cells of
// four unsigned each, every cell as maxima over zero of (width - x0, height - y0, x1 + 1, y1 + 1): an empty box is all zero, a union
// the element-wise maximum.  c_box, cnt: the cells and counts of the changed positions (C).  v_box: the cells of the positions that
// vanish in the next frame (V), or null for plain maps, which have no such box.  full: the frame is the whole first map whatever the
// cells hold (plain maps, frame 0).
//   rect   (x0, y0, w, h) of the smallest box that holds C and V; (0, 0, 0, 0) when both are empty (no cell has an x1 + 1)
//   count  the changed positions;  vanish: V is not empty (RGBA maps: disposal 2)
struct GivenFrameFold { int32_t rect[4]; unsigned long long count; bool vanish; };
inline GivenFrameFold given_fold_frame(const unsigned *c_box, const unsigned *v_box, const unsigned long long *cnt, int slots, size_t width,
                                       size_t height, bool full) {
    unsigned m[4] = {0, 0, 0, 0};
    GivenFrameFold out{{0, 0, 0, 0}, 0, false};
    for (int j = 0; j < slots; j++) {
        for (int a = 0; a < 4; a++) {
            if (c_box[4 * j + a] > m[a]) m[a] = c_box[4 * j + a];
            if (v_box && v_box[4 * j + a] > m[a]) m[a] = v_box[4 * j + a];
        }
        if (v_box && v_box[4 * j + 2] != 0) out.vanish = true;
        out.count += cnt[j];
    }
    if (full) { m[0] = m[2] = (unsigned)width; m[1] = m[3] = (unsigned)height; out.count = (unsigned long long)width * height; }
    if (m[2] != 0) {
        const unsigned x0 = (unsigned)width - m[0], y0 = (unsigned)height - m[1];
        out.rect[0] = (int32_t)x0; out.rect[1] = (int32_t)y0; out.rect[2] = (int32_t)(m[2] - x0); out.rect[3] = (int32_t)(m[3] - y0);
    }
    return out;
}

}  // namespace pamd
