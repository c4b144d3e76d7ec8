// map.h -- launchers of the palette-mapping kernels (map.hip).
#pragma once

#include "common.h"

namespace pamd {

// colours: planar, plane p at d_colors + p*plane_stride, n pixels mapped; palette planar (k,3);
// output elements of elem_bytes (1, 4 or 8)
struct NNWork {                        // scratch of the pruned NN map
    DevBuf<unsigned char> lut;         // per grid cell: 32 candidate slots (u8 or u16), count in the last
    DevBuf<unsigned long long> keys;   // min/max keys when the caller has no bounds
    DevBuf<unsigned char> clist;       // coarse pass of the LUT build: surviving entries per 4x4x4 block of cells
    DevBuf<unsigned int> mid;          // (G/2)^3 table of up to four candidates per cell, held in LDS by k_nn_map_mid
    DevBuf<double> dtab;               // dither with more than 3200 palette entries: its two palette tables (6 k doubles)
    DevBuf<unsigned int> dside;        // segment-parallel dither: [S][16] boundary choices + the repair counter
    PinBuf<unsigned int> hrep;         // ... the counter's landing place on the host
    DevBuf<double> dsort;              // lane-per-run dither: the pixels in curve order (3 planes)
    DevBuf<unsigned int> dpos;         // ... their linear pixel numbers (a function of width and height: kept between calls)
    size_t order_w = 0, order_h = 0; int order_dev = -1;
    DevBuf<unsigned int> dmpos;        // masked dither: the opaque pixels' compact numbers in curve order (made from dpos, which stays as it is)
    DevBuf<unsigned int> dmcnt;        // ... the compaction's tile counts / offsets and, behind them, the count
    DevBuf<unsigned char> dsmap;       // ... the choices in curve order, and behind them the [S][16] boundary records
    DevBuf<unsigned char> dflag;       // ... [S + 1] which boundaries the last check listed
    size_t dither_segments = 0, dither_repairs = 0, dither_rounds = 0;   // of the last launch_dither
    size_t dither_through = 0;         // ... times a stalled verification was resolved by walking one run through its successors
    size_t dither_jumps = 0;           // ... periodic jumps through flat stretches (lane layout's repair walks)
    size_t dither_solo = 0;            // ... passes taken by one wavefront alone (lane layout)
    hipStream_t side_stream = nullptr, side_stream2 = nullptr;   // lane-per-run dither: the record grids are built here while the pixels are gathered
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;
    int side_dev = -1;
    // tests (dither_lane_tables): what the last dither's lane layout gave its kernels -- the three grids (first, 1.5 extents, 4 extents)
    // and the margins of the f32 first pass; the record tables themselves are still in `lut`.  valid: the last dither or nearest map
    // on this workspace was a lane-layout dither that finished
    struct LaneTables { bool valid = false; double lo[3][3], hi[3][3], inv[3][3]; int G[3]; float amb, amb_p, amb_x; } lane_tables;
    NNWork() = default;
    NNWork(const NNWork &) = delete;
    NNWork &operator=(const NNWork &) = delete;
    ~NNWork() {
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (ev_join2) (void)hipEventDestroy(ev_join2);
        if (side_stream) (void)hipStreamDestroy(side_stream);
        if (side_stream2) (void)hipStreamDestroy(side_stream2);
    }
};
// lo/hi: exact per-plane min/max of the colours if known (else nullptr: computed with one more pass)
void launch_nn_map(const double *d_colors, size_t plane_stride, size_t n, const double *d_pal, int k,
                   void *d_out, int elem_bytes, const double *lo, const double *hi, NNWork &w, hipStream_t s);
// TESTS ONLY: the size class launch_nn_map and nn_map_u8_applies pretend (0 = the one of n, 1 = below 16 384 pixels, 2 = from 16 384,
// 3 = from 2^22); the limits on k are untouched.  Process-wide; returns the previous setting.
int nn_debug_route(int route);
// The same map straight from interleaved 8-bit sRGB pixels (`channels` 3 or 4 bytes each; palette in ICtCp): the LDS-table kernel with
// a byte source that converts in registers, no f64 image.  Only where nn_map_u8_applies (the sizes and palettes that kernel takes);
// elements of 1 or 4 bytes.
bool nn_map_u8_applies(size_t n, int k);
void launch_nn_map_u8(const unsigned char *d_px, int channels, size_t n, const double *d_pal, int k, void *d_out, int elem_bytes, NNWork &w, hipStream_t s);
// which: the conversion the pixels still need on their way into linear Rec2020 (PAMD_COPY: none) -- only the lane-per-run layout
// (dither_lane_layout) converts on the fly; h_pal: the same palette on the host if the caller has it (else it is read back)
bool dither_lane_layout(size_t width, size_t height, int k);
void launch_dither(const double *d_img, size_t plane_stride, int which, size_t width, size_t height, const double *d_pal, const double *h_pal, int k,
                   void *d_out, int elem_bytes, NNWork &w, hipStream_t s, int layout = -1);   // layout: 1 lanes, 0 wavefronts, -1 decide here

// `frames` images of width x height one after another (frame f's pixels at offset f * width * height of every plane and of d_out), one
// palette: every frame is dithered along its own curve from the empty error queue, exactly as launch_dither would dither it alone.
// Where dither_frames_lane_layout holds, all frames are walked side by side in one set of launches; otherwise frame after frame
// through the wavefront layout, which takes linear Rec2020 pixels (which == PAMD_COPY).  At most kDitherFramesMaxPixels in all.
constexpr size_t kDitherFramesMaxPixels = (size_t)1 << 31;
bool dither_frames_lane_layout(size_t frames, size_t width, size_t height, int k);
void launch_dither_frames(const double *d_img, size_t plane_stride, int which, size_t frames, size_t width, size_t height, const double *d_pal,
                          const double *h_pal, int k, void *d_out, int elem_bytes, NNWork &w, hipStream_t s, int layout = -1);

// The lane layout straight from interleaved 8-bit sRGB pixels (the remap entry): `frames` images of width x height, `channels` (3 or 4)
// bytes per pixel, palette in linear Rec2020; the conversion rides on the gather and no f64 image exists.  Only where the lane layout
// applies (dither_lane_layout, resp. dither_frames_lane_layout for frames > 1).  Returns false when the walk's verification stalled
// for good: the caller then converts the image and calls launch_dither / launch_dither_frames.
bool launch_dither_u8(const unsigned char *d_px, int channels, size_t frames, size_t width, size_t height, const double *d_pal, const double *h_pal,
                      int k, void *d_out, int elem_bytes, NNWork &w, hipStream_t s);

// The same chain over a width x height image of which only some pixels are visited (the RGBA entry): d_cpos[pixel] = the pixel's
// number among the m opaque ones (row-scan order), or -1 for a transparent pixel, which the walk skips exactly like a position
// outside the image.  d_img: the opaque pixels' compact planes (plane_stride >= m), d_out: m choices in compact order.  The layout
// is decided on m (dither_lane_layout(m, 1, k)) unless the caller passes it.
void launch_dither_masked(const double *d_img, size_t plane_stride, int which, size_t width, size_t height, const int *d_cpos, size_t m,
                          const double *d_pal, const double *h_pal, int k, void *d_out, int elem_bytes, NNWork &w, hipStream_t s, int layout = -1);
// what launch_dither_masked takes of the workspace for an image of npix pixels, reserved before anything is enqueued
void dither_mask_reserve(NNWork &w, size_t npix);

// test / tuning knob: runs the curve is cut into (0 = chosen from the image size) and in-image pixels of warm-up (< 0 = default)
void dither_config(int segments, int warm);
// which layout walks the runs: 1 = one lane per run where it applies (default), 0 = one wavefront per run, -1 = default
void dither_layout(int lanes);
// tests: solo passes after which the lane layout gives up and the wavefront layout takes the image (default 4096, never reached);
// returns the previous value
int dither_solo_cap(int cap);
int dither_stall_passes(int n);
// tests: the lane layout's tables of the last dither on this workspace, read back (patolette_amd_debug_dither_lane_tables in
// patolette_amd.h says what goes where).  0, or -1 where that dither did not take the lane layout or `capacity` is too small.
int dither_lane_tables(NNWork &w, double *geom30, float *amb3, unsigned char *tables, size_t capacity, hipStream_t s);
// keep the curve order of an image size on the device between calls (default) or make it again in every call
void dither_order_cache(bool on);

}  // namespace pamd
