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

// ---- the Riemersma dither ----
// One dither call: what is walked, onto which palette, into which map.  Every frame is dithered along its own width x height curve
// from the empty error queue.
struct DitherJob {
    // the pixels, one of two forms.  Planes: f64, plane p at planes + p * plane_stride, frame f at offset f * width * height of every
    // plane; `which`: the conversion they still need on their way into linear Rec2020 (PAMD_COPY: none) -- only the lane layout
    // converts on the fly.  Bytes: interleaved 8-bit sRGB, `channels` (3 or 4) each, frame after frame; the conversion rides on the
    // lane layout's gather and no f64 image exists, so the caller has checked that the lane layout applies (dither_lane_layout, resp.
    // dither_frames_lane_layout for frames > 1).
    const double *planes = nullptr;
    size_t plane_stride = 0;
    int which = -1;
    const unsigned char *bytes = nullptr;
    int channels = 3;
    // A single image has up to 2^32 - 1 pixels; more frames than one, and bytes, kDitherFramesMaxPixels in all.
    size_t frames = 1, width = 0, height = 0;
    // Masked (the RGBA entries; planes, one frame): only some pixels are visited.  cpos[pixel] = the pixel's number among the `opaque`
    // ones (row-scan order), or -1 for a transparent pixel, which the walk skips exactly like a position outside the image.  The planes
    // are then the opaque pixels' compact ones (plane_stride >= opaque), the map `opaque` choices in compact order, and the layout is
    // decided on `opaque`.  mpos: the launcher's own (the table it makes of cpos, in dither_mask_reserve's part of the workspace).
    const int *cpos = nullptr;
    size_t opaque = 0;
    const unsigned *mpos = nullptr;
    // the palette, planar (k,3) in linear Rec2020: on the device and, if the caller has it, on the host (else it is read back)
    const double *d_pal = nullptr, *h_pal = nullptr;
    int k = 0;
    // the map: frame f's choices at element f * width * height; elements of 1, 4 or 8 bytes
    void *out = nullptr;
    int elem_bytes = 0;
    int layout = -1;                   // 1 lanes, 0 wavefronts, -1 decided by the launcher (what the caller decided when it chose the pixels' form)
};
constexpr size_t kDitherFramesMaxPixels = (size_t)1 << 31;
// Which layout walks the runs when the job does not say: one lane per run (all frames side by side in one set of launches) where these
// hold, else one wavefront per run, frame after frame, which takes planes in linear Rec2020 (which == PAMD_COPY).
bool dither_lane_layout(size_t width, size_t height, int k);
bool dither_frames_lane_layout(size_t frames, size_t width, size_t height, int k);
// Returns false only for bytes, when the lane walk's verification stalled for good and nothing usable was written: the caller then
// converts the image and sends the planes with layout 0.  Planes that stall are converted and walked by the wavefront layout here.
bool launch_dither(const DitherJob &job, NNWork &w, hipStream_t s);
// what a masked job takes of the workspace for an image of npix pixels, for callers that reserve before anything is enqueued
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
