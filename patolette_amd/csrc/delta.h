// delta.h -- launchers of the frame-delta kernels (delta.hip): plain maps, plain maps with a colour table per frame, and maps whose
// index 0 is a transparent entry.
#pragma once

#include "common.h"

namespace pamd {

// palette rows a block of the lossy kernels holds in LDS (given_device.h, LossyLds: 24 KB next to the 4 KB of pow tables and the
// 2 KB companding table); a longer palette is indexed in global memory
constexpr int kDeltaChunk = 1024;
// same-address atomics serialise in L2: a frame's box and count are spread over this many slots, which the host folds
// (given.h, given_fold_frame)
constexpr int kDeltaSlots = 32;

// what the kernels leave for the host, as unsigned long long words: per frame and slot a box of four unsigned ints (given_device.h
// says how a box is kept), then per frame and slot a count, then one word whose low bit says that some element was not below `rows`
inline size_t frame_deltas_words(size_t frames) { return frames * (size_t)kDeltaSlots * 3 + 1; }
// between the two kernels: per frame one 64-bit ballot per wavefront of positions (bit i of word w: position 64 w + i changed)
inline size_t frame_deltas_masks(size_t frames, size_t n) { return frames * ceil_div(n, 64); }

// The frame deltas of include/patolette_amd.h (patolette_amd_frame_deltas): `frames` index maps of width x height with elements of
// 1 or 4 bytes; rows: the number every element must stay below (lossy: the palette's used rows, the stride of d_pal); T: the
// transparent index.  lossy: d_px are the frames' interleaved 8-bit sRGB pixels, d_pal the palette in ICtCp, planar (rows,3), tol2
// the squared tolerance; otherwise none of the three is read.  d_delta (may be d_maps) and d_shown may be null.  d_masks:
// frame_deltas_masks(frames, n) words of scratch; d_words: frame_deltas_words(frames) words, zeroed here.  One kernel walks all
// frames (k_frame_deltas), a small one folds its ballots into the boxes and counts (k_delta_boxes).
void launch_frame_deltas(const void *d_maps, int elem_bytes, size_t frames, size_t width, size_t height, size_t rows, size_t T, bool lossy,
                         const unsigned char *d_px, int channels, const double *d_pal, double tol2, void *d_delta, void *d_shown,
                         unsigned long long *d_masks, unsigned long long *d_words, hipStream_t s);

// colour words a block of k_frame_deltas_local holds in LDS at most (16 KB beside the lossy mode's 30 KB: five blocks a CU stay)
constexpr int kLocalLdsRows = 4096;

// The frame deltas of maps with a colour table per frame (include/patolette_amd.h, patolette_amd_frame_deltas_local): `frames` maps of
// one-byte elements; frame f indexes table d_pof[f] (each in [0, P): the caller has checked them) of P tables of K rows, K in
// [1, 255]; T in [K, 255].  d_rows: the P K rows' packed RGB words (given.h, given_row_words); d_pal (lossy only): the P K rows in
// ICtCp, planar (P K,3).  d_delta (frames x n bytes, may be d_maps) and d_shown (frames x n x 3 bytes, colours) may be null.  d_masks,
// d_words: as launch_frame_deltas takes them, and the words come out in its layout.  One launch of k_frame_deltas_local, then
// k_delta_boxes.  The rows' words go to LDS when they number at most kLocalLdsRows and at most 256 per frame, otherwise they are
// read from global memory; same results.
void launch_frame_deltas_local(const unsigned char *d_maps, size_t frames, size_t width, size_t height, size_t K, size_t P, size_t T, bool lossy,
                               const int *d_pof, const unsigned *d_rows, const unsigned char *d_px, int channels, const double *d_pal, double tol2,
                               unsigned char *d_delta, unsigned char *d_shown, unsigned long long *d_masks, unsigned long long *d_words, hipStream_t s);
// TESTS ONLY: where k_frame_deltas_local reads the rows' words: -1 the launcher's rule, 0 global memory, 1 LDS whenever they number at
// most kLocalLdsRows.  Same results.  Returns the previous mode.  delta_local_route: what the last launch took, 1 LDS, 0 global
// memory, -1 before the first one.
int delta_debug_local_tables(int mode);
int delta_local_route();

// what the kernels of the RGBA flavour leave for the host, as unsigned long long words: per frame and slot the box of the changed
// positions (C), then per frame and slot the box of the positions that vanish in the next frame (V), both as above and 16 bytes a
// cell; then per frame and slot the count of C; then the flag word
inline size_t frame_deltas_rgba_words(size_t frames) { return frames * (size_t)kDeltaSlots * 5 + 1; }

// The frame deltas of maps whose index 0 is the transparent entry (include/patolette_amd.h, patolette_amd_frame_deltas_rgba): the
// arguments of launch_frame_deltas without T; loop: whether frame 0 follows the last one.  d_delta (may be d_maps) may be null.
// d_shown: frames x n elements or null; without it d_canvas is one frame of workspace (n elements) that holds the canvas between the
// launches.  d_words: frame_deltas_rgba_words(frames) words, zeroed here.  One launch of k_rgba_vanish for every frame's V box and
// the flag, then one of k_frame_delta_rgba per frame, all on `s`; nothing waits in between.
void launch_frame_deltas_rgba(const void *d_maps, int elem_bytes, size_t frames, size_t width, size_t height, size_t rows, int loop, bool lossy,
                              const unsigned char *d_px, int channels, const double *d_pal, double tol2, void *d_delta, void *d_shown,
                              void *d_canvas, unsigned long long *d_words, hipStream_t s);

// TESTS ONLY: how many positions a lane of k_frame_deltas (and of the RGBA flavour's kernels) owns: -1 the launcher's rule (four from 32 wavefronts per CU on, where the
// sizes and addresses allow vector accesses), 0 always one, 1 four wherever they are allowed.  Same results.  Returns the previous mode.
int delta_debug_quad(int mode);

}  // namespace pamd
