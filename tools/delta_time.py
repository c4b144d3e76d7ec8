"""Kernel time of the frame deltas (k_frame_deltas, and k_delta_boxes behind it), exact and lossy, beside the ordered map (k_ordered_map) that made the maps.

Per call the kernel's time is taken from the profile (patolette_amd_profile_*); reported: the median over --calls calls after --warmup
calls, and the spread (min .. max).  Content: the clip of tests/delta_ref.py (one scene, +-2 of noise per frame, a moving inverted
block) -- 64 frames of 640 x 360 and 2 frames of 4096 x 4096 -- on the ordered maps of a quantize_frames(clip, 255) call.  For the
exact mode the traffic is 2 x element bytes per pixel-frame (the element read, the delta written); its share of the HBM peak is given
against the 8.0 TB/s of the data sheet.

    python tools/delta_time.py [--calls 12] [--warmup 3] [--tolerance 0.05] [--skip-large] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
import patolette_amd as p  # noqa: E402
from tests import delta_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--tolerance", type=float, default=0.05)
ap.add_argument("--skip-large", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

HBM_PEAK = 8.0e12
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, name, also=None):
    per_call, others = [], []
    for i in range(args.warmup + args.calls):
        p.profile(True)
        fn()
        res = p.profile_results()
        p.profile(False)
        if i >= args.warmup:
            per_call.append(res[name]["total_ms"])
            if also:
                others.append(res[also]["total_ms"])
    text = "%.3f (%.3f .. %.3f)" % (statistics.median(per_call), min(per_call), max(per_call))
    if also:
        text += " + %s %.3f (%.3f .. %.3f)" % (also, statistics.median(others), min(others), max(others))
    return statistics.median(per_call), text


say("ms per call: median (min .. max) of %d calls after %d" % (args.calls, args.warmup))
for F, h, w in ((64, 360, 640),) + (() if args.skip_large else ((2, 4096, 4096),)):
    frames = delta_ref.clip(h, w, F)
    ok, pal8, maps, _, _, msg = p.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2, kmeans_max_samples=65536,
                                                  want_quantized=False)
    assert ok, msg
    N = F * h * w
    say("%d frames of %d x %d, %d-byte elements, 255 rows" % (F, w, h, maps.dtype.itemsize))
    _, text = timed(lambda: p.remap(frames, pal8, dither="ordered", want_quantized=False), "k_ordered_map")
    say("  k_ordered_map (the maps themselves)      %s" % text)
    for tolerance, shown in ((0.0, False), (0.0, True), (args.tolerance, False), (args.tolerance, True)):
        out = []
        med, text = timed(lambda: out.append(p.frame_deltas(maps, pal8, frames=frames, tolerance=tolerance, want_shown=shown)), "k_frame_deltas",
                          "k_delta_boxes")
        ok, d, r, c, s, msg = out[-1]
        assert ok, msg
        note = "changed per frame %.2f %% .. %.2f %%" % (100.0 * c[1:].min() / (h * w), 100.0 * c[1:].max() / (h * w))
        if tolerance == 0.0 and not shown:
            rate = 2.0 * maps.dtype.itemsize * N / (med * 1e-3)
            note += "; %.0f GB/s = %.1f %% of the HBM peak" % (rate / 1e9, 100.0 * rate / HBM_PEAK)
        say("  k_frame_deltas tolerance %-4g shown=%-5s  %s   %s" % (tolerance, shown, text, note))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
