"""Kernel time of gif_lzw_lossy's k_lzw_lossy_segments beside gif_lzw's k_lzw_segments on the same inputs in the same session, the
bytes both leave, and what the lossy streams cost in error.

Per call the kernels' times are taken from the profile (patolette_amd_profile_*); reported: the median over --calls calls after
--warmup calls, and the spread (min .. max).  Content: the clip of tests/delta_ref.py, 64 frames of 640 x 360, on the ordered maps of
a quantize_frames(clip, 255) call, in three forms -- the full maps, its deltas at tolerance 0 and its deltas at tolerance 0.05 (both
with their dirty rectangles).  Per form: the exact coder (the yardstick, timed here, not taken from a document); then the lossy coder
under the empty table (the same bytes: what the step itself costs) and under the tables of gif_neighbours at t2 = 0.02, 0.05 and 0.1,
with the mean number of candidates per used row, the share of entries changed, the bytes against the exact coder's, and -- from
`measure` on the composited coded maps against the clip's pixels -- the PSNR and the largest ICtCp distance of a shown entry to its
source pixel (the first row of each form gives both for the exact coder's maps).

    python tools/lzw_lossy_time.py [--calls 12] [--warmup 3] [--frames 64] [--out FILE]"""
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
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()

T = 255
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, name):
    """(median, its text) of kernel `name` over the calls"""
    v = []
    for i in range(args.warmup + args.calls):
        p.profile(True)
        fn()
        res = p.profile_results()
        p.profile(False)
        if i >= args.warmup:
            v.append(res[name]["total_ms"] if name in res else 0.0)
    return statistics.median(v), "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def composite(coded, rects):
    """what a viewer shows: inside its rectangle every entry but T overwrites the canvas (full maps: the maps themselves)"""
    if rects is None:
        return coded
    out = np.empty_like(coded)
    canvas = coded[0].copy()
    for f in range(coded.shape[0]):
        x0, y0, w, h = (int(v) for v in rects[f])
        part = coded[f, y0:y0 + h, x0:x0 + w]
        canvas[y0:y0 + h, x0:x0 + w] = np.where(part == T, canvas[y0:y0 + h, x0:x0 + w], part)
        out[f] = canvas
    return out


def cost(frames, shown, pal8):
    ok, _, per, ictcp, msg = p.measure(frames, shown, pal8)
    assert ok, msg
    return "PSNR %.2f dB, largest distance to the source %.4f" % (p.psnr(per.sum(axis=0)), float(np.sqrt(ictcp[:, 1].max())))


say("ms per call: median (min .. max) of %d calls after %d" % (args.calls, args.warmup))
frames = delta_ref.clip(360, 640, args.frames)
ok, pal8, maps, _, palf, msg = p.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2, kmeans_max_samples=65536,
                                                 want_quantized=False)
assert ok, msg
say("%d frames of 640 x 360, 255 rows, ordered maps, the default segment" % args.frames)
forms = [("the full maps", maps, None)]
for tolerance in (0.0, 0.05):
    ok, deltas, rects, changed, _, msg = p.frame_deltas(maps, pal8, transparent_index=T, frames=frames, tolerance=tolerance)
    assert ok, msg
    forms.append(("deltas at tolerance %g, in their rectangles" % tolerance, deltas, rects))
tables = [("the empty table", np.zeros((256, 16), dtype=np.uint8))]
for t2 in (0.02, 0.05, 0.1):
    ok, near, msg = p.gif_neighbours(pal8, t2, transparent_index=T)
    assert ok, msg
    tables.append(("t2 = %-4g (%.1f candidates a row)" % (t2, near[:255, 0].mean()), near))
for what, m8, rects in forms:
    say(" %s" % what)
    out = []
    exact_ms, text = timed(lambda: out.append(p.gif_lzw(m8, rects)), "k_lzw_segments")
    ok, data, offsets, msg = out[-1]
    assert ok, msg
    exact_bytes = data.size
    r = None if rects is None else np.where(rects[:, 2:3] == 0, np.array([[0, 0, 1, 1]], dtype=rects.dtype), rects)
    say("  the exact coder     k_lzw_segments       %s  %9d bytes; %s" % (text, exact_bytes, cost(frames, composite(m8, r), pal8)))
    for name, near in tables:
        out = []
        ms, text = timed(lambda: out.append(p.gif_lzw_lossy(m8, near, rects, want_coded=True)), "k_lzw_lossy_segments")
        ok, data, offsets, coded, msg = out[-1]
        assert ok, msg
        inside = np.ones(m8.shape, dtype=bool) if r is None else np.zeros(m8.shape, dtype=bool)
        if r is not None:
            for f, (x0, y0, w, h) in enumerate(r):
                inside[f, y0:y0 + h, x0:x0 + w] = True
        say("  %-34s k_lzw_lossy_segments %s = %.2f x; %9d bytes = %.3f x; %.1f %% of the coded entries changed; %s"
            % (name, text, ms / exact_ms, data.size, data.size / exact_bytes, 100.0 * np.sum(coded != m8) / inside.sum(),
               cost(frames, composite(coded, r), pal8)))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
