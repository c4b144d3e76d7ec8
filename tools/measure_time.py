"""Kernel time of measure (k_measure, and k_measure_fold behind it), integers only and with the ICtCp part, beside the nearest remap of
the same pixels (which reads the same channels + element bytes per pixel and searches the palette besides).

Per call the kernels' times are taken from the profile (patolette_amd_profile_*); reported: the median over --calls calls after
--warmup calls, and the spread (min .. max).  Content: the synthetic scene of tests/util.py at --size x --size with the 256-row byte
palette of a quantize_u8 call on it and its nearest map -- and, as the worst and the best case for the per-entry atomics, a map
with every position on one row and a uniformly random one; then the clip of tests/delta_ref.py, 64 frames of 640 x 360, on the ordered maps of a quantize_frames(clip, 255)
call.  For the integer-only mode the traffic is channels + element bytes per position; its share of the HBM peak is given against
the 8.0 TB/s of the data sheet.

    python tools/measure_time.py [--size 4096] [--calls 12] [--warmup 3] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
import patolette_amd as p  # noqa: E402
from tests import delta_ref  # noqa: E402
from tests.util import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

HBM_PEAK = 8.0e12
NEAREST = ("k_convert_u8", "k_nn_map", "k_nn_map_u8")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, names):
    """median and text of the summed times of `names`, per call"""
    per_call = []
    for i in range(args.warmup + args.calls):
        p.profile(True)
        fn()
        res = p.profile_results()
        p.profile(False)
        if i >= args.warmup:
            per_call.append(sum(res[k]["total_ms"] for k in names if k in res))
    return statistics.median(per_call), "%.3f (%.3f .. %.3f)" % (statistics.median(per_call), min(per_call), max(per_call))


def report(image, maps, pal8, what):
    N = maps.size
    remap_ms, text = timed(lambda: p.remap(image, pal8, dither=False, want_quantized=False), NEAREST)
    say("  nearest remap [%s]   %s" % (" + ".join(NEAREST), text))
    for ictcp in (False, True):
        out = []
        ms, text = timed(lambda: out.append(p.measure(image, maps, pal8, ictcp=ictcp)), ("k_measure",))
        _, fold = timed(lambda: p.measure(image, maps, pal8, ictcp=ictcp), ("k_measure_fold",))
        ok, ent, per, dist, msg = out[-1]
        assert ok, msg
        note = "%.3f of the nearest remap" % (ms / remap_ms)
        if not ictcp:
            rate = (image.shape[-1] + maps.dtype.itemsize) * N / (ms * 1e-3)
            note += "; %.0f GB/s = %.1f %% of the HBM peak" % (rate / 1e9, 100.0 * rate / HBM_PEAK)
        say("  k_measure %s ictcp=%-5s  %s + k_measure_fold %s   %s; PSNR %.2f dB, %d of %d rows named"
            % (what, ictcp, text, fold, note, float(p.psnr(per.sum(axis=0) * [1, 1, 0])), int(np.sum(ent[:, 0] > 0)), ent.shape[0]))


say("ms per call: median (min .. max) of %d calls after %d" % (args.calls, args.warmup))
img = np.round(scene(args.size, args.size, 3) * 255).astype(np.uint8)
ok, pal8, _, _, _, msg = p.quantize_u8(img, 256, dither=False, tile_size=0, kmeans_niter=2, kmeans_max_samples=65536, want_quantized=False)
assert ok, msg
ok, pmap, _, msg = p.remap(img, pal8, dither=False, want_quantized=False)
assert ok, msg
say("%d x %d scene, %d-byte elements, %d rows" % (args.size, args.size, pmap.dtype.itemsize, pal8.shape[0]))
report(img, pmap, pal8, "its nearest map  ")
report(img, np.zeros_like(pmap), pal8, "all on one row   ")
report(img, np.random.default_rng(1).integers(0, pal8.shape[0], size=pmap.shape).astype(pmap.dtype), pal8, "a random map     ")
frames = delta_ref.clip(360, 640, 64)
ok, pal8, maps, _, _, msg = p.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2, kmeans_max_samples=65536,
                                              want_quantized=False)
assert ok, msg
say("64 frames of 640 x 360, %d-byte elements, %d rows" % (maps.dtype.itemsize, pal8.shape[0]))
report(frames, maps, pal8, "its ordered maps ")
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
