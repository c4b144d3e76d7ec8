"""Kernel time of the ordered map (k_ordered_map) beside the two other maps of remap(): the nearest map and the Riemersma walk.

Per call the times of the kernels named below are summed from the profile (patolette_amd_profile_*); reported: the median over
--calls calls after --warmup calls, and the spread (min .. max).  Content: uniform noise and the synthetic scene of tests/util.py at
--size x --size; the palette is the byte palette of a quantize_u8 call on the same image (256 rows; 16 and 64 too for the ordered
map, whose time is a fixed part per pixel plus a part per row).

    python tools/ordered_time.py [--size 4096] [--calls 12] [--warmup 3] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
import patolette_amd as p  # noqa: E402
from tests.util import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

KERNELS = {"ordered": ("k_ordered_map",),
           False: ("k_convert_u8", "k_nn_map", "k_nn_map_u8"),
           True: ("k_convert_u8", "k_convert", "k_dither_gather", "k_dither_gather_u8", "k_dither", "k_dither_fix", "k_dither_unpermute")}
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, names):
    per_call = []
    for i in range(args.warmup + args.calls):
        p.profile(True)
        fn()
        res = p.profile_results()
        p.profile(False)
        if i >= args.warmup:
            per_call.append(sum(res[k]["total_ms"] for k in names if k in res))
    return "%.3f (%.3f .. %.3f)" % (statistics.median(per_call), min(per_call), max(per_call))


def contents(n):
    rng = np.random.default_rng(1)
    yield "noise", rng.integers(0, 256, size=(n, n, 3), dtype=np.uint8)
    yield "scene", np.round(scene(n, n, 3) * 255).astype(np.uint8)


say("%d x %d, ms per call: median (min .. max) of %d calls after %d" % (args.size, args.size, args.calls, args.warmup))
for kind, img in contents(args.size):
    for rows in (256, 64, 16):
        ok, pal8, _, _, _, msg = p.quantize_u8(img, rows, dither=False, tile_size=0, kmeans_niter=2, kmeans_max_samples=65536, want_quantized=False)
        assert ok, msg
        spread = p.ordered_spread(pal8)
        for mode in ("ordered", False, True) if rows == 256 else ("ordered",):
            t = timed(lambda: p.remap(img, pal8, dither=mode, want_quantized=False), KERNELS[mode])
            say("%s, %3d rows, dither=%-7s %s   [%s]%s" % (kind, rows, mode, t, " + ".join(KERNELS[mode]),
                                                          "  spread %.4f" % spread if mode == "ordered" else ""))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
