"""Kernel time of k_rgba_stamp, the pass remap_rgba adds behind the nearest and the ordered map, beside those maps' own kernels on the
same pixels in the same session -- with four pixels per lane (the default) and with one (patolette_amd_debug_rgba_stamp_quad).

Per call the kernels' times are taken from the profile (patolette_amd_profile_*); reported: the median over --calls calls after
--warmup calls, and the spread (min .. max).  Content: the synthetic scene of tests/util.py at --size x --size, then the clip of
tests/delta_ref.py, 64 frames of 640 x 360; alpha 0 outside a disc (about 45 % of the pixels), 255 inside; the 256-row palette
(transparent entry included) of a quantize_rgba_frames call on the pixels.  The stamp moves 4 (pixel) + 1 (the mapper's element) + 1
(the final element) + 4 (the RGBA word) = 10 bytes per pixel; its share of the HBM peak is given against the 8.0 TB/s of the data sheet.

    python tools/remap_rgba_time.py [--size 4096] [--calls 12] [--warmup 3] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
import patolette_amd as p  # noqa: E402
from patolette_amd import _native  # noqa: E402
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


def with_alpha(frames):
    """(F, h, w, 3) -> (F, h, w, 4): opaque inside a centred disc"""
    f, h, w, _ = frames.shape
    yy, xx = np.mgrid[0:h, 0:w]
    inside = np.hypot((yy - (h - 1) / 2) / h, (xx - (w - 1) / 2) / w) < 0.42
    alpha = np.broadcast_to(np.where(inside, 255, 0).astype(np.uint8)[None, :, :, None], (f, h, w, 1))
    return np.ascontiguousarray(np.concatenate([frames, alpha], axis=-1))


def report(frames):
    ok, prgba, _, _, _, tidx, msg = p.quantize_rgba_frames(frames, 256, palette_only=False, dither=False, tile_size=0, kmeans_niter=2,
                                                          kmeans_max_samples=65536, want_quantized=False)
    assert ok and tidx == 0, msg
    N = frames.shape[0] * frames.shape[1] * frames.shape[2]
    say("  %d pixels, %.1f %% transparent, %d palette rows" % (N, 100.0 * float(np.mean(frames[..., 3] < 128)), prgba.shape[0]))
    for dither, mapper in ((False, NEAREST), ("ordered", ("k_ordered_map",))):
        call = lambda: p.remap_rgba(frames, prgba, dither=dither)   # noqa: E731
        map_ms, map_text = timed(call, mapper)
        say("  dither=%-9r mapper [%s]   %s" % (dither, " + ".join(mapper), map_text))
        for quad, what in ((-1, "four pixels per lane"), (0, "one pixel per lane  ")):
            _native.lib().patolette_amd_debug_rgba_stamp_quad(quad)
            ms, text = timed(call, ("k_rgba_stamp",))
            _native.lib().patolette_amd_debug_rgba_stamp_quad(-1)
            rate = 10.0 * N / (ms * 1e-3)
            say("  dither=%-9r k_rgba_stamp, %s   %s   %.3f of the mapper; %.0f GB/s = %.1f %% of the HBM peak"
                % (dither, what, text, ms / map_ms, rate / 1e9, 100.0 * rate / HBM_PEAK))


say("ms per call: median (min .. max) of %d calls after %d" % (args.calls, args.warmup))
say("%d x %d scene" % (args.size, args.size))
report(with_alpha(np.round(scene(args.size, args.size, 3) * 255).astype(np.uint8)[None]))
say("64 frames of 640 x 360")
report(with_alpha(delta_ref.clip(360, 640, 64)))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
