"""Kernel time of ColorHistogram.add (k_hist_add, with k_hist_units ahead of it in a weighted table) beside the nearest remap of the
same pixels -- another one-pass u8 kernel -- and the time of export and palette(256) at the number of colours of each input.

Per call the kernels' times are taken from the profile (patolette_amd_profile_*); reported: the median over --calls calls after
--warmup calls, and the spread (min .. max).  Inputs: the clip of tests/delta_ref.py (64 frames of 640 x 360), and at --size x --size
uniform noise, the synthetic scene of tests/util.py and one colour.  "Mpx/s" is pixels per second of k_hist_add; for noise nearly
every pixel ends as one global 64-bit atomic add (a block meets few repeats among 2^24 keys), so there it is the atomic rate.
The load rate of the same kernel is taken from RGBA noise whose every pixel is skipped by alpha (nothing is added).
For the clip also: quantize_frames split into palette stage and the rest, and the PSNR of the nearest remap onto the histogram's
palette beside that onto quantize_frames' palette.  --lib: a build made with `make VARIANT=name`.

    python tools/hist_time.py [--size 4096] [--calls 12] [--warmup 3] [--lib PATH] [--quick] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

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
ap.add_argument("--lib", default=None)
ap.add_argument("--quick", action="store_true", help="the add timings only")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.lib:
    _native.LIB_PATH = os.path.abspath(args.lib)

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


def wall(fn, calls=5):
    out, ms = None, []
    for _ in range(calls):
        t = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return out, statistics.median(ms)


def report(px, what, pal8):
    N = px.size // px.shape[-1]
    remap_ms, remap_text = timed(lambda: p.remap(px, pal8, dither=False, want_quantized=False), NEAREST)
    with p.ColorHistogram() as h:
        ms, text = timed(lambda: h.add(px), ("k_hist_add",))
        say("  %-28s k_hist_add %s   %6.0f Mpx/s   nearest remap %s   add = %.2f of it" % (what, text, N / ms / 1e3, remap_text, ms / remap_ms))
        if args.quick:
            return
        m = h.colors
        _, ex_ms = wall(h.export)
        _, ex_k = timed(h.export, ("k_hist_totals", "k_hist_export_count", "k_hist_export_write"))
        (ok, _, _, msg), pal_ms = wall(lambda: h.palette(256))
        assert ok, msg
        st = p.last_stats()
        say("  %-28s M = %d colours: export %.2f ms wall (kernels %s); palette(256) %.2f ms wall (its quantiser call: %.2f ms, KMeans %.2f)"
            % ("", m, ex_ms, ex_k, pal_ms, st["ms_total"], st["ms_kmeans"]))
    if what.startswith("scene"):
        w = 0.5 + np.random.default_rng(1).random(px.shape[:-1])
        with p.ColorHistogram(weighted=True) as h:
            ms, text = timed(lambda: h.add(px, weights=w), ("k_hist_add",))
            _, utext = timed(lambda: h.add(px, weights=w), ("k_hist_units",))
            say("  %-28s k_hist_add %s + k_hist_units %s" % (what + ", weighted", text, utext))


say("ms per call: median (min .. max) of %d calls after %d; library %s" % (args.calls, args.warmup, os.path.relpath(_native.LIB_PATH, ROOT)))
S = args.size
rng = np.random.default_rng(7)
frames = delta_ref.clip(360, 640, 64)
img = np.round(scene(S, S, 3) * 255).astype(np.uint8)
ok, pal8, _, _, _, msg = p.quantize_u8(img, 256, dither=False, tile_size=0, kmeans_niter=2, kmeans_max_samples=65536, want_quantized=False)
assert ok, msg
one = np.empty((S, S, 3), dtype=np.uint8)
one[:] = (90, 140, 200)
report(frames, "64 frames of 640 x 360", pal8)
report(rng.integers(0, 256, (S, S, 3), dtype=np.uint8), "noise %d^2" % S, pal8)
report(img, "scene %d^2" % S, pal8)
report(one, "one colour %d^2" % S, pal8)
# the same kernel's load rate: every pixel skipped by alpha, against every pixel entering
rgba = rng.integers(0, 256, (S, S, 4), dtype=np.uint8)
with p.ColorHistogram() as h:
    for alpha, what in ((0, "every pixel skipped"), (255, "every pixel enters")):
        rgba[..., 3] = alpha
        ms, text = timed(lambda: h.add(rgba, alpha_threshold=1), ("k_hist_add",))
        say("  %-28s k_hist_add %s   %6.0f Mpx/s" % ("RGBA noise, " + what, text, S * S / ms / 1e3))
if not args.quick:
    kw = dict(tile_size=0, kmeans_niter=32, kmeans_max_samples=512 ** 2)
    (ok, fpal8, _, _, fpal, msg), q_ms = wall(lambda: p.quantize_frames(frames, 256, dither=False, want_quantized=False, **kw), 3)
    assert ok, msg
    st = p.last_stats()
    stage = st["ms_convert"] + st["ms_gq"] + st["ms_lq"] + st["ms_kmeans"]
    say("clip: quantize_frames(256, dither=False, want_quantized=False) %.2f ms wall: palette stage %.2f ms (convert %.2f, quantisers %.2f, "
        "KMeans %.2f), the rest %.2f ms (upload %.2f, map %.2f, download %.2f)"
        % (q_ms, stage, st["ms_convert"], st["ms_gq"] + st["ms_lq"], st["ms_kmeans"], st["ms_total"] - stage, st["ms_upload"], st["ms_map"],
           st["ms_download"]))
    with p.ColorHistogram() as h:
        for i in range(0, 64, 8):                                       # the clip in chunks of 8 frames
            h.add(frames[i:i + 8])
        ok, hpal8, hpal, msg = h.palette(256, kmeans_niter=32, kmeans_max_samples=512 ** 2)
        assert ok, msg
    for name, pal in (("histogram palette", hpal), ("quantize_frames palette", fpal)):
        ok, maps, _, msg = p.remap(frames, pal, dither=False, want_quantized=False)
        assert ok, msg
        ok, _, per, _, msg = p.measure(frames, maps, pal, ictcp=False)
        assert ok, msg
        say("clip: nearest remap onto the %-24s PSNR %.3f dB" % (name, float(p.psnr(per.sum(axis=0) * [1, 1, 0]))))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
