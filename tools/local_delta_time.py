"""Kernel time of the frame deltas with a colour table per frame (k_frame_deltas_local) beside k_frame_deltas on the same maps.

The workloads and the statistic of tools/delta_time.py: the clip of tests/delta_ref.py -- 64 frames of 640 x 360 and 2 frames of
4096 x 4096 -- on the ordered maps of a quantize_frames(clip, 255) call; per call the kernel's time from the profile, the median over
--calls calls after --warmup calls and the spread.  The local entry gets the same palette as P = 1 table and as P = F copies of it,
so every decision is the sibling's and only the table look-ups differ; the P = 1 case also with the rows forced into global memory.
Then the end-to-end clip: two scenes of three frames at 640 x 360, 16 colours, one palette against a palette per scene -- PSNR of what
a viewer shows against the source, and the two file sizes.

    python tools/local_delta_time.py [--calls 12] [--warmup 3] [--tolerance 0.05] [--skip-large] [--out FILE]"""
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
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--tolerance", type=float, default=0.05)
ap.add_argument("--skip-large", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, name, also):
    per_call, others = [], []
    for i in range(args.warmup + args.calls):
        p.profile(True)
        fn()
        res = p.profile_results()
        p.profile(False)
        if i >= args.warmup:
            per_call.append(res[name]["total_ms"])
            others.append(res[also]["total_ms"])
    return "%.3f (%.3f .. %.3f) + %s %.3f (%.3f .. %.3f)" % (statistics.median(per_call), min(per_call), max(per_call), also,
                                                           statistics.median(others), min(others), max(others))


say("ms per call: median (min .. max) of %d calls after %d" % (args.calls, args.warmup))
L = _native.lib()
for F, h, w in ((64, 360, 640),) + (() if args.skip_large else ((2, 4096, 4096),)):
    frames = delta_ref.clip(h, w, F)
    ok, pal8, maps, _, _, msg = p.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2, kmeans_max_samples=65536,
                                                  want_quantized=False)
    assert ok, msg
    say("%d frames of %d x %d, one-byte elements, 255 rows" % (F, w, h))
    for tolerance in (0.0, args.tolerance):
        out = []
        text = timed(lambda: out.append(p.frame_deltas(maps, pal8, frames=frames, tolerance=tolerance)), "k_frame_deltas", "k_delta_boxes")
        assert out[-1][0], out[-1][-1]
        say("  tolerance %-4g k_frame_deltas                          %s" % (tolerance, text))
        for label, pals, of, route, shown in (("P = 1", pal8[None], [0] * F, -1, False), ("P = 1, rows in global memory", pal8[None], [0] * F, 0, False),
                                              ("P = F", np.stack([pal8] * F), None, -1, False), ("P = F, rows in LDS if they fit", np.stack([pal8] * F), None, 1, False),
                                              ("P = 1 with shown_rgb", pal8[None], [0] * F, -1, True)):
            L.patolette_amd_debug_delta_local_tables(route)
            got = []
            text = timed(lambda: got.append(p.frame_deltas_local(maps, pals, of, frames=frames, tolerance=tolerance, want_shown=shown)),
                         "k_frame_deltas_local", "k_delta_boxes")
            where = "LDS" if L.patolette_amd_debug_delta_local_route() == 1 else "global"
            L.patolette_amd_debug_delta_local_tables(-1)
            assert got[-1][0], got[-1][-1]
            assert np.array_equal(got[-1][1], out[-1][1]) and np.array_equal(got[-1][2], out[-1][2])       # the sibling's deltas and rectangles
            say("  tolerance %-4g k_frame_deltas_local %-30s %s   rows in %s" % (tolerance, label, text, where))

# end to end: one palette against a palette per scene
h, w = 360, 640
rng = np.random.default_rng(11)
clip = []
for seed, invert in ((5, False), (9, True)):
    base = np.round(scene(h, w, seed) * 255).astype(np.int64)
    base = 255 - base if invert else base
    for _ in range(3):
        clip.append(np.clip(base + rng.integers(-2, 3, size=base.shape), 0, 255).astype(np.uint8))
clip = np.stack(clip)
kw = dict(dither=False, tile_size=0, kmeans_niter=2, kmeans_max_samples=65536, want_quantized=False)


def psnr(shown):
    mse = np.mean((shown.astype(np.float64) - clip.astype(np.float64)) ** 2)
    return 10.0 * np.log10(255.0 ** 2 / mse)


ok, pal8, maps, _, _, msg = p.quantize_frames(clip, 16, **kw)
assert ok, msg
ok, d, r, c, s, msg = p.frame_deltas(maps, pal8, want_shown=True)
assert ok, msg
one = p.write_gif(None, d, pal8, r, transparent_index=16)
say("two scenes of three frames, %d x %d, 16 colours, tolerance 0" % (w, h))
say("  one palette:         PSNR %.2f dB, %d bytes" % (psnr(pal8[s]), len(one)))
pals, local = [], []
for part in (clip[:3], clip[3:]):
    ok, p8, m, _, _, msg = p.quantize_frames(part, 16, **kw)
    assert ok, msg
    pals.append(p8)
    local.append(m)
ok, d, r, c, shown, msg = p.frame_deltas_local(np.concatenate(local), np.stack(pals), [0, 0, 0, 1, 1, 1], want_shown=True)
assert ok, msg
two = p.write_gif(None, d, np.stack(pals), r, transparent_index=16, palette_of=[0, 0, 0, 1, 1, 1])
say("  a palette per scene: PSNR %.2f dB, %d bytes" % (psnr(shown), len(two)))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
