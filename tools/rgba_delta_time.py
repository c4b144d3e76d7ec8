"""Kernel times of frame_deltas_rgba (k_rgba_vanish once, k_frame_delta_rgba once per frame) and what its deltas buy in size, beside
k_frame_deltas on the same maps and k_ordered_map on the same clip, all from one session.

Per call the kernels' times are taken from the profile (patolette_amd_profile_*); reported: the median over --calls calls after
--warmup calls, and the spread (min .. max).  Content: the RGBA clip of tests/rgba_delta_ref.py, 64 frames of 640 x 360 on the ordered
maps of a quantize_rgba_frames(clip, 255) call -- with the disc moving in every frame (every frame is then drawn whole: the lossy mode
has nothing to keep) and with the disc resting every second frame --, then 2 frames of 4096 x 4096.  Exact and at tolerance 0.05, with
and without `shown`.  Sizes: the summed rectangle area and the gif_lzw bytes of the deltas, against the full maps written with
disposal 2.

    python tools/rgba_delta_time.py [--calls 12] [--warmup 3] [--no-big] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
import patolette_amd as p  # noqa: E402
from tests import rgba_delta_ref  # noqa: E402
from tests.util import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-big", action="store_true", help="leave out the 2 frames of 4096 x 4096")
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, names):
    """per name (median ms, its text, launches per call) over the calls"""
    per_call, launches = {k: [] for k in names}, {k: 0 for k in names}
    for i in range(args.warmup + args.calls):
        p.profile(True)
        fn()
        res = p.profile_results()
        p.profile(False)
        if i >= args.warmup:
            for k in names:
                per_call[k].append(res[k]["total_ms"] if k in res else 0.0)
                launches[k] = res[k]["launches"] if k in res else 0
    return {k: (statistics.median(v), "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v)), launches[k]) for k, v in per_call.items()}


def stage(what, frames, maps, prgba, yardstick_ms):
    F = maps.shape[0]
    pal8 = prgba[:, :3]
    ok, full, full_offsets, msg = p.gif_lzw(maps, None, 8)
    assert ok, msg
    for tolerance in (0.0, 0.05):
        t = timed(lambda: p.frame_deltas(maps, pal8, transparent_index=255, frames=frames, tolerance=tolerance), ("k_frame_deltas", "k_delta_boxes"))
        say("  %s, tolerance %-4g  yardstick: k_frame_deltas %s + k_delta_boxes %s on the same maps (index 0 as any row)"
            % (what, tolerance, t["k_frame_deltas"][1], t["k_delta_boxes"][1]))
        for want_shown in (False, True):
            out = []
            t = timed(lambda: out.append(p.frame_deltas_rgba(maps, prgba, frames=frames, tolerance=tolerance, want_shown=want_shown)),
                      ("k_rgba_vanish", "k_frame_delta_rgba"))
            ok, deltas, rects, disposals, changed, shown, msg = out[-1]
            assert ok, msg
            total = t["k_rgba_vanish"][0] + t["k_frame_delta_rgba"][0]
            walls = []                                                  # unprofiled: the host's clock from the first launch to the results
            for _ in range(args.calls):
                assert p.frame_deltas_rgba(maps, prgba, frames=frames, tolerance=tolerance, want_shown=want_shown)[0]
                walls.append(p.last_stats()["ms_map"])
            say("  %s, tolerance %-4g shown %d  k_rgba_vanish %s (%d launch) + k_frame_delta_rgba %s (%d launches) = %.3f ms%s; "
                "ms_map without the profile %.3f (%.3f .. %.3f)"
                % (what, tolerance, want_shown, t["k_rgba_vanish"][1], t["k_rgba_vanish"][2], t["k_frame_delta_rgba"][1],
                   t["k_frame_delta_rgba"][2], total, "" if not yardstick_ms else " = %.2f x k_ordered_map" % (total / yardstick_ms),
                   statistics.median(walls), min(walls), max(walls)))
        ok, data, offsets, msg = p.gif_lzw(deltas, rects, 8)
        assert ok, msg
        area = int(np.sum(rects[:, 2].astype(np.int64) * rects[:, 3]))
        say("  %s, tolerance %-4g  %d of %d frames with disposal 2; %.1f %% of the positions change; rectangles hold %d of %d positions "
            "(%.1f %%); gif_lzw: %d bytes as deltas, %d as full maps with disposal 2 (%.2f x)"
            % (what, tolerance, int(np.sum(disposals == 2)), F, 100.0 * changed.sum() / maps.size, area, maps.size, 100.0 * area / maps.size,
               data.size, full.size, data.size / full.size))


say("ms per call: median (min .. max) of %d calls after %d" % (args.calls, args.warmup))
for rest in (1, 2):
    frames = rgba_delta_ref.clip(360, 640, 64, rest=rest)
    ok, prgba, maps, _, palf, tidx, msg = p.quantize_rgba_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2,
                                                                 kmeans_max_samples=65536, want_quantized=False)
    assert ok and tidx == 0, msg
    what = "64 x 640 x 360, disc moves every %s frame" % ("" if rest == 1 else "second")
    say("%s, 255 rows, ordered maps" % what)
    ordered = timed(lambda: p.remap(frames, palf[1:], dither="ordered", want_quantized=False), ("k_ordered_map",))["k_ordered_map"]
    say("  k_ordered_map of the clip's RGB on the opaque rows   %s" % ordered[1])
    stage("clip", frames, maps, prgba, ordered[0])
if not args.no_big:
    img = np.round(scene(4096, 4096, 3) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:4096, 0:4096]
    big = np.empty((2, 4096, 4096, 4), dtype=np.uint8)
    big[0, ..., :3], big[1, ..., :3] = img, img[::-1]
    for f, (cy, cx) in enumerate(((1900, 2000), (2100, 2300))):
        big[f, ..., 3] = np.where((yy - cy) ** 2 + (xx - cx) ** 2 <= 1700 ** 2, 255, 0)
    ok, prgba, maps, _, palf, tidx, msg = p.quantize_rgba_frames(big, 255, dither=False, tile_size=0, kmeans_niter=2, kmeans_max_samples=65536,
                                                                 want_quantized=False)
    assert ok and tidx == 0, msg
    say("2 x 4096 x 4096, a disc of radius 1700 that moves by (200, 300), 255 rows, nearest maps")
    stage("big", big, maps, prgba, None)
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
