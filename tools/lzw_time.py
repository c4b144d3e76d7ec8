"""Kernel times of gif_lzw (k_lzw_segments, k_lzw_offsets, k_lzw_pack) and the size its segments cost, beside the stages before it.

Per call the kernels' times are taken from the profile (patolette_amd_profile_*); reported: the median over --calls calls after
--warmup calls, and the spread (min .. max).  Content: the clip of tests/delta_ref.py, 64 frames of 640 x 360, on the ordered maps of
a quantize_frames(clip, 255) call, in three forms -- its deltas at tolerance 0, its deltas at tolerance 0.05 (both with their dirty
rectangles), and the full maps -- with k_ordered_map and k_frame_deltas of the same clip from the same session; then 2 frames of
4096 x 4096 (the scene of tests/util.py on a 256-row palette, nearest maps).  For the segments 2048 .. 65536 the size of the streams is
given relative to the reference encoder of tests/lzw_ref.py with one segment per frame (which the device's own one-segment streams
must equal in size).  Where PIL is installed, the wall time of its own GIF save of the same frames stands beside the clip's figures:
the CPU figure of a different coder with no segments, not a parity target.

    python tools/lzw_time.py [--calls 12] [--warmup 3] [--no-big] [--out FILE]"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
import patolette_amd as p  # noqa: E402
from tests import delta_ref, lzw_ref  # noqa: E402
from tests.util import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-big", action="store_true", help="leave out the 2 frames of 4096 x 4096")
ap.add_argument("--out", default=None)
args = ap.parse_args()

KERNELS = ("k_lzw_segments", "k_lzw_offsets", "k_lzw_pack")
SEGMENTS = (2048, 4096, 8192, 16384, 65536)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, names):
    """per name the median and its text over the calls, per call"""
    per_call = {k: [] for k in names}
    for i in range(args.warmup + args.calls):
        p.profile(True)
        fn()
        res = p.profile_results()
        p.profile(False)
        if i >= args.warmup:
            for k in names:
                per_call[k].append(res[k]["total_ms"] if k in res else 0.0)
    return {k: (statistics.median(v), "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))) for k, v in per_call.items()}


def lzw_rows(maps, rects, m, one_segment_bytes, yardstick_ms):
    for segment in SEGMENTS:
        out = []
        t = timed(lambda: out.append(p.gif_lzw(maps, rects, m, segment)), KERNELS)
        ok, data, offsets, msg = out[-1]
        assert ok, msg
        total = sum(t[k][0] for k in KERNELS)
        note = "" if one_segment_bytes is None else "; %d bytes = %+.2f %% on one segment per frame" % (
            data.size, 100.0 * (data.size / one_segment_bytes - 1.0))
        if yardstick_ms:
            note += "; the three = %.2f x k_ordered_map" % (total / yardstick_ms)
        say("  segment %5d%s  k_lzw_segments %s + k_lzw_offsets %s + k_lzw_pack %s%s"
            % (segment, " (default)" if segment == 8192 else "          ", t["k_lzw_segments"][1], t["k_lzw_offsets"][1], t["k_lzw_pack"][1], note))


def reference_bytes(maps, rects, m):
    """the reference encoder with one segment per frame; the device's one-segment streams must have its size"""
    t0 = time.time()
    data, offsets = lzw_ref.encode_frames(maps, rects, m, 1 << 24)
    ok, dev, dev_offsets, msg = p.gif_lzw(maps, rects, m, 1 << 24)
    assert ok and np.array_equal(dev_offsets, offsets) and np.array_equal(dev, data), msg
    say("  reference encoder, one segment per frame: %d bytes (%.1f s of one CPU core in Python; the device's bytes are the same)"
        % (data.size, time.time() - t0))
    return data.size


say("ms per call: median (min .. max) of %d calls after %d" % (args.calls, args.warmup))
frames = delta_ref.clip(360, 640, 64)
ok, pal8, maps, _, palf, msg = p.quantize_frames(frames, 255, dither="ordered", tile_size=0, kmeans_niter=2, kmeans_max_samples=65536,
                                                 want_quantized=False)
assert ok, msg
say("64 frames of 640 x 360, 255 rows, ordered maps")
ordered = timed(lambda: p.remap(frames, palf, dither="ordered", want_quantized=False), ("k_ordered_map",))["k_ordered_map"]
say("  k_ordered_map of the clip                 %s" % ordered[1])
forms = []
for tolerance in (0.0, 0.05):
    out = []
    t = timed(lambda: out.append(p.frame_deltas(maps, pal8, transparent_index=255, frames=frames, tolerance=tolerance)), ("k_frame_deltas",))
    ok, deltas, rects, changed, _, msg = out[-1]
    assert ok, msg
    say("  k_frame_deltas of the clip, tolerance %-4g %s   (%.1f %% of the positions change, the rectangles hold %.1f %% of them)"
        % (tolerance, t["k_frame_deltas"][1], 100.0 * changed.sum() / maps.size,
           100.0 * np.sum(rects[:, 2].astype(np.int64) * rects[:, 3]) / maps.size))
    forms.append(("deltas at tolerance %g, in their rectangles" % tolerance, deltas, rects))
forms.append(("the full maps", maps, None))
for what, m8, rects in forms:
    say(" %s" % what)
    lzw_rows(m8, rects, 8, reference_bytes(m8, rects, 8), ordered[0])
try:
    import PIL
    from PIL import Image
    ims = []
    for f in range(maps.shape[0]):
        im = Image.fromarray(maps[f])
        im.putpalette(pal8.tobytes())                                # (mode L becomes mode P)
        ims.append(im)
    best = None
    for _ in range(3):
        sink = io.BytesIO()
        t0 = time.time()
        ims[0].save(sink, format="GIF", save_all=True, append_images=ims[1:], optimize=False, duration=40, loop=0)
        best = min(best or 1e9, time.time() - t0)
    say(" PIL %s, Image.save of the same 64 maps as a GIF (its own coder and frame differencing, one CPU core): %.1f ms wall, %d bytes"
        % (PIL.__version__, 1e3 * best, sink.getbuffer().nbytes))
except ImportError:
    say(" PIL is not installed: no CPU figure")
if not args.no_big:
    img = np.round(scene(4096, 4096, 3) * 255).astype(np.uint8)
    big = np.stack([img, img[::-1].copy()])
    ok, bpal, _, _, _, msg = p.quantize_u8(img, 256, dither=False, tile_size=0, kmeans_niter=2, kmeans_max_samples=65536, want_quantized=False)
    assert ok, msg
    ok, bmaps, _, msg = p.remap(big, bpal, dither=False, want_quantized=False)
    assert ok, msg
    say("2 frames of 4096 x 4096, 256 rows, nearest maps")
    lzw_rows(bmaps, None, 8, None, None)
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
