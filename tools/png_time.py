"""Kernel times of png_deflate (k_png_filter, k_deflate_segments, k_lzw_offsets, k_lzw_pack) and the size its segments cost, beside the
LZW stage, the ordered map and PIL's PNG save of the same maps.

Per call the kernels' times are taken from the profile (patolette_amd_profile_*); reported: the median over --calls calls after
--warmup calls, and the spread (min .. max).  Content, as tools/lzw_time.py: the clip of tests/delta_ref.py, 64 frames of 640 x 360,
on the ordered maps of a quantize_frames(clip, 255) call, in three forms -- its deltas at tolerance 0, its deltas at tolerance 0.05
(both with their dirty rectangles), and the full maps -- with k_ordered_map and k_lzw_segments of the same inputs from the same
session; then 2 frames of 4096 x 4096 (the scene of tests/util.py on a 256-row palette, nearest maps).  For the segments 4096 ..
32768 the size of the streams is given relative to zlib level 6 of the same filtered streams and to the coder's own size at 32768.
Where PIL is installed, the wall time and bytes of its PNG save of the same maps on one core, at its default level, stand beside them.
Then the ratios to zlib level 6 on the six maps of tests/test_gpu_png.py at the default segment.

    python tools/png_time.py [--calls 12] [--warmup 3] [--no-big] [--out FILE]"""
import argparse
import io
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
import patolette_amd as p  # noqa: E402
from tests import delta_ref, png_ref  # noqa: E402
from tests.util import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-big", action="store_true", help="leave out the 2 frames of 4096 x 4096")
ap.add_argument("--out", default=None)
args = ap.parse_args()

KERNELS = ("k_png_filter", "k_deflate_segments", "k_lzw_offsets", "k_lzw_pack")
SEGMENTS = (4096, 8192, 16384, 32768)
DEFAULT = 16384
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


def zlib_bytes(maps, rects, level=6):
    return int(png_ref.zlib_png_deflate(maps, rects, None, level)[1].size)


def rows(maps, rects, yardsticks):
    t0 = time.time()
    ref = zlib_bytes(maps, rects)
    say("  zlib level 6 of the same filtered streams: %d bytes (%.0f ms of one CPU core)" % (ref, 1e3 * (time.time() - t0)))
    sizes = {}
    for segment in reversed(SEGMENTS):
        out = []
        t = timed(lambda: out.append(p.png_deflate(maps, rects, segment)), KERNELS)
        ok, data, offsets, adler, msg = out[-1]
        assert ok, msg
        sizes[segment] = data.size
        total = sum(t[k][0] for k in KERNELS)
        note = "; %d bytes = %.3f x zlib, %+.2f %% on segment 32768" % (data.size, data.size / ref, 100.0 * (data.size / sizes[32768] - 1.0))
        note += "; the four = %.3f ms" % total + "".join(", %.2f x %s" % (total / ms, name) for name, ms in yardsticks if ms)
        say("  segment %5d%s  k_deflate_segments %s + k_png_filter %s + k_lzw_offsets %s + k_lzw_pack %s%s"
            % (segment, " (default)" if segment == DEFAULT else "          ", t["k_deflate_segments"][1], t["k_png_filter"][1], t["k_lzw_offsets"][1],
               t["k_lzw_pack"][1], note))
    png_ref.check_streams(maps, rects, data, offsets, adler)


def lzw_ms(maps, rects):
    return timed(lambda: p.gif_lzw(maps, rects, 8), ("k_lzw_segments",))["k_lzw_segments"]


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
    ok, deltas, rects, changed, _, msg = p.frame_deltas(maps, pal8, transparent_index=255, frames=frames, tolerance=tolerance)
    assert ok, msg
    rects = p._gif_rects(rects, maps.shape[0], maps.shape[1], maps.shape[2])
    forms.append(("deltas at tolerance %g, in their rectangles" % tolerance, deltas, rects))
forms.append(("the full maps", maps, None))
for what, m8, rects in forms:
    lzw = lzw_ms(m8, rects)
    say(" %s; k_lzw_segments of the same (segment 8192): %s" % (what, lzw[1]))
    rows(m8, rects, (("k_lzw_segments", lzw[0]), ("k_ordered_map", ordered[0])))
try:
    import PIL
    from PIL import Image
    best, size = None, 0
    for _ in range(3):
        t0 = time.time()
        size = 0
        for f in range(maps.shape[0]):
            im = Image.fromarray(maps[f])
            im.putpalette(pal8.tobytes())
            sink = io.BytesIO()
            im.save(sink, format="PNG")
            size += sink.getbuffer().nbytes
        best = min(best or 1e9, time.time() - t0)
    say(" PIL %s, Image.save of the same 64 full maps as 64 PNG files (one CPU core, its default level): %.1f ms wall, %d bytes"
        % (PIL.__version__, 1e3 * best, size))
except ImportError:
    Image = None
    say(" PIL is not installed: no CPU figure")
if not args.no_big:
    img = np.round(scene(4096, 4096, 3) * 255).astype(np.uint8)
    big = np.stack([img, img[::-1].copy()])
    ok, bpal, _, _, _, msg = p.quantize_u8(img, 256, dither=False, tile_size=0, kmeans_niter=2, kmeans_max_samples=65536, want_quantized=False)
    assert ok, msg
    ok, bmaps, _, msg = p.remap(big, bpal, dither=False, want_quantized=False)
    assert ok, msg
    lzw = lzw_ms(bmaps, None)
    say("2 frames of 4096 x 4096, 256 rows, nearest maps; k_lzw_segments of the same (segment 8192): %s" % lzw[1])
    rows(bmaps, None, (("k_lzw_segments", lzw[0]),))
    if Image is not None:
        im = Image.fromarray(bmaps[0])
        im.putpalette(bpal.tobytes())
        sink = io.BytesIO()
        t0 = time.time()
        im.save(sink, format="PNG")
        say(" PIL's PNG save of ONE of the two 4096 x 4096 maps: %.1f ms wall, %d bytes" % (1e3 * (time.time() - t0), sink.getbuffer().nbytes))
say("the maps of tests/test_gpu_png.py, 640 x 360, default segment: bytes / zlib level 6")
from tests.test_gpu_png import _size_maps  # noqa: E402
for name, m in _size_maps().items():
    ok, data, offsets, adler, msg = p.png_deflate(m)
    assert ok, msg
    ref = zlib_bytes(m[None], None)
    say("  %-10s %7d bytes, zlib level 6 %7d, ratio %.4f" % (name, data.size, ref, data.size / ref))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
