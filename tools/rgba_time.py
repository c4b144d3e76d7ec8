"""quantize_u8 against quantize_rgba at 0 / 25 / 50 / 90 % transparent pixels: ms per call (host numpy image in, map and
quantized image out), 4096^2 by default, K = 256, ICtCp + KMeans (32 iterations), no saliency weights, dither off and on; then
the new kernels' times and algorithmic bytes of the last configuration (patolette_amd_profile_*).
usage: rgba_time.py [side] [reps]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import patolette_amd as p  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K = 256
rng = np.random.default_rng(5)
yy, xx = np.mgrid[0:side, 0:side].astype(np.float32) / side
rgb = np.stack([255 * xx, 255 * yy, 255 * (1 - xx) * yy], axis=2)
rgb = np.clip(rgb + rng.normal(0, 12, rgb.shape), 0, 255).astype(np.uint8)
noise = rng.random((side // 16, side // 16)).repeat(16, 0).repeat(16, 1)      # blobby alpha: transparency in patches


def med(f):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        t.append(1e3 * (time.perf_counter() - t0))
        assert r[0], r[-1]
    return float(np.median(t[1:] if reps > 1 else t))


kw = dict(color_space=p.ColorSpace_ICtCp, tile_size=0, kmeans_niter=32)
print("%dx%d K=%d ICtCp KMeans 32: median ms per call of %d" % (side, side, K, reps))
for dither in (False, True):
    u8 = med(lambda: p.quantize_u8(rgb, K, dither=dither, **kw))
    line = ["dither %-5s  quantize_u8 %8.2f" % (dither, u8)]
    for frac in (0.0, 0.25, 0.5, 0.9):
        a = np.where(noise < frac, 0, 255).astype(np.uint8)[..., None]
        img = np.ascontiguousarray(np.concatenate([rgb, a], axis=2))
        line.append("rgba %2d%% %8.2f" % (round(100 * frac), med(lambda: p.quantize_rgba(img, K, dither=dither, **kw))))
    print("  ".join(line), flush=True)

p.profile(True)
for frac in (0.0, 0.5):
    a = np.where(noise < frac, 0, 255).astype(np.uint8)[..., None]
    img = np.ascontiguousarray(np.concatenate([rgb, a], axis=2))
    p.profile(True)
    for _ in range(3):
        p.quantize_rgba(img, K, dither=True, **kw)
    print("kernels at %d%% transparent, dither on (3 calls):" % round(100 * frac))
    for name, r in sorted(p.profile_results().items()):
        if name in ("k_alpha_count", "k_alpha_compact", "k_rgba_expand", "k_dither_mask"):
            ms, by = r["total_ms"] / r["launches"], r["bytes"] / r["launches"]
            print("  %-16s %8.4f ms per launch  %8.1f MB  %7.1f GB/s" % (name, ms, by / 1e6, by / ms / 1e6 if ms > 0 else 0.0))
p.profile(False)
