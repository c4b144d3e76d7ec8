"""quantize_frames against quantize_u8_batch on the same frames with the same options: median ms per call after the first (host
array in, maps and quantized frames out), the spread of the repetitions, the stage times of the frames call
(patolette_amd_last_stats), the map stage of ONE frame through quantize_u8 (times F: the frame-by-frame dither), and the dither
kernels' times (patolette_amd_profile_*).  Default: 64 frames of 640x360 scene content, K = 256, ICtCp, KMeans 32, tile_size=0,
dither on.  On a checkout without quantize_frames only the batch and single-frame numbers are printed (the yardstick).
usage: frames_time.py [F] [W] [H] [reps]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import patolette_amd as p  # noqa: E402
from tests.util import scene  # noqa: E402

F = int(sys.argv[1]) if len(sys.argv) > 1 else 64
W = int(sys.argv[2]) if len(sys.argv) > 2 else 640
H = int(sys.argv[3]) if len(sys.argv) > 3 else 360
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
K = 256
base = [np.round(scene(H, W, 3 + i) * 255).astype(np.uint8) for i in range(min(F, 8))]
frames = np.ascontiguousarray(np.stack([np.roll(base[i % len(base)], 7 * i, axis=1) for i in range(F)]))
kw = dict(dither=True, color_space=p.ColorSpace_ICtCp, tile_size=0, kmeans_niter=32)


def timed(f, check):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        t.append(1e3 * (time.perf_counter() - t0))
        check(r)
    t = t[1:] if reps > 1 else t
    return float(np.median(t)), float(min(t)), float(max(t))


print("%d frames of %dx%d (%.1f Mpx), K=%d ICtCp KMeans 32 dither: ms per call, median (min .. max) of %d after the first"
      % (F, W, H, F * W * H / 1e6, K, max(1, reps - 1)))
if hasattr(p, "quantize_frames"):
    m = timed(lambda: p.quantize_frames(frames, K, **kw), lambda r: r[0] or sys.exit(r[-1]))
    st = p.last_stats()
    print("(a) quantize_frames    %8.2f (%8.2f .. %8.2f)" % m)
    print("    stages: " + "  ".join("%s %.2f" % (k[3:], v) for k, v in st.items() if k.startswith("ms_")))
    print("    dither: " + "  ".join("%s %d" % (k[7:], v) for k, v in st.items() if k.startswith("dither_")))
m = timed(lambda: p.quantize_u8_batch(list(frames), K, **kw), lambda r: all(x[0] for x in r) or sys.exit("batch failed"))
print("(b) quantize_u8_batch  %8.2f (%8.2f .. %8.2f)" % m)
one_call, one_map = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    r = p.quantize_u8(frames[0], K, **kw)
    one_call.append(1e3 * (time.perf_counter() - t0))
    one_map.append(p.last_stats()["ms_map"])
    assert r[0], r[-1]
mm = float(np.median(one_map[1:] if reps > 1 else one_map))
print("    one frame through quantize_u8: %.2f ms per call, ms_map %.3f, x %d frames = %.2f"
      % (float(np.median(one_call[1:] if reps > 1 else one_call)), mm, F, F * mm))
if hasattr(p, "quantize_frames"):
    p.profile(True)
    for _ in range(3):
        p.quantize_frames(frames, K, **kw)
    print("(c) kernels of the map stage, 3 calls:")
    for name, r in sorted(p.profile_results().items()):
        if name.startswith("k_dither") or name == "k_nn_lut_build":
            print("    %-20s %8.4f ms per launch  x %d" % (name, r["total_ms"] / r["launches"], r["launches"]))
    p.profile(False)
