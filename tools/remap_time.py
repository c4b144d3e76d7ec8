"""Kernel time of the map stage: inside quantize_u8 (conversion + map kernels), and for remap of the same image onto that call's
byte palette -- through the route remap takes by default and through the forced two-pass route (patolette_amd_debug_remap_two_pass).

Per call the times of the kernels named below are summed from the profile (patolette_amd_profile_*); reported: the median over
--calls calls after --warmup calls, and the spread (min .. max).  Content: uniform noise and the synthetic scene of tests/util.py at
--size x --size, 256 palette rows.  A package without `remap` (an older commit on PYTHONPATH) reports the quantize_u8 figures alone.

    python tools/remap_time.py [--size 4096] [--calls 12] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                                          # (appended: a package given on PYTHONPATH comes first)
import patolette_amd as p  # noqa: E402
from tests.util import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

NEAREST = ("k_convert_u8", "k_nn_map", "k_nn_map_u8")
DITHER = ("k_convert_u8", "k_convert", "k_dither_gather", "k_dither_gather_u8", "k_dither", "k_dither_fix", "k_dither_unpermute")


def timed(fn, names):
    per_call, seen = [], {}
    for i in range(args.warmup + args.calls):
        p.profile(True)
        fn()
        res = p.profile_results()
        p.profile(False)
        if i >= args.warmup:
            per_call.append(sum(res[k]["total_ms"] for k in names if k in res))
            for k in names:
                if k in res:
                    seen.setdefault(k, []).append(res[k]["total_ms"])
    return dict(median_ms=statistics.median(per_call), min_ms=min(per_call), max_ms=max(per_call),
                kernels={k: statistics.median(v) for k, v in seen.items()})


def contents(n):
    rng = np.random.default_rng(1)
    yield "noise", rng.integers(0, 256, size=(n, n, 3), dtype=np.uint8)
    yield "scene", np.round(scene(n, n, 3) * 255).astype(np.uint8)


rows = []
have_remap = hasattr(p, "remap")
for kind, img in contents(args.size):
    for dither in (False, True):
        names = DITHER if dither else NEAREST
        kw = dict(dither=dither, tile_size=0, kmeans_niter=2, kmeans_max_samples=65536, want_quantized=False)
        ok, pal8, _, _, _, msg = p.quantize_u8(img, 256, **kw)
        assert ok, msg
        rec = dict(content=kind, size=args.size, dither=dither, package=os.path.dirname(p.__file__),
                   quantize_u8=timed(lambda: p.quantize_u8(img, 256, **kw), names))
        if have_remap:
            L = p._native.lib()
            for label, two_pass in (("remap", 0), ("remap_two_pass", 1)):
                L.patolette_amd_debug_remap_two_pass(two_pass)
                rec[label] = timed(lambda: p.remap(img, pal8, dither=dither, want_quantized=False), names)
            L.patolette_amd_debug_remap_two_pass(0)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(rows, fh, indent=1)
