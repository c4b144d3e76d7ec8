"""The streaming sweeps of a split round (quant.hip: k_minmax, k_hist / k_hist_fix, k_count, k_scatter_bin) at the shapes where their
fetch and store code takes another path: an odd pixel count (planes not 16-byte aligned to each other), one tile, a tile boundary
and a one-pixel tail tile, either side of the 2^18 pixels at which the global quantiser's histogram changes kernels, palettes whose
nodes start at odd offsets and shrink to a pixel or two, weights, both colour spaces, posterised content (the degenerate-node
bucket rule and the wave-combine branch of the histogram) and the tiling-invariant sums of the sliced entry points.

One image is dealt out over two ranks (`patolette_amd_slice`) at an odd boundary, with slices beyond the size at which the partition
kernel takes its last-use loads, and held to the single-GPU result.  Every other case goes through `quantize` and is held to the
existing machinery: the device-driven split loop takes the host-driven loop's
decisions record for record, and the palette (1e-9 relative) and the index map (bit for bit) are the oracle's.  The content is noise
or `tests.util.scene`; that the oracle ALONE is tie-free on every such case is checked on the CPU (the unmarked test below)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tie_prover as tp
from tests.test_gpu_split_loop import _same_decisions
from tests.test_tie_prover import content, run
from tests.util import ROOT, scene

# (name, width, height, content, K, colour space, weighted)
CASES = [
    ("odd pixel count", 97, 61, "noise", 16, 2, False),
    ("odd pixel count, weighted CIELuv", 97, 61, "scene", 16, 1, True),
    ("one tile less a pixel", 8191, 1, "noise", 16, 2, False),
    ("one tile", 128, 64, "noise", 16, 2, True),
    ("one tile and a one-pixel tail", 2731, 3, "noise", 16, 2, False),
    ("two tiles less a pixel", 5461, 3, "noise", 16, 1, False),
    ("two tiles and a one-pixel tail", 3277, 5, "noise", 16, 2, True),
    ("below 2^18 pixels", 511, 513, "noise", 16, 2, False),
    ("above 2^18 pixels", 512, 513, "noise", 16, 2, False),
    ("above 2^18 pixels, weighted CIELuv", 512, 513, "noise", 16, 1, True),
    ("K = 2", 300, 200, "scene", 2, 2, False),
    ("K = 3", 301, 199, "scene", 3, 1, True),
    ("K = 16", 299, 201, "scene", 16, 2, True),
    ("K = 256: nodes of a pixel or two", 300, 200, "scene", 256, 2, False),
    ("K = 256, weighted CIELuv", 303, 197, "scene", 256, 1, True),
]
IDS = [c[0] for c in CASES]
# the images of the tests further down: (width, height, weighted) beyond the Infinity Cache; the invariant-sums image
BEYOND = [(2399, 2401, False), (2049, 2051, True)]
INV_SMALL = (301, 199, 64, 2)


def _beyond_inputs(w, h, weighted):
    rng = np.random.default_rng(5)
    colors = rng.random((w * h, 3))
    return colors, (1.0 + 3.0 * rng.random(w * h)) if weighted else None


def _inv_small_inputs(weighted):
    w, h, K, cs = INV_SMALL
    rng = np.random.default_rng(91)
    colors = np.ascontiguousarray(scene(h, w, 3).reshape(-1, 3))
    return colors, (1.0 + 3.0 * rng.random(w * h)) if weighted else None


def _inputs(case):
    name, w, h, kind, K, cs, weighted = case
    rng = np.random.default_rng(4000 + CASES.index(case))
    colors = rng.random((w * h, 3)) if kind == "noise" else scene(h, w, 7 + CASES.index(case)).reshape(-1, 3)
    wts = (1.0 + 3.0 * rng.random(w * h)) if weighted else None
    return w, h, np.ascontiguousarray(colors), wts, K, cs


@pytest.fixture
def loop(gpu):
    first = []

    def set_mode(on_device):
        prev = gpu.patolette_amd_set_split_loop(on_device)
        if not first:
            first.append(prev)
    yield set_mode
    if first:
        gpu.patolette_amd_set_split_loop(first[0])


def _quantize(p, native, w, h, colors, K, cs, wts):
    ok, pal, pmap, msg = p.quantize(w, h, colors, K, dither=False, color_space=cs, tile_size=0, kmeans_niter=0, weights=wts)
    assert ok, msg
    return pal, pmap, native.last_split_trace()


def _is_oracles(pal, pmap, pal_o, map_o):
    rel = float(np.max(np.abs(pal - pal_o))) / max(1e-300, float(np.max(np.abs(pal_o))))
    return rel <= 1e-9 and np.array_equal(pmap, map_o)


def _tie_free_inputs(which):
    if which in CASES:
        return _inputs(which)
    if which[0] == "beyond":
        _, w, h, weighted = which
        return (w, h) + _beyond_inputs(w, h, weighted) + (16, 2)
    w, h, K, cs = INV_SMALL
    return (w, h) + _inv_small_inputs(which[1]) + (K, cs)


ORACLE_CASES = CASES + [("beyond",) + b for b in BEYOND] + [("invariant", False), ("invariant", True)]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=IDS + ["beyond %dx%d" % b[:2] for b in BEYOND] + ["invariant", "invariant weighted"])
def test_the_oracle_alone_is_tie_free_on_the_edge_cases(ob, case):
    """both summation orders of the oracle take the same decisions and find the same centres: what the GPU tests below demand of the
    HIP path (the oracle's palette and map, exactly) is then a fair demand.  Every image a GPU test compares with the oracle is here"""
    w, h, colors, wts, K, cs = _tie_free_inputs(case)
    data = tp.converted(ob, ob.planar(colors), cs)
    ra, ta = run(ob, data, wts, w * h, K)
    rb, tb = run(ob, data, wts, w * h, K, reversed_sums=1)
    assert tp.first_divergence(ta, tb) is None
    # a centre is a mean of at most n values: the two orders of the sequential f64 sum differ by at most n * 2^-53 of the largest
    # (3e-11 at the largest case) -- a tenth of the 1e-9 the GPU test allows the palette
    ca, cb = np.nan_to_num(ra["centers"]), np.nan_to_num(rb["centers"])
    assert np.array_equal(np.isnan(ra["centers"]), np.isnan(rb["centers"]))
    assert float(np.max(np.abs(ca - cb))) <= 1e-10 * float(np.max(np.abs(ca)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sweeps_at_their_edges(gpu, native, ob, loop, case):
    import patolette_amd as p
    w, h, colors, wts, K, cs = _inputs(case)
    loop(0)
    pal_h, map_h, tr_h = _quantize(p, native, w, h, colors, K, cs, wts)
    loop(1)
    pal_d, map_d, tr_d = _quantize(p, native, w, h, colors, K, cs, wts)
    assert _same_decisions(tr_h, tr_d)
    assert np.array_equal(pal_h, pal_d) and np.array_equal(map_h, map_d)
    ec, pal_o, map_o = ob.patolette(w, h, ob.planar(colors), wts, K, dither=False, color_space=cs, kmeans_niter=0)
    assert ec == 0
    assert _is_oracles(pal_d, map_d, pal_o, map_o)


@pytest.mark.gpu
def test_posterised_content_is_the_oracles_or_a_proven_tie(gpu, native, ob, loop):
    """few distinct colours: degenerate nodes (buckets by pixel position) and whole wavefronts in one bucket (the histogram's
    wave-combine branch).  The oracle's own decisions are ties here, so: identical, or every decision proven by tests/tie_prover.py"""
    import patolette_amd as p
    w, h, K, cs = 173, 131, 64, 2
    colors = np.ascontiguousarray(content(np.random.default_rng(77), "post", h, w))
    results = []
    for on_device in (0, 1):
        loop(on_device)
        results.append(_quantize(p, native, w, h, colors, K, cs, None))
    (pal_h, map_h, tr_h), (pal_d, map_d, tr_d) = results
    assert _same_decisions(tr_h, tr_d)
    assert np.array_equal(pal_h, pal_d) and np.array_equal(map_h, map_d)
    ec, pal_o, map_o = ob.patolette(w, h, ob.planar(colors), None, K, dither=False, color_space=cs, kmeans_niter=0)
    assert ec == 0
    if not _is_oracles(pal_d, map_d, pal_o, map_o):
        why = tp.explain_divergence(ob, native, gpu, w, h, ob.planar(colors), None, K, cs, False, 0, 512 ** 2, pal_d, map_d)
        print("proven tie:", why["first"])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,weighted,invariant", [BEYOND[0] + (False,), BEYOND[0] + (True,), BEYOND[1] + (False,), BEYOND[1] + (True,)])
def test_images_beyond_the_infinity_cache_take_the_last_use_loads(gpu, native, ob, loop, w, h, weighted, invariant):
    """source and destination planes together above 256 MiB (launch_partition): the partition kernel reads its pixels and bucket ids
    non-temporally -- the smallest such images, an odd pixel count, with and without weights, default and tiling-invariant sums (all
    four forms of the kernel): both split loops, the oracle"""
    import patolette_amd as p
    assert 2 * (4 if weighted else 3) * w * h * 8 > 256 << 20
    colors, wts = _beyond_inputs(w, h, weighted)
    gpu.patolette_amd_set_invariant_sums(1 if invariant else 0)
    try:
        loop(0)
        pal_h, map_h, tr_h = _quantize(p, native, w, h, colors, 16, 2, wts)
        loop(1)
        pal_d, map_d, tr_d = _quantize(p, native, w, h, colors, 16, 2, wts)
    finally:
        gpu.patolette_amd_set_invariant_sums(0)
    assert _same_decisions(tr_h, tr_d)
    assert np.array_equal(pal_h, pal_d) and np.array_equal(map_h, map_d)
    ec, pal_o, map_o = ob.patolette(w, h, ob.planar(colors), wts, 16, dither=False, color_space=2, kmeans_niter=0)
    assert ec == 0
    assert _is_oracles(pal_d, map_d, pal_o, map_o)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
def test_tiling_invariant_sums_at_an_odd_pixel_count(gpu, native, ob, weighted):
    """patolette_amd_set_invariant_sums(1): the partition kernel in the form the sliced entry points use (every product split onto
    the exact grids before it is added) -- the oracle's palette and map as well"""
    import patolette_amd as p
    w, h, K, cs = INV_SMALL
    colors, wts = _inv_small_inputs(weighted)
    gpu.patolette_amd_set_invariant_sums(1)
    try:
        pal, pmap, _ = _quantize(p, native, w, h, colors, K, cs, wts)
    finally:
        gpu.patolette_amd_set_invariant_sums(0)
    ec, pal_o, map_o = ob.patolette(w, h, ob.planar(colors), wts, K, dither=False, color_space=cs, kmeans_niter=0)
    assert ec == 0
    assert _is_oracles(pal, pmap, pal_o, map_o)


@pytest.mark.gpu
@pytest.mark.parametrize("weights", ["unweighted", "weighted"])
def test_sliced_image_at_an_odd_boundary_beyond_the_infinity_cache(gpu, tmp_path, weights):
    """patolette_amd_slice over two ranks (gloo; they share the GPU), slices of 5 600 001 and 5 600 002 pixels: the per-slice pixel
    count and offset, the cross-rank reductions, and k_scatter_bin in its tiling-invariant form with last-use loads -- every rank's
    palette and its part of the index map equal the whole image quantised on one GPU, bit for bit (tests/sweep_slice_worker.py)"""
    out = tmp_path / "slice"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29661" if weights == "weighted" else "29660", os.path.join(ROOT, "tests", "sweep_slice_worker.py"), str(out), weights]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in range(2):
        text = open("%s.%d" % (out, rank)).read()
        assert text.startswith("OK"), text
