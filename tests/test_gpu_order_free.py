"""Results must not depend on the order of the pixels where the sums are exact: one call on `colors` (with `weights`) against one
on `colors[perm]` (with `weights[perm]`).  Repeating a call, or cutting an image into contiguous slices, leaves every addend
next to the neighbours it always had; a permutation changes which addends meet in a thread, a wavefront, a block, a tile and an
atomic -- an addend off its grid, or a grid whose bound does not hold, then shows in the last bits.

Permutations (fixed seeds): reversal; rotation by one pixel (every pixel changes lane, 16-byte alignment and, at the edges,
tile); a uniform shuffle; ascending by first channel (per-thread partial sums see monotone data: the worst case for a sum that
is secretly sequential).  Content is continuous noise or `tests.util.scene`: no node is degenerate (degenerate nodes bucket by
pixel position, by design).  Shapes are those of tests/test_gpu_sweep_edges.py at which a path changes.

What the DEFAULT mode makes exact under a permutation, and what not (quant.hip, pipeline.hip):

* exact: the trace header -- `n_base`, `n_clusters`, `stopped_early`, `gq_cuts`, and for ICtCp and CIELuv on one GPU `gq_axis` and
  `gq_cov6`, which come from the column sums and raw second moments that ride with the conversion (k_convert: every value and
  every product through `bin_add`); for sRGB the root takes k_sum3 and k_cov_nodes, every product through `bin_add` as well.
  Of every record the integers (`row`, `new_row`, `split`, `degenerate`, `n`, `n_left`, `n_right`) and `sw`: extrema are ordered
  keys, the 512-bucket tables are integer counts and `bin_split` parts, the cut is k_cut's arithmetic on the reduced table.  The
  cluster centres are quotients of such tables.  The index map is a function of the pixel and the palette.
* NOT exact: a record's `dist`, `dist_left`, `dist_right`, `cov6`, and with them `axis` and `benefit`.  k_scatter_bin sums a child's
  seven centred products per THREAD in plain f64 over the pixels that thread moves, and only the per-thread partials go through
  `bin_split` -- deterministic for a given image and tiling, but another order of pixels is another set of partials.  The project
  allows these 1e-12 relative (`_same_decisions` of tests/test_gpu_split_loop.py), far from any decision on tie-free content.
* `patolette_amd_set_invariant_sums(1)` splits every product before it is added (k_scatter_bin<INV>; k_cov_children and
  k_cov_nodes always do): then everything above is exact, and the tests demand every field of the trace bit for bit.

The oracle ALONE is tie-free on every image that is compared with it here, in both of its summation orders: the unmarked test
below (CPU).  tests/test_order_free_model.py holds the model of the sums, and says why test D cannot leave the a-priori bounds."""
import functools

import numpy as np
import pytest

from tests import tie_prover as tp
from tests.test_gpu_split_loop import _same_decisions
from tests.test_gpu_sweep_edges import _is_oracles
from tests.test_order_free_model import BEYOND_H, BEYOND_W, beyond_unit_image
from tests.test_tie_prover import run
from tests.util import scene

PERMS = ("reversal", "rotation", "shuffle", "sorted")
# A: default sums.  (width, height, content, K, colour space, device-driven loop, permutation, weights: 0 none, 3, 1000)
A_CASES = [
    (97, 61, "noise", 16, 2, 1, "shuffle", 0),
    (97, 61, "scene", 256, 1, 0, "sorted", 3),
    (97, 61, "noise", 16, 0, 1, "sorted", 3),
    (2731, 3, "noise", 2, 0, 1, "rotation", 0),
    (2731, 3, "noise", 256, 0, 0, "shuffle", 1000),
    (5461, 3, "noise", 16, 1, 0, "reversal", 0),
    (512, 513, "noise", 16, 2, 1, "sorted", 3),
    (512, 513, "noise", 16, 1, 0, "shuffle", 0),
]
# B: tiling-invariant sums.  (entry, width, height, content, K, colour space, loop, permutation, weights)
B_CASES = [
    ("planar", 97, 61, "scene", 16, 2, 1, "shuffle", 3),
    ("planar", 5461, 3, "noise", 256, 1, 0, "sorted", 0),
    ("rows", 2731, 3, "noise", 16, 0, 1, "rotation", 3),
    ("planar", 512, 513, "noise", 16, 2, 0, "reversal", 0),
    ("planar", 512, 513, "noise", 16, 1, 1, "shuffle", 3),
    ("u8", 97, 61, "u8", 16, 2, 1, "shuffle", 0),
    ("u8", 97, 61, "u8", 16, 1, 0, "sorted", 3),
    ("u8", 2731, 3, "u8", 2, 2, 0, "rotation", 1000),
]
# C: the a-priori edges of the colour spaces, a pixel count either side of 2^16 (rootP 16 and 17)
C_CASES = [(255, 257, 1, 1, "shuffle"), (65537, 1, 1, 0, "sorted"), (255, 257, 2, 0, "sorted"), (65537, 1, 2, 1, "shuffle")]
C_K = 16


def _id(case):
    return "-".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def _inputs(w, h, content, weights):
    """(colors (n, 3) row-major, weights or None), computed once and read-only; the seed is a function of the arguments."""
    n = w * h
    rng = np.random.default_rng(7000 + 13 * w + h + weights)
    if content == "noise":
        colors = rng.random((n, 3))
    elif content == "scene":
        colors = np.ascontiguousarray(scene(h, w, 31).reshape(-1, 3))
    elif content == "u8":
        colors = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    elif content == "corners":
        colors = _corners(n, rng)
    else:
        colors = np.ascontiguousarray(beyond_unit_image(content))
    wts = (1.0 + (weights - 1.0) * rng.random(n)) if weights == 1000 else (1.0 + 3.0 * rng.random(n)) if weights else None
    for a in (colors, wts):
        if a is not None:
            a.setflags(write=False)
    return colors, wts


def _corners(n, rng):
    """The eight corners of the sRGB cube -- white is CIELuv's L = 100, the primaries and secondaries carry its largest |u|, |v|
    and ICtCp's extreme Ct, Cp -- once each exactly, then their neighbourhoods: a corner pulled up to 0.04 into the cube per
    channel, so that every cloud has an extent in every direction and no node is degenerate."""
    corner = rng.integers(0, 2, size=(n, 3)).astype(np.float64)
    corner[:8] = [[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)]
    pull = 0.04 * rng.random((n, 3))
    pull[:8] = 0.0
    return np.ascontiguousarray(corner * (1.0 - pull) + (1.0 - corner) * pull)


@functools.lru_cache(maxsize=None)
def _perm(kind, w, h, content, weights):
    colors, _ = _inputs(w, h, content, weights)
    n = w * h
    if kind == "identity":
        perm = np.arange(n)
    elif kind == "reversal":
        perm = np.arange(n)[::-1].copy()
    elif kind == "rotation":
        perm = np.roll(np.arange(n), 1)
    elif kind == "shuffle":
        perm = np.random.default_rng(99).permutation(n)
    else:
        perm = np.argsort(colors[:, 0], kind="stable")
    perm.setflags(write=False)
    return perm


def _permuted(kind, w, h, content, weights):
    colors, wts = _inputs(w, h, content, weights)
    perm = _perm(kind, w, h, content, weights)
    return np.ascontiguousarray(colors[perm]), (None if wts is None else np.ascontiguousarray(wts[perm])), perm


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


@pytest.fixture
def invariant_sums(gpu):
    prev = gpu.patolette_amd_set_invariant_sums(1)
    yield
    gpu.patolette_amd_set_invariant_sums(prev)


def _call(p, native, entry, w, h, colors, wts, K, cs, niter=0, max_samples=512 ** 2):
    kw = dict(dither=False, color_space=cs, tile_size=0, kmeans_niter=niter, kmeans_max_samples=max_samples, weights=wts)
    if entry == "u8":
        ok, _, pmap, _, pal, msg = p.quantize_u8(colors.reshape(h, w, 3), K, want_quantized=False, **kw)
        pmap = None if pmap is None else pmap.reshape(-1)
    else:
        src = np.asfortranarray(colors) if entry == "planar" else np.ascontiguousarray(colors)
        assert src.flags.f_contiguous != src.flags.c_contiguous
        ok, pal, pmap, msg = p.quantize(w, h, src, K, **kw)
    assert ok, msg
    return dict(pal=np.array(pal), map=np.array(pmap), trace=native.last_split_trace(), centers=native.last_cluster_centers())


def _trace_words(tr):
    """Every field of a split trace, header and records, as one uint64 array: floats by their bits."""
    ints = [tr["n_base"], tr["n_clusters"], int(tr["stopped_early"]), len(tr["splits"])] + list(tr["gq_cuts"])
    flts = list(tr["gq_axis"]) + list(tr["gq_cov6"])
    for r in tr["splits"]:
        ints += [r[k] for k in ("row", "new_row", "split", "degenerate", "n", "n_left", "n_right")]
        flts += [r["sw"], r["dist"], r["dist_left"], r["dist_right"], r["benefit"]] + list(r["axis"]) + list(r["cov6"])
    return np.concatenate([np.array(ints, dtype=np.int64).view(np.uint64), np.array(flts, dtype=np.float64).view(np.uint64)])


def _root_words(tr):
    return np.array(list(tr["gq_axis"]) + list(tr["gq_cov6"]), dtype=np.float64).view(np.uint64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _no_degenerate_node(tr):
    """(K = 2 commits no split at all: the global quantiser's two base clusters are the palette)"""
    return len(tr["splits"]) == max(0, tr["n_clusters"] - tr["n_base"]) and not any(r["degenerate"] for r in tr["splits"])


def _assert_everything_bit_equal(a, b, perm):
    assert _no_degenerate_node(a["trace"])
    assert np.array_equal(_trace_words(a["trace"]), _trace_words(b["trace"]))
    assert np.array_equal(_bits(a["centers"]), _bits(b["centers"]))
    assert np.array_equal(_bits(a["pal"]), _bits(b["pal"]))
    assert np.array_equal(b["map"], a["map"][perm])


# ----------------------------------------------------------------------------------------------------------------------
# 3. the oracle alone is tie-free on every (image, permutation) that is compared with it below (CPU)
# ----------------------------------------------------------------------------------------------------------------------
ORACLE_CASES = [(c[0], c[1], c[2], c[7], c[3], c[4], c[6]) for c in A_CASES] + [(c[0], c[1], "corners", 0, C_K, c[2], c[4]) for c in C_CASES]


@pytest.mark.parametrize("kind", ["identity", "permuted"])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=_id)
def test_the_oracle_alone_is_tie_free_on_every_image_and_permutation(ob, case, kind):
    """both summation orders of the oracle take the same decisions and find the same centres on the image as it is and as tests A
    and C permute it: demanding the oracle's palette and map of the HIP path is then a fair demand"""
    w, h, content, weights, K, cs, perm_kind = case
    colors, wts, _ = _permuted(perm_kind if kind == "permuted" else "identity", w, h, content, weights)
    data = tp.converted(ob, ob.planar(colors), cs)
    ra, ta = run(ob, data, wts, w * h, K)
    rb, tb = run(ob, data, wts, w * h, K, reversed_sums=1)
    assert tp.first_divergence(ta, tb) is None
    assert _no_degenerate_node(ta)
    # a centre is a mean of at most n values: two orders of a sequential f64 sum differ by at most n 2^-53 of the largest
    # (3e-11 at 512 x 513) -- a tenth of the 1e-9 the GPU tests allow the palette
    ca, cb = np.nan_to_num(ra["centers"]), np.nan_to_num(rb["centers"])
    assert np.array_equal(np.isnan(ra["centers"]), np.isnan(rb["centers"]))
    assert float(np.max(np.abs(ca - cb))) <= 1e-10 * float(np.max(np.abs(ca)))


# ----------------------------------------------------------------------------------------------------------------------
# A. default sums
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", A_CASES, ids=_id)
def test_default_sums_take_the_same_decisions_for_any_pixel_order(gpu, native, ob, loop, case):
    import patolette_amd as p
    w, h, content, K, cs, on_device, perm_kind, weights = case
    colors, wts = _inputs(w, h, content, weights)
    colors_p, wts_p, perm = _permuted(perm_kind, w, h, content, weights)
    loop(on_device)
    a = _call(p, native, "rows", w, h, colors, wts, K, cs)
    b = _call(p, native, "rows", w, h, colors_p, wts_p, K, cs)
    assert _no_degenerate_node(a["trace"])
    # the root: sums and raw moments that ride with the conversion (ICtCp, CIELuv); k_sum3 and k_cov_nodes (sRGB) -- exact
    assert np.array_equal(_root_words(a["trace"]), _root_words(b["trace"]))
    assert _same_decisions(a["trace"], b["trace"])
    scale = float(np.max(np.abs(a["centers"])))
    assert a["centers"].shape == b["centers"].shape and float(np.max(np.abs(a["centers"] - b["centers"]))) <= 1e-9 * scale
    assert np.array_equal(b["map"], a["map"][perm])
    # and the permuted image's result is the oracle's for that image
    ec, pal_o, map_o = ob.patolette(w, h, ob.planar(colors_p), wts_p, K, dither=False, color_space=cs, kmeans_niter=0)
    assert ec == 0
    assert _is_oracles(b["pal"], b["map"], pal_o, map_o)


# ----------------------------------------------------------------------------------------------------------------------
# B. tiling-invariant sums: everything
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", B_CASES, ids=_id)
def test_invariant_sums_give_every_bit_for_any_pixel_order(gpu, native, loop, invariant_sums, case):
    import patolette_amd as p
    entry, w, h, content, K, cs, on_device, perm_kind, weights = case
    colors, wts = _inputs(w, h, content, weights)
    colors_p, wts_p, perm = _permuted(perm_kind, w, h, content, weights)
    loop(on_device)
    a = _call(p, native, entry, w, h, colors, wts, K, cs)
    b = _call(p, native, entry, w, h, colors_p, wts_p, K, cs)
    _assert_everything_bit_equal(a, b, perm)


@pytest.mark.gpu
def test_order_free_kmeans_update_gives_every_bit_for_any_pixel_order(gpu, native, loop, invariant_sums):
    """patolette_amd_set_kmeans_update(1): the centroid update is 64-bit fixed-point sums rounded once, the assignment a function
    of the sample and the centroids.  No position-based subsample: kmeans_refine (pipeline.hip) draws one only if
    n > K * (max(kmeans_max_samples, 65536) // K) (Clustering.cpp:311), and here n = 5917 is below it -- every pixel is a sample."""
    import patolette_amd as p
    w, h, K, cs, niter, max_samples = 97, 61, 16, 2, 4, 512 ** 2
    assert w * h <= K * (max(max_samples, 256 * 256) // K)
    colors, wts = _inputs(w, h, "noise", 3)
    colors_p, wts_p, perm = _permuted("shuffle", w, h, "noise", 3)
    loop(1)
    prev = p.set_kmeans_update(1)
    try:
        a = _call(p, native, "rows", w, h, colors, wts, K, cs, niter, max_samples)
        route = gpu.patolette_amd_debug_km_route()
        stats = p.last_stats()
        b = _call(p, native, "rows", w, h, colors_p, wts_p, K, cs, niter, max_samples)
    finally:
        p.set_kmeans_update(prev)
    assert route & 2048 and stats["kmeans_samples"] == w * h          # the order-free sums ran, on every pixel
    assert not np.array_equal(a["pal"], p.quantize(w, h, colors, K, dither=False, color_space=cs, tile_size=0, kmeans_niter=0, weights=wts)[1])
    _assert_everything_bit_equal(a, b, perm)


# ----------------------------------------------------------------------------------------------------------------------
# C. the grids at their a-priori edges, inside the bounds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", C_CASES, ids=_id)
def test_the_colour_spaces_extremes_either_side_of_a_power_of_two(gpu, native, ob, loop, invariant_sums, case):
    """the cube's corners and their neighbourhoods, 2^16 - 1 and 2^16 + 1 pixels (the grids' P goes from 16 to 17): every bit is the
    same for the permuted image, and the result is the oracle's"""
    import patolette_amd as p
    w, h, cs, on_device, perm_kind = case
    colors, _ = _inputs(w, h, "corners", 0)
    colors_p, _, perm = _permuted(perm_kind, w, h, "corners", 0)
    assert colors.min() == 0.0 and colors.max() == 1.0 and len(np.unique(colors, axis=0)) == w * h
    loop(on_device)
    a = _call(p, native, "planar", w, h, colors, None, C_K, cs)
    b = _call(p, native, "planar", w, h, colors_p, None, C_K, cs)
    _assert_everything_bit_equal(a, b, perm)
    ec, pal_o, map_o = ob.patolette(w, h, ob.planar(colors_p), None, C_K, dither=False, color_space=cs, kmeans_niter=0)
    assert ec == 0
    assert _is_oracles(b["pal"], b["map"], pal_o, map_o)


# ----------------------------------------------------------------------------------------------------------------------
# D. input beyond [0, 1]
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cs", [1, 2])
@pytest.mark.parametrize("content", ["far", "wide"])
def test_input_beyond_the_unit_cube_stays_on_the_grids(gpu, native, ob, content, cs):
    """sRGB channels in [7.5, 9] ("far") and in [-0.25, 1.25] ("wide"), 256 x 256: the sums that ride with the conversion are built
    for the colour space's a-priori bounds and nothing compares the measured extrema with them -- but the companding clamps to
    [0, 1] (tests/test_order_free_model.py), so the bounds hold: the root's axis and covariance have the same bits under all four
    permutations, and the palette is the oracle's.  "far" is one colour once converted: 65 536 white pixels, a root without extent."""
    import patolette_amd as p
    w, h, K = BEYOND_W, BEYOND_H, 16
    colors, _ = _inputs(w, h, content, 0)
    a = _call(p, native, "rows", w, h, colors, None, K, cs)
    for perm_kind in PERMS:
        colors_p, _, perm = _permuted(perm_kind, w, h, content, 0)
        b = _call(p, native, "rows", w, h, colors_p, None, K, cs)
        assert np.array_equal(_root_words(a["trace"]), _root_words(b["trace"])), perm_kind
    ec, pal_o, _ = ob.patolette(w, h, ob.planar(colors), None, K, dither=False, color_space=cs, kmeans_niter=0)
    assert ec == 0
    assert float(np.max(np.abs(a["pal"] - pal_o))) <= 1e-9 * float(np.max(np.abs(pal_o)))


# ----------------------------------------------------------------------------------------------------------------------
# E. measure: integer atomics
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ictcp", [True, False])
@pytest.mark.parametrize("skip_index", [None, 3])
def test_measure_counts_and_error_sums_for_any_pixel_order(gpu, ictcp, skip_index):
    """a 2-frame 37 x 53 clip mapped onto 16 colours, each frame's pixels and its map permuted alike (another shuffle per frame):
    `entries` and `per_frame` are counts, sums and maxima of integers -- not a bit changes"""
    import patolette_amd as p
    F, H, W, K = 2, 53, 37, 16
    rng = np.random.default_rng(61)
    clip = rng.integers(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    pal = rng.integers(0, 256, size=(K, 3)).astype(np.uint8)
    ok, maps, _, msg = p.remap(clip, pal, dither=False, want_quantized=False)
    assert ok, msg
    maps = np.array(maps)
    maps[rng.random(maps.shape) < 0.25] = 3                         # any map has an error: a quarter of the positions on entry 3
    clip_p, maps_p = np.empty_like(clip), np.empty_like(maps)
    for f in range(F):
        perm = rng.permutation(H * W)
        clip_p[f] = clip[f].reshape(-1, 3)[perm].reshape(H, W, 3)
        maps_p[f] = maps[f].reshape(-1)[perm].reshape(H, W)
    ok, ent, per, _, msg = p.measure(clip, maps, pal, skip_index=skip_index, ictcp=ictcp)
    assert ok, msg
    ok, ent_p, per_p, _, msg = p.measure(clip_p, maps_p, pal, skip_index=skip_index, ictcp=ictcp)
    assert ok, msg
    assert ent[:, 0].sum() == F * H * W - (int((maps == 3).sum()) if skip_index == 3 else 0) and ent[:, 1].sum() > 0
    assert np.array_equal(ent, ent_p) and np.array_equal(per, per_p)
