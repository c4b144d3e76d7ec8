"""The global quantiser (global.c:189-377) at its edges, on BOTH routes of the engine: the host's turn (k_gq_prefix / k_gq_init /
k_gq_dp, then hm::gq_principal_quantizer and the records of gq_host_decide) and the control kernel (k_gq_control), each driven from
a moment table through patolette_amd_debug_gq_table -- the production code on scratch buffers -- and held to the model of
tests/gq_ref.py BIT FOR BIT, with no tolerance: both routes and the model evaluate the same f64 expressions in the same order (the
build has -ffp-contract=off, the eigen-solver is pinned bit for bit elsewhere).  Compared: the inclusive prefix tables, the count of
base clusters, the error flag, the cuts, the dynamic programme's cut table, the bucket -> cluster table and the base clusters' records.

The tables (tests/gq_ref.tables, their properties asserted on the CPU by tests/test_gq_reference.py) aim at exact ties of the
dynamic programme inside one lane and across lanes, empty buckets and empty base clusters, the carry-over rule E_k[n] = E_{k-1}[n]
for n <= k, the in-register prefix chains, and every branch of the termination test a finite table can reach.  Palette sizes 2, 3, 12,
13 and 256 on both routes, though quantize() takes the control kernel above 12 only.

Then whole images of grey bands, which go to twelve base clusters with most of them EMPTY (zero-pixel children in the partition,
the children's covariance sweep and the split loop's frontier; NaN centres in the nearest map), through quantize() on every route."""
import numpy as np
import pytest

from tests import gq_ref as gr
from tests.test_gpu_split_loop import _same_decisions
from tests.test_gpu_sweep_edges import _is_oracles
from tests.test_gq_reference import IMAGE_CASES, NAMES, TABLES, model
from tests.util import bits

pytestmark = pytest.mark.gpu

PALETTE_SIZES = (2, 3, 12, 13, 256)


def _check(name, K, route, r, m, d):
    at = (name, K, "device route" if route else "host route")
    # the prefix tables: the chains the termination test reads (on the host route also the DP kernels' own)
    assert np.array_equal(r["prefix_w0"][0], m["prefix_w0"]), at
    assert np.array_equal(bits(r["prefix"][:10]), bits(m["prefix"])), (at, np.argwhere(bits(r["prefix"][:10]) != bits(m["prefix"]))[:4])
    if route == 0:
        assert np.array_equal(r["prefix_w0"][1], m["prefix_w0"]), at
        assert np.array_equal(bits(r["prefix"][10:14]), bits(m["prefix"][:4])), at
    assert (r["error"], r["kbase"], r["cuts"]) == (m["error"], m["kbase"], m["cuts"]), (at, r["cuts"], m["cuts"])
    # the cut table: every step up to min(K, 12) on the host route, the full steps 2 .. kbase - 1 on the device route; everything
    # else as the reference starts it (zero, L[r][r] = r)
    want = m["cut_full"] if route == 0 else m["cut_dev"]
    assert np.array_equal(r["cut_table"], want), (at, np.argwhere(r["cut_table"] != want)[:6])
    assert np.array_equal(r["bucket_table"], m["bucket_table"]), at
    assert np.array_equal(r["begin"], m["begin"]) and np.array_equal(r["n"], m["n"]), at
    # sw: the members' count, or quantity 13 -- the weights of every weighted table here are multiples of 1/4, their sum is exact
    assert np.array_equal(bits(r["sw"]), bits(m["sw"])), (at, r["sw"], m["sw"])
    if d["dyadic"]:
        # The means only where the table's entries are small dyadic numbers, so that ANY summation order gives the same sum: the
        # device adds eight buckets per lane and then shuffles across lanes, the host adds bucket after bucket.  An empty cluster's
        # mean is 0 * inf on both: a NaN, whose sign bit is the processor's choice and is not compared.
        nan = np.isnan(m["mean"])
        assert np.array_equal(np.isnan(r["mean"]), nan), at
        assert np.array_equal(bits(r["mean"])[~nan], bits(m["mean"])[~nan]), (at, r["mean"], m["mean"])


@pytest.mark.parametrize("name", NAMES)
def test_table_through_both_routes_is_the_models(gpu, native, name):
    d = TABLES[name]
    for K in PALETTE_SIZES:
        m = model(name, K)
        for route in (0, 1):
            r = native.debug_gq_table(d["table"], d["counts"], d["weighted"], K, route)
            _check(name, K, route, r, m, d)


def test_without_the_optional_outputs_the_decisions_are_the_same(gpu, native):
    """production passes a null pointer where the test entry asks for the prefixes: the decisions do not depend on it"""
    for name in ("six_colours", "bands3_along_weighted"):
        d = TABLES[name]
        for route in (0, 1):
            a = native.debug_gq_table(d["table"], d["counts"], d["weighted"], 16, route, details=True)
            b = native.debug_gq_table(d["table"], d["counts"], d["weighted"], 16, route, details=False)
            assert (a["kbase"], a["error"], a["cuts"]) == (b["kbase"], b["error"], b["cuts"])
            assert np.array_equal(a["bucket_table"], b["bucket_table"]) and np.array_equal(a["n"], b["n"])
            assert np.array_equal(bits(a["sw"]), bits(b["sw"]))


@pytest.fixture
def routes(gpu):
    first = {}

    def set_routes(gq_on_device, loop_on_device):
        a = gpu.patolette_amd_set_global_quantiser(gq_on_device)
        b = gpu.patolette_amd_set_split_loop(loop_on_device)
        first.setdefault("gq", a)
        first.setdefault("loop", b)
    yield set_routes
    if first:
        gpu.patolette_amd_set_global_quantiser(first["gq"])
        gpu.patolette_amd_set_split_loop(first["loop"])


@pytest.mark.parametrize("levels,seed,cs,weighted,K", IMAGE_CASES)
def test_grey_bands_reach_twelve_base_clusters_most_of_them_empty(gpu, native, ob, routes, levels, seed, cs, weighted, K):
    """K = 12: the host's turn whatever the switch says, and kbase == K (no split at all); 13 and 16: the control kernel when the
    switch is on.  Every route: the same decisions and centres (NaN rows where a base cluster is empty), palette and map equal bit
    for bit, and both the oracle's (tests/test_gq_reference.py shows the oracle tie-free on every one of these images)."""
    import patolette_amd as p
    w, h, colors, wts = gr.band_image(levels, seed, weighted)
    results = []
    for gq_on_device in (0, 1):
        for loop_on_device in (0, 1):
            routes(gq_on_device, loop_on_device)
            ok, pal, pmap, msg = p.quantize(w, h, colors, K, dither=False, color_space=cs, tile_size=0, kmeans_niter=0, weights=wts)
            assert ok, msg
            results.append((pal, pmap, native.last_split_trace(), native.last_cluster_centers(), p.last_stats()))
    pal0, map0, tr0, cen0, st0 = results[0]
    assert st0["n_base_clusters"] == 12 and tr0["n_base"] == 12
    empty = np.all(np.isnan(cen0), axis=1)
    assert int(np.sum(empty[:12])) >= 1 and not np.any(np.isnan(cen0[~empty]))
    for pal, pmap, tr, cen, st in results[1:]:
        assert st["n_base_clusters"] == 12 and _same_decisions(tr0, tr)
        assert np.array_equal(np.isnan(cen), np.isnan(cen0)) and np.array_equal(np.nan_to_num(cen), np.nan_to_num(cen0))
        assert np.array_equal(bits(pal), bits(pal0)) and np.array_equal(pmap, map0)
    ec, pal_o, map_o = ob.patolette(w, h, ob.planar(colors), wts, K, dither=False, color_space=cs, kmeans_niter=0)
    assert ec == 0
    assert list(tr0["gq_cuts"]) == list(ob.last_split_trace()["gq_cuts"])
    assert _is_oracles(pal0, map0, pal_o, map_o)
