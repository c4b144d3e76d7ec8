"""The KMeans stage at the edges of every route, bit for bit against the independent model (tests/km_ref.py; the model itself is
held to the oracle and to the reference-faiss goldens by tests/test_km_reference.py, which also shows that the generators reach
what they are for).  Every case calls patolette_amd_kmeans_refine, asserts the route mask (patolette_amd_debug_km_route: a forced
route that silently fell back fails here) and then the centroid bits.  No tolerance, nothing skipped.  Only the subsampled cases
are compared with the oracle (the model does not subsample).

k_km_scatter_lds (chunks of 4096 samples: from 16.5 M samples) is not reached at these sizes; it stays with
test_gpu_kmeans_update.py::test_kmeans_over_every_pixel_of_a_16_mp_image."""
import ctypes as C

import numpy as np
import pytest

from tests import km_ref as kr

pytestmark = pytest.mark.gpu

dp = C.POINTER(C.c_double)
f32, f64 = np.float32, np.float64

LIST, SCAN, BIGK, G32, G64, MID, SC_INT, SC_BYTE, SC_PAIR, SC_LDS, COOP, SUMS = (1 << b for b in range(12))

ENV = {
    "list": {},
    "scan": {"PAMD_KM_LIST_LONGEST": "0"},
    "coop": {"PAMD_KM_LIST_LONGEST": "0", "PAMD_KM_LONG_MIN": "1"},
    "g32": {"PAMD_KM_LUT_MIN": "1"},
    "g32coop": {"PAMD_KM_LUT_MIN": "1", "PAMD_KM_LONG_MIN": "1"},
    "g64": {"PAMD_KM_LUT_MIN": "1", "PAMD_KM_G64_MIN": "1"},
}


def _chunk_len(nx):
    c = -(-nx // 4096)                                           # chunk_len_for: at most ~4096 chunks, whole wavefront steps
    return max(64, -(-c // 64) * 64)


def expected_mask(route, nx, k, sums=False):
    """what kmeans_iterate must have decided for this route name, sample count and k"""
    long_min = 1 if route.endswith("coop") else 8192
    if route == "list":
        assert k <= 256 and nx <= 1 << 19 and not sums
        return LIST
    if route in ("scan", "coop"):
        m = SCAN | (BIGK if k > 4096 else 0)
        mid = False
    else:
        assert 16 <= k <= 256
        g64 = route == "g64"
        mid = g64 and k % 8 == 0
        m = (G64 if g64 else G32) | (MID if mid else 0)
    if sums and k <= 4096:
        return m | SUMS
    cl = _chunk_len(nx)
    m |= SC_INT if not mid else SC_LDS if cl >= 4096 else SC_PAIR if cl >= 2 * k else SC_BYTE
    return m | (COOP if nx >= long_min else 0)


def _d(a):
    return a.ctypes.data_as(dp) if a is not None else None


def run(gpu, monkeypatch, route, pts, w, cent, niter, max_samples=None):
    for name in ("PAMD_KM_LIST_LONGEST", "PAMD_KM_LONG_MIN", "PAMD_KM_LUT_MIN", "PAMD_KM_G64_MIN"):
        monkeypatch.delenv(name, raising=False)
    for name, v in ENV[route].items():
        monkeypatch.setenv(name, v)
    n, k = pts.shape[0], cent.shape[0]
    flat = np.ascontiguousarray(pts.T).reshape(-1).copy()
    c = np.ascontiguousarray(cent.T).reshape(-1).copy()
    wv = None if w is None else np.ascontiguousarray(w, f64)
    assert gpu.patolette_amd_kmeans_refine(_d(flat), _d(wv), n, _d(c), k, int(niter), int(max_samples if max_samples else n + k)) == 0
    return c.reshape(3, k).T.astype(f32), gpu.patolette_amd_debug_km_route()


_DATA = {}


def data(key, make):
    if key not in _DATA:
        _DATA[key] = make()
    return _DATA[key]


_WANT = {}


def want(key, niter, order_free=False):
    """the model's centroids of case `key`, computed once"""
    kk = (key, niter, order_free)
    if kk not in _WANT:
        _WANT[kk] = kr.refine(*_DATA[key], niter, order_free=order_free)
    return _WANT[kk]


def check(gpu, monkeypatch, route, key, niter, sums=False):
    pts, w, cent = _DATA[key]
    if sums:
        assert gpu.patolette_amd_set_kmeans_update(1) == 0
    try:
        got, mask = run(gpu, monkeypatch, route, pts, w, cent, niter)
    finally:
        if sums:
            gpu.patolette_amd_set_kmeans_update(0)
    assert mask == expected_mask(route, pts.shape[0], cent.shape[0], sums), "route %s: mask %#x" % (route, mask)
    ref = want(key, niter, sums)
    bad = np.nonzero((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%d of %d centroids differ, first %s: %s != %s" % (bad.size, ref.shape[0], bad[:5], got[bad[:2]], ref[bad[:2]])


# ------------------------------------------------------------------------------------------------ staircase
@pytest.mark.parametrize("route", ["list", "scan", "coop", "g32", "g32coop"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("layout", ["shuffled", "runs", "striped"])
def test_staircase(gpu, monkeypatch, layout, weighted, route):
    key = ("stair", layout, weighted)
    data(key, lambda: kr.staircase(kr.STAIR_COUNTS, layout, weighted))
    check(gpu, monkeypatch, route, key, 1)


@pytest.mark.parametrize("route", ["scan", "coop"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("layout", ["shuffled", "runs", "striped"])
def test_staircase_beyond_4096_centroids(gpu, monkeypatch, layout, weighted, route):
    """k = 4097: the staircase padded with single-member centres; cluster sizes and sort cursors in memory"""
    key = ("stair4097", layout, weighted)
    data(key, lambda: kr.staircase(kr.STAIR_COUNTS, layout, weighted, k_pad=4097 - len(kr.STAIR_COUNTS)))
    check(gpu, monkeypatch, route, key, 1)


# ------------------------------------------------------------------------------------------------ binade walk
@pytest.mark.parametrize("route,niter", [("list", 1), ("list", 3), ("scan", 1), ("coop", 1), ("coop", 3)])
@pytest.mark.parametrize("weighted", [False, True])
def test_binade_walk(gpu, monkeypatch, weighted, route, niter):
    key = ("binade", weighted)
    data(key, lambda: kr.binade_walk(weighted))
    check(gpu, monkeypatch, route, key, niter)


# ------------------------------------------------------------------------------------------------ ties
def _tie_routes(k):
    r = ["list", "scan"]
    if 16 <= k <= 256:
        r += ["g32", "g64"]                                        # g64: records for k % 8 != 0, the LDS table for k % 8 == 0
    return r


@pytest.mark.parametrize("niter", [1, 2])
@pytest.mark.parametrize("k,route", [(k, r) for k in kr.TIES_K for r in _tie_routes(k)])
def test_ties(gpu, monkeypatch, k, route, niter):
    key = ("ties", k)
    data(key, lambda: kr.ties(k))
    check(gpu, monkeypatch, route, key, niter)


# ------------------------------------------------------------------------------------------------ degenerate boxes
@pytest.mark.parametrize("route,k", [("scan", 24), ("g32", 24), ("g64", 24), ("g64", 27)])
@pytest.mark.parametrize("kind", ["flat1", "flat2", "flat3", "tiny30", "tiny40", "huge", "small"])
def test_degenerate_box(gpu, monkeypatch, kind, route, k):
    key = ("box", kind, k)
    data(key, lambda: kr.degenerate_box(kind, k))
    check(gpu, monkeypatch, route, key, 2)


# ------------------------------------------------------------------------------------------------ starved
@pytest.mark.parametrize("k,ncol,route,sums", [(k, nc, r, s) for k, nc in ((2, 1), (3, 2), (40, 5), (64, 9), (65, 9), (256, 30))
                                              for r, s in (("list", False), ("scan", False), ("scan", True))]
                         + [(4100, 900, "scan", False), (4100, 900, "coop", False)])
def test_starved(gpu, monkeypatch, k, ncol, route, sums):
    key = ("starved", k, ncol)
    data(key, lambda: kr.starved(k, ncol))
    check(gpu, monkeypatch, route, key, 2, sums)


# ------------------------------------------------------------------------------------------------ sample counts
NX = [25, 63, 64, 65, 960, 1023, 1024, 1025, 1088, 4095, 4096, 4097, 4095 * 64, 262144, 262145]


@pytest.mark.parametrize("route", ["list", "scan", "coop", "g64"])
@pytest.mark.parametrize("nx", NX)
def test_sample_counts(gpu, monkeypatch, nx, route):
    """nx % 64, one chunk and an odd number of them (15, 16, 17 at 960, 1024, 1088), 4095 and 4096 chunks, chunk length 64 -> 128 at
    262 145; on the list path 262 145 is the 257th block of 1024 samples, the second batch of 256"""
    key = ("nx", nx)
    data(key, lambda: kr.counts_case(nx))
    check(gpu, monkeypatch, route, key, 1)


@pytest.mark.parametrize("nx", [1025, 4097, 262144])
def test_sample_counts_byte_scatter(gpu, monkeypatch, nx):
    """k = 64: chunks of 64 samples are shorter than 2 k, the LDS-table route scatters single records from byte assignments"""
    key = ("nx64", nx)
    data(key, lambda: kr.counts_case(nx, 64))
    check(gpu, monkeypatch, "g64", key, 1)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nx", [63, 65, 1025, 4097, 262144, 262145])
def test_sample_counts_paired_scatter_at_its_limit(gpu, monkeypatch, nx, weighted):
    """k = 32: chunks of 64 samples are exactly 2 k long, the shortest the paired byte scatter takes (SC_PAIR is asserted); at
    262 145 the chunks are 128 long"""
    key = ("nx32", nx, weighted)
    data(key, lambda: kr.counts_case(nx, 32, weighted))
    assert expected_mask("g64", nx, 32) & SC_PAIR
    check(gpu, monkeypatch, "g64", key, 1)


@pytest.mark.parametrize("route", ["list", "scan", "g32", "g64"])
@pytest.mark.parametrize("weighted", [False, True])
def test_striped_one_member_per_step(gpu, monkeypatch, weighted, route):
    """200 clusters of 40, round robin: no 64-sample step holds two members of a centroid (all step counts are 0 or 1)"""
    key = ("striped_even", weighted)
    data(key, lambda: kr.striped_even(weighted))
    check(gpu, monkeypatch, route, key, 1)


def test_the_4096th_member_ends_block_255(gpu, monkeypatch):
    """list path: a cluster whose 4096th member (the end of a listed piece) is the last record of sample block 255, its 4097th
    alone in block 256"""
    key = ("end255",)
    data(key, kr.end255)
    check(gpu, monkeypatch, "list", key, 1)


def test_n_equal_k(gpu, monkeypatch):
    pts, w, cent = kr.staircase([1] * 24, "shuffled", False)
    got, mask = run(gpu, monkeypatch, "list", pts, w, cent, 3)
    assert mask == 0
    assert np.array_equal(got.view(np.uint32), pts.astype(f32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ order-free
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k,route", [(2, "scan"), (61, "scan"), (61, "g64"), (256, "scan"), (256, "g64"), (4096, "scan")])
@pytest.mark.parametrize("rem", [0, 1, 2, 3])
def test_order_free_sums_are_the_integer_model(gpu, monkeypatch, rem, k, route, weighted):
    key = ("sums", k, rem, weighted)
    counts = [3 + (j * 7) % 5 for j in range(k)]
    counts[0] += (rem - sum(counts)) % 4
    data(key, lambda: kr.staircase(counts, "shuffled", weighted))
    assert _DATA[key][0].shape[0] % 4 == rem
    check(gpu, monkeypatch, route, key, 2, sums=True)


# ------------------------------------------------------------------------------------------------ subsampled (oracle)
@pytest.mark.parametrize("route", ["list", "scan"])
@pytest.mark.parametrize("weighted", [False, True])
def test_subsampled_against_the_oracle(gpu, ob, monkeypatch, weighted, route):
    """n = 70 000 > 24 * (65536 // 24) = 65 520: the samples are gathered through the subsample list"""
    k, nx = 24, 24 * (65536 // 24)
    pts, w, cent = kr.counts_case(70000)
    if weighted:
        w = (((np.arange(70000, dtype=np.int64) * 40503) % 4093) + 3).astype(f64) * 2.0 ** -12
    got, mask = run(gpu, monkeypatch, route, pts, w, cent, 2, max_samples=65536)
    assert mask == expected_mask(route, nx, k)
    flat = np.ascontiguousarray(pts.T).reshape(-1).copy()
    ref = ob.kmeans_refine(flat, w, 70000, np.ascontiguousarray(cent), 2, 65536).astype(f32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the two departures
@pytest.mark.parametrize("route,sums", [("list", False), ("scan", False), ("scan", True)])
def test_empty_clusters_without_a_donor_stay(gpu, monkeypatch, route, sums):
    """weights of 2^-10: no cluster size exceeds 1, no candidate of the donor walk can be accepted (the reference does not return)"""
    key = ("nodonor",)
    data(key, kr.no_donor)
    check(gpu, monkeypatch, route, key, 2, sums)


def test_subsample_of_no_samples_is_skipped(gpu, monkeypatch):
    """k = 70 000 > max_samples: the reference subsamples to k * (65536 // k) = 0 samples and n - k wraps"""
    k = 70000
    pts, w, cent = kr.staircase([1] * (k + 1), "runs", False)
    cent = cent[:k]
    got, mask = run(gpu, monkeypatch, "scan", pts, None, cent, 2, max_samples=65536)
    assert mask == 0
    assert np.array_equal(got.view(np.uint32), cent.astype(f32).view(np.uint32))


@pytest.mark.parametrize("what", ["sample", "centre", "weights"])
def test_outside_the_finite_domain_is_skipped(gpu, monkeypatch, what):
    """host side only: no kernel sees these"""
    pts, w, cent = kr.no_donor()
    pts, cent = pts.copy(), cent.copy()
    if what == "sample":
        pts[7, 1] = 1e20
    elif what == "centre":
        cent[2, 0] = 1e20
    else:
        w = np.full(pts.shape[0], 1e-44)
    assert not kr.in_domain(pts, w, cent)
    got, mask = run(gpu, monkeypatch, "list", pts, w, cent, 2)
    assert mask == 0
    assert np.array_equal(got.view(np.uint32), cent.astype(f32).view(np.uint32))


@pytest.mark.parametrize("what", ["subnormal", "negative"])
def test_full_entry_outside_the_finite_domain_skips_kmeans(gpu, monkeypatch, what):
    """the same rule on the full path (the weights' statistics pass hands the smallest positive weight and the sign to KMeans):
    one weight of 1e-44 (subnormal as f32) or one negative weight among ordinary ones -> the palette is the one without KMeans and
    the route mask is 0; with ordinary weights KMeans runs (host side only: no KMeans kernel sees the bad weights)"""
    import patolette_amd as p
    from oracle import binding as ob
    for name in ("PAMD_KM_LIST_LONGEST", "PAMD_KM_LONG_MIN", "PAMD_KM_LUT_MIN", "PAMD_KM_G64_MIN"):
        monkeypatch.delenv(name, raising=False)
    w_, h_, K = 96, 64, 16
    n = w_ * h_
    colors = ob.image(n, 5).reshape(3, n).T.copy()
    wts = ob.weights(n, 5).copy()

    def quantize(weights, niter):
        ok, pal, pmap, msg = p.quantize(w_, h_, colors, K, dither=False, color_space=0, tile_size=0, kmeans_niter=niter,
                                        kmeans_max_samples=65536, weights=weights)
        assert ok, msg
        return np.array(pal, dtype=f64), gpu.patolette_amd_debug_km_route()

    _, mask = quantize(wts, 2)
    assert mask == LIST                                           # ordinary weights: KMeans runs
    wts[n // 3] = 1e-44 if what == "subnormal" else -1e-30
    pal0, _ = quantize(wts, 0)
    pal2, mask = quantize(wts, 2)
    assert mask == 0
    # KMeans skipped: the centres (sRGB is the quantisation space here) come back rounded to f32 and otherwise untouched
    assert np.array_equal(pal2, pal0.astype(f32).astype(f64))
