"""The KMeans model of tests/km_ref.py against the C oracle, bit for bit, on the generator cases that tests/test_gpu_kmeans_edges.py
runs on the device -- all of them but two kinds: the staircase padded to 4097 centroids (the model takes 20 s; it is the staircase
below plus single-member clusters) and the order-free cases (the oracle has no such update: test_order_free_model_is_the_exact_
rational_mean stands in) -- and on the reference-faiss goldens that are not subsampled -- and the proof that the generators reach what they
are for: the block classifier reports every outcome of km_block_exact / km_block_step, the tie generator reports ties of every
multiplicity and ties made by the clamp, the staircase is order-sensitive.  No GPU.

(The cases of the donor walk that the reference does not end -- km_ref.split_clusters' rule -- are never given to the oracle.)"""
import numpy as np
import pytest

from tests import km_ref as kr
from tests.golden import make_golden as mg
from tests.util import golden

f32, f64 = np.float32, np.float64


def _oracle(ob, pts, w, cent, niter):
    n = pts.shape[0]
    flat = np.ascontiguousarray(pts.T).reshape(-1).copy()
    got = ob.kmeans_refine(flat, None if w is None else np.ascontiguousarray(w), n, np.ascontiguousarray(cent), niter, n + cent.shape[0])      # no subsampling
    return got.astype(f32)


def _same(ob, pts, w, cent, niters=(1, 3)):
    for it in niters:
        got = kr.refine(pts, w, cent, it)
        want = _oracle(ob, pts, w, cent, it)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "niter %d" % it


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("layout", ["shuffled", "runs", "striped"])
def test_staircase(ob, layout, weighted):
    _same(ob, *kr.staircase(kr.STAIR_COUNTS, layout, weighted), niters=(1, 3))


@pytest.mark.parametrize("weighted", [False, True])
def test_binade_walk(ob, weighted):
    _same(ob, *kr.binade_walk(weighted))


@pytest.mark.parametrize("k", kr.TIES_K)
def test_ties(ob, k):
    _same(ob, *kr.ties(k))


@pytest.mark.parametrize("nx,k,weighted", [(nx, 24, False) for nx in (25, 63, 64, 65, 960, 1023, 1024, 1025, 1088, 4095, 4096, 4097, 4095 * 64,
                                                                     262144, 262145)]
                         + [(nx, 64, False) for nx in (1025, 4097, 262144)]
                         + [(nx, 32, wt) for nx in (63, 65, 1025, 4097, 262144, 262145) for wt in (False, True)])
def test_sample_counts(ob, nx, k, weighted):
    _same(ob, *kr.counts_case(nx, k, weighted), niters=(1,))


def test_end255(ob):
    _same(ob, *kr.end255(), niters=(1,))


@pytest.mark.parametrize("weighted", [False, True])
def test_striped_even(ob, weighted):
    pts, w, cent = kr.striped_even(weighted)
    _same(ob, pts, w, cent, niters=(1,))
    a = kr.assign(pts.astype(f32), cent.astype(f32))
    per_step = max(int(np.bincount(a[s0:s0 + 64]).max()) for s0 in range(0, a.shape[0], 64))
    assert per_step == 1                                      # at most one member of a centroid in any 64-sample step


@pytest.mark.parametrize("k", [24, 27])
@pytest.mark.parametrize("kind", ["flat1", "flat2", "flat3", "tiny30", "tiny40", "huge", "small"])
def test_degenerate_box(ob, kind, k):
    pts, w, cent = kr.degenerate_box(kind, k)
    assert kr.in_domain(pts, w, cent)
    _same(ob, pts, w, cent, niters=(2,))


@pytest.mark.parametrize("k,ncol", [(2, 1), (3, 2), (40, 5), (64, 9), (65, 9), (256, 30), (4100, 900)])
def test_starved(ob, k, ncol):
    pts, w, cent = kr.starved(k, ncol)
    _same(ob, pts, w, cent, niters=(1, 3) if k < 1000 else (2,))
    cnt = {}
    kr.refine(pts, w, cent, 1, counters=cnt)
    print("starved k %d: %d clusters re-seeded, %d blocks of 624 draws" % (k, cnt["splits"], cnt["refills"]))
    assert cnt["splits"] >= 1
    if k >= 64:
        assert cnt["refills"] >= 3                          # the generator's block is refilled at least twice


@pytest.mark.parametrize("ci", [0, 1, 4])
def test_goldens_without_subsampling(ci):
    """the reference's own faiss (kmeans_ref.npz)"""
    g = golden("kmeans_ref.npz")
    n, k, niter, max_samples, weighted, seed, plant = (int(v) for v in g["cases"][ci])
    assert n <= k * (max(max_samples, 65536) // k)
    x, w, cent = mg.km_inputs(n, k, bool(weighted), seed, bool(plant))
    got = kr.refine(x.reshape(3, n).T, w, cent, niter)
    assert np.array_equal(got.view(np.uint32), g["cent_%d" % ci].astype(f32).view(np.uint32))


def _classify(pts, w, cent, j, margins=None):
    x, c = pts.astype(f32), cent.astype(f32)
    wf = None if w is None else w.astype(f32)
    a = kr.assign(x, c)
    _, _, tr = kr.update(x, wf, a, c.shape[0], trace_of=j)
    m = np.nonzero(a == j)[0]
    tot = dict.fromkeys(kr.OUTCOMES, 0)
    for comp in range(4 if wf is not None else 3):
        add = wf[m].astype(f64) if comp == 3 else x[m, comp].astype(f64) * (wf[m].astype(f64) if wf is not None else 1.0)
        for key, v in kr.classify_blocks(add, tr[:, comp], margins).items():
            tot[key] += v
    return tot


@pytest.mark.parametrize("weighted", [False, True])
def test_binade_walk_meets_every_outcome_of_the_block_form(weighted):
    margins = []
    tot = _classify(*kr.binade_walk(weighted), 0, margins)
    print("binade_walk weighted=%d: %s" % (weighted, tot))
    for key in kr.OUTCOMES:
        assert tot[key] >= 1, key
    # tie-free blocks and quarters that end one unit inside, on and one unit beyond each bound of km_block_exact
    up = sorted({int(a) for a, _ in margins if abs(a) <= 1})
    lo = sorted({int(b) for _, b in margins if abs(b) <= 1})
    print("units left below the upper bound: %s, above the lower bound: %s (of %d evaluations)" % (up, lo, len(margins)))
    assert up == [-1, 0, 1] and lo == [-1, 0, 1]


def test_staircase_long_counts_pass_whole_and_by_quarters():
    pts, w, cent = kr.staircase(kr.STAIR_COUNTS, "runs", False)
    tot = _classify(pts, w, cent, kr.STAIR_COUNTS.index(12289))
    print("staircase, 12289 members: %s" % tot)
    assert tot["whole"] >= 1 and tot["quarters"] >= 1


@pytest.mark.parametrize("weighted", [False, True])
def test_staircase_chains_are_order_sensitive(weighted):
    """the members of a cluster taken in another order change a bit of its centroid, for every cluster of 31 members and more: with
    the order reversed, and with just two members exchanged (one of a dozen fixed pairs per cluster: an exchange moves the sum by an
    ulp or two, which the product with 1 / h can round away, so each cluster is asked for one pair that moves its centroid)"""
    pts, w, cent = kr.staircase(kr.STAIR_COUNTS, "runs", weighted)
    base = kr.refine(pts, w, cent, 1)
    start = np.concatenate([[0], np.cumsum(kr.STAIR_COUNTS)])
    big = [j for j, c in enumerate(kr.STAIR_COUNTS) if c >= 31]

    def changed_by(pairs):
        perm = np.arange(pts.shape[0])
        for j in big:
            c = kr.STAIR_COUNTS[j]
            if pairs is None:
                perm[start[j]:start[j + 1]] = perm[start[j]:start[j + 1]][::-1]
            else:
                a, b = start[j] + pairs[0] % c, start[j] + pairs[1] % c
                perm[[a, b]] = perm[[b, a]]
        other = kr.refine(pts[perm], None if w is None else w[perm], cent, 1)
        return (base.view(np.uint32) != other.view(np.uint32)).any(axis=1)[big]
    rev = changed_by(None)
    print("reversed: clusters whose centroid bits change: %d of %d" % (int(rev.sum()), len(big)))
    assert rev.all()
    any_pair = np.zeros(len(big), bool)
    for pair in ((3, -2), (0, -1), (1, 17), (5, 29), (2, 30), (7, 11), (0, 15), (4, -3), (6, 23), (8, 27), (9, 19), (10, -5)):
        if any_pair.all():
            break
        ch = changed_by(pair)
        print("members %s exchanged: clusters whose centroid bits change: %d of %d" % (pair, int(ch.sum()), len(big)))
        any_pair |= ch
    assert any_pair.all()


@pytest.mark.parametrize("k", kr.TIES_K)
def test_ties_reach_every_multiplicity_and_the_clamp(k):
    pts, _, cent = kr.ties(k)
    _, nwin, nneg = kr.assign(pts.astype(f32), cent.astype(f32), stats=True)
    two, three, more, clamp = (int(v) for v in ((nwin == 2).sum(), (nwin == 3).sum(), (nwin > 3).sum(), (nneg >= 2).sum()))
    print("ties k %d, %d samples: equidistant winners 2: %d, 3: %d, more: %d; two centres negative before the clamp: %d"
          % (k, pts.shape[0], two, three, more, clamp))
    assert two >= 1 and clamp >= 1
    if k >= 7:                                                # (two centres cannot tie three ways)
        assert three >= 1 and more >= 1


def test_order_free_model_is_the_exact_rational_mean():
    pts, w, cent = kr.staircase([5, 9, 0, 33, 2], "shuffled", True)
    n, k = pts.shape[0], cent.shape[0]
    x, wf, c = pts.astype(f32), w.astype(f32), cent.astype(f32)
    qx, qw = kr.km_fix(float(np.abs(pts).max()), max(1.0, float(np.abs(w).max())), True, n)
    a = kr.assign(x, c)
    got, h = kr.update_sums(x, wf, a, k, qx, qw)
    for j in range(k):
        want, hw = kr.exact_sums_mean(x, wf, np.nonzero(a == j)[0], qx, qw)
        assert h[j].view(np.uint32) == hw.view(np.uint32)
        assert np.array_equal(got[j].view(np.uint32), want.view(np.uint32)), j
    got_u, h_u = kr.update_sums(x, None, a, k, *kr.km_fix(float(np.abs(pts).max()), 1.0, False, n))
    for j in range(k):
        want, hw = kr.exact_sums_mean(x, None, np.nonzero(a == j)[0], *kr.km_fix(float(np.abs(pts).max()), 1.0, False, n))
        assert h_u[j] == hw and np.array_equal(got_u[j].view(np.uint32), want.view(np.uint32)), j


def test_no_donor_rule_and_domain():
    """the two departures as the header states them: weights of 2^-10 leave no size above 1 -> empty clusters stay (0, 0) and the
    iterations go on; 1e20 values and subnormal weights are outside the finite domain"""
    pts, w, cent = kr.no_donor()
    got = kr.refine(pts, w, cent, 2)
    assert np.isfinite(got).all() and int((got == 0).all(axis=1).sum()) == 5
    assert kr.in_domain(pts, w, cent)
    p2 = pts.copy()
    p2[7, 1] = 1e20
    assert not kr.in_domain(p2, w, cent)
    c2 = cent.copy()
    c2[2, 0] = 1e20
    assert not kr.in_domain(pts, w, c2)
    assert not kr.in_domain(pts, np.full(pts.shape[0], 1e-44), cent)
