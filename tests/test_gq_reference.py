"""The global quantiser's model (tests/gq_ref.py) and the tables of tests/test_gpu_gq_edges.py, checked on the CPU:

a. on tables made from pixels the model's cuts are independent_ref.principal_quantizer's on those pixels;
b. on the tables called exact, every f64 distortion(a, b) and every candidate E_{k-1}[t] + distortion(t, n) the search forms is the
   EXACT value (rational arithmetic), so equal candidates are real ties and the cuts follow from the tie rule alone;
c. every table shows what it was chosen for: where the search stops and on which branch of the termination test, empty cells, a
   tied plateau wider than a wavefront's 64 lanes -- and over all tables every count of base clusters from 1 to 12 is reached;
d. the oracle alone is tie-free on the grey-band images the GPU test compares with it, and goes to twelve base clusters there, some empty.

Needs no GPU."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from tests import gq_ref as gr
from tests import independent_ref as ir
from tests import tie_prover as tp
from tests.test_tie_prover import run

TABLES = gr.tables()
NAMES = list(TABLES)
EXACT = [n for n in NAMES if TABLES[n]["exact"]]


@functools.lru_cache(maxsize=None)
def _model(name, kmax):
    from oracle import binding
    d = TABLES[name]
    return gr.run(d["table"], d["counts"], d["weighted"], kmax, binding.eigen_sym3)


def model(name, K=256):
    return _model(name, min(K, gr.MAX_K))


def _pixels(kind, rng):
    n = 3000
    if kind == "noise":
        return rng.random((n, 3))
    if kind == "blobs":
        d = np.array([0.5, 0.6, 0.62])
        cen = 0.1 + np.sort(rng.random(6))[:, None] * d[None, :]
        return cen[rng.integers(0, 6, n)] + 0.004 * rng.standard_normal((n, 3))
    return gr.band_image(4, 9, False, 60, 50)[2]


@pytest.mark.parametrize("kind", ["noise", "blobs", "bands"])
def test_model_on_a_table_is_the_pixel_level_reading(ob, kind):
    """(a) the same pixels as independent_ref.Cells takes them and as a table: the same prefixes bit for bit, the same cuts -- with
    LAPACK's solver on both sides, and with the oracle's (the one the GPU tests inject) on the model's."""
    c = np.ascontiguousarray(_pixels(kind, np.random.default_rng(3)))
    bmap = ir.axis_sort(c, ir.pca_axis(c, None))
    cells = ir.Cells(c, bmap)
    table, counts = gr.table_from_pixels(c, bmap)
    tc = gr.TableCells(table, counts)
    assert np.array_equal(tc.w0, cells.w0) and np.array_equal(tc.w1, cells.w1) and np.array_equal(tc.w2, cells.w2)
    assert all(np.array_equal(tc.wrs[rs], cells.wrs[rs]) for rs in gr.RS)
    seen = set()
    for K in (2, 3, 5, 12, 16):
        want = ir.principal_quantizer(K, cells)
        assert gr.run(table, counts, False, K)["cuts"] == want
        assert gr.run(table, counts, False, K, ob.eigen_sym3)["cuts"] == want
        seen.add(len(want) - 1)
    assert kind == "noise" or max(seen) >= 4, seen


def test_prefix_stress_tells_a_sequential_chain_from_any_other_order():
    """blocked (eight per lane, then across lanes) and pairwise sums of the stress table differ from table[i] += table[i-1] in the
    last bits of most rows: a scheme that is not the sequential chain cannot pass the bit-for-bit comparison"""
    d = TABLES["prefix_stress"]
    t = d["table"][:, 0, :] + d["table"][:, 1, :]
    seq = gr.TableCells(d["table"], d["counts"]).prefix()[:, 1:]
    blocks = t.reshape(10, 64, 8)
    inner = np.cumsum(blocks, axis=2)
    before = np.concatenate((np.zeros((10, 1)), np.cumsum(inner[:, :, 7], axis=1)[:, :-1]), axis=1)
    blocked = (before[:, :, None] + inner).reshape(10, 512)
    pair_total = np.array([np.add.reduce(t[q]) for q in range(10)])
    assert sum(1 for q in range(10) if not np.array_equal(blocked[q], seq[q])) >= 8
    assert sum(1 for q in range(10) if pair_total[q] != seq[q, -1]) >= 5
    assert np.any(t[:3] < 0) and np.any(t[:3] > 0)


def _exact_prefixes(d):
    """the table's prefixes as integers over a common power-of-two denominator (Fraction(float) is exact)"""
    t = d["table"]
    fr = [[Fraction(float(t[q, 0, b])) + Fraction(float(t[q, 1, b])) for b in range(gr.N)] for q in range(4)]
    den = max(f.denominator for row in fr for f in row)
    assert den & (den - 1) == 0
    rows = []
    for row in fr:
        acc, out = 0, [0]
        for f in row:
            acc += int(f * den)
            out.append(acc)
        rows.append(np.array(out, dtype=object))
    w0 = np.array([int(v) for v in np.cumsum(np.concatenate(([0], d["counts"].astype(np.uint64))))], dtype=object)
    return den, rows, w0


def _two_sum_exact(a, b):
    """a + b rounds to itself: Knuth's TwoSum leaves no error term"""
    s = a + b
    bb = s - a
    return ((a - (s - bb)) + (b - bb)) == 0


@pytest.mark.parametrize("name", EXACT)
def test_exact_tables_are_exact(name):
    """(b) with D = the common denominator: distortion(a, b) = (dW2 * cnt * D - |dW1|^2) / (cnt * D^2) over the integers; the model's
    f64 value, as a Fraction, must equal it for every a < b, and every candidate sum of every step must be free of rounding.  The
    minimum the f64 search takes is then the exact minimum, and its equal candidates are exactly equal."""
    d = TABLES[name]
    den, (s0, s1, s2, sq), w0 = _exact_prefixes(d)
    m = model(name)
    cells = m["cells"]
    dmat = {}
    for b in range(1, gr.N + 1):
        a = np.arange(0, b)
        got = cells.distortion_to(a, b)
        cnt = w0[b] - w0[a]
        q2 = (s0[b] - s0[a]) ** 2 + (s1[b] - s1[a]) ** 2 + (s2[b] - s2[a]) ** 2
        num = (sq[b] - sq[a]) * cnt * den - q2                      # distortion x cnt x den^2
        # got x cnt x den^2 as an integer: got is dyadic, 2^80 clears its fraction (asserted)
        scaled = np.array([int(Fraction(float(g)) * (1 << 80)) if Fraction(float(g)).denominator <= (1 << 80) else None for g in got], dtype=object)
        assert all(v is not None for v in scaled), name
        ok = (scaled * cnt * den * den == num * (1 << 80)) | ((cnt == 0) & (got == 0))
        assert bool(np.all(ok)), (name, b, int(np.flatnonzero(~ok.astype(bool))[0]))
        dmat[b] = got
    assert Fraction(float(dmat[gr.N][0])) == Fraction(int((sq[gr.N] * w0[gr.N] * den - (s0[gr.N] ** 2 + s1[gr.N] ** 2 + s2[gr.N] ** 2))),
                                                      int(w0[gr.N]) * den * den)
    for k in range(2, max(m["E"]) + 1):
        Ep = m["E"][k - 1]
        for n in range(k + 1, gr.N + 1):
            ts = np.arange(k - 1, n - 1)
            assert bool(np.all(_two_sum_exact(Ep[ts], dmat[n][ts]))), (name, k, n)


def test_every_table_shows_what_it_was_chosen_for():
    """(c)"""
    for name, d in TABLES.items():
        p = d["props"]
        K = p.get("K", 256)
        m = model(name, K)
        assert m["error"] == 0, name
        last_k, last_branch, _, _ = m["steps"][-1]
        if "kbase" in p:
            assert m["kbase"] == p["kbase"], (name, m["kbase"])
        if "kbase_at_least" in p:
            assert m["kbase"] >= p["kbase_at_least"], (name, m["kbase"])
        if "branch" in p:
            assert last_branch == p["branch"], (name, m["steps"])
        if "cuts" in p:
            assert m["cuts"] == p["cuts"], (name, m["cuts"])
        if "cuts_head" in p:
            assert m["cuts"][:len(p["cuts_head"])] == p["cuts_head"], (name, m["cuts"])
        if "K4_cuts" in p:
            assert model(name, 4)["cuts"] == p["K4_cuts"], name
        if "empty_cell" in p:
            assert bool(np.any(m["n"] == 0)) == p["empty_cell"], (name, m["n"])
        if "skipped" in p:
            assert m["steps"][-1][2]["skipped"], name
        if "total" in p:                                             # the one cell's distortion, either side of 1e-16
            lo, hi = p["total"]
            assert lo < m["E"][1][gr.N] < hi, (name, m["E"][1][gr.N])
        if "all_tie_cut" in p:                                       # every candidate of (2, 512) ties; t = n - 1 comes first
            assert gr.minima(m["cells"], m["E"][1], 2, gr.N) == list(range(1, gr.N))
            assert m["cut_full"][2, gr.N] == p["all_tie_cut"]
        if "plateau" in p:
            lo, hi = p["plateau"]
            tied = gr.minima(m["cells"], m["E"][1], 2, gr.N)
            assert tied == list(range(lo, hi + 1)) and len(tied) > 3 * 64, (name, tied[:3], tied[-3:])
            assert (gr.N - 1 in tied) == (hi == gr.N - 1)
            assert m["cut_full"][2, gr.N] == hi
        if "symmetric" in p:                                         # three cells of 171 + 171 + 170 buckets, in any order: tied
            assert len(gr.minima(m["cells"], m["E"][2], 3, gr.N)) >= 2
        if "single_pixel" in p:                                      # the cell of one pixel is tested: zero covariance
            assert any(any(int(m["prefix_w0"][q[j + 1]] - m["prefix_w0"][q[j]]) == 1 for j in range(len(q) - 1)) for _, _, _, q in m["steps"])
        if d["dyadic"]:                                              # the rows the records add up: multiples of 2^-12, and even the
            rows = d["table"][[0, 1, 2] + ([10, 11, 12, 13] if d["weighted"] else [])]   # sum of all magnitudes stays below 2^53 of them
            assert np.all(rows == np.round(rows * 4096) / 4096) and float(np.sum(np.abs(rows))) * 4096 < 2.0 ** 53, name
    assert TABLES["threshold_below"]["props"]["total"][1] == ir.DELTA == TABLES["threshold_above"]["props"]["total"][0]
    # `norms < 1e-16` (cells.c:309) cannot fire on a finite table: both factors are norms of eigenvectors the solver returns with
    # unit length (a zero covariance gives the unit vector e3).  No table shows it; the model confirms that none does
    assert not any(s[2]["norms"] for n in NAMES for s in model(n, TABLES[n]["props"].get("K", 256))["steps"])


def test_every_count_of_base_clusters_is_reached():
    """over all tables the search stops at every kbase from 1 to 12: on the device route every full step kk = 2 .. 11 runs, each over
    n = kk + 1 .. 512 -- entries with zero candidates besides t = n - 1, with one, and with 63, 64 and 65"""
    reached = {model(n, TABLES[n]["props"].get("K", 256))["kbase"] for n in NAMES}
    assert reached >= set(range(1, 13)), reached
    branches = {model(n)["steps"][-1][1] for n in NAMES}
    assert branches >= {"distortion", "bias", None}, branches
    assert any(s[2]["skipped"] for n in NAMES for s in model(n)["steps"])


IMAGE_CASES = [(lv, seed, cs, weighted, K) for lv, seed in gr.BAND_IMAGES for cs in (0, 1, 2) for weighted in (False, True) for K in (12, 13, 16)]


@pytest.mark.parametrize("levels,seed,cs,weighted,K", IMAGE_CASES)
def test_the_oracle_alone_is_tie_free_on_the_band_images(ob, levels, seed, cs, weighted, K):
    """(d) both summation orders of the oracle take the same decisions and find the same centres (NaN pattern included), so the GPU
    test may demand the oracle's palette and map; and the images do what they are for: twelve base clusters, some of them empty."""
    w, h, colors, wts = gr.band_image(levels, seed, weighted)
    data = tp.converted(ob, ob.planar(colors), cs)
    ra, ta = run(ob, data, wts, w * h, K)
    rb, tb = run(ob, data, wts, w * h, K, reversed_sums=1)
    assert tp.first_divergence(ta, tb) is None
    assert np.array_equal(np.isnan(ra["centers"]), np.isnan(rb["centers"]))
    ca, cb = np.nan_to_num(ra["centers"]), np.nan_to_num(rb["centers"])
    assert float(np.max(np.abs(ca - cb))) <= 1e-10 * float(np.max(np.abs(ca)))
    assert ta["n_base"] == 12 and ra["n_base"] == 12
    cuts = ta["gq_cuts"]
    assert len(cuts) == 13
    assert int(np.sum(np.all(np.isnan(ra["centers"][:ra["n_clusters"]]), axis=1))) >= 1
