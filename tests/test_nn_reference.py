"""tests/nn_ref.py without a GPU: the numpy reference against the CPU oracle and against integer arithmetic, the properties every
generator promises (the GPU tests in test_gpu_nn_edges.py are only as sharp as these inputs), and a numpy model of the f32 first pass
of k_nn_map_mid against its documented error bound E = M / 2.5."""
import numpy as np
import pytest

from tests import nn_ref


def _oracle(ob, px, pal):
    return ob.nn_map(ob.planar(px), px.shape[0], np.ascontiguousarray(pal)).astype(np.int64)


def _inputs():
    """name -> (pixels, palette) of every generator"""
    out = {"lattice": nn_ref.lattice()}
    for s in (30, 40, 50, 52):
        out["shifted-%d" % s] = nn_ref.lattice_shifted(s)
    for box in nn_ref.BOXES:
        out["sweep-" + box] = nn_ref.margin_sweep(64, box)[:2]
    lo, hi = nn_ref.random_box()
    for G in (32, 64):
        for k in (8, 256, 300):
            out["edges-%d-%d" % (G, k)] = (nn_ref.cell_edges(G, lo, hi), nn_ref.box_palette(k, lo, hi))
    out["bisectors"] = nn_ref.edge_bisectors(lo, hi)[:2]
    for d in nn_ref.CROWDED:
        out["crowded-" + d] = nn_ref.crowded(d)[:2]
    return out


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


def test_brute_is_the_oracle_on_every_input(ob, inputs):
    for name, (px, pal) in inputs.items():
        idx, gap, ties = nn_ref.brute(px, pal)
        assert np.array_equal(idx, _oracle(ob, px, pal)), name
        assert np.all(ties >= 1) and np.all(gap >= 0) and np.array_equal(ties > 1, gap == 0), name


def test_brute_on_non_finite_pixels(ob):
    rng = np.random.default_rng(3)
    px, pal = rng.random((50, 3)), rng.random((16, 3))
    clean = nn_ref.brute(px, pal)[0]
    for plane, value in ((0, np.inf), (1, np.nan), (2, -np.inf), (0, 1e39)):
        p = px.copy()
        p[7, plane] = value
        idx = nn_ref.brute(p, pal)[0]
        assert np.array_equal(idx, _oracle(ob, p, pal))
        assert np.array_equal(np.delete(idx, 7), np.delete(clean, 7))
        if not np.isfinite(value):
            assert idx[7] == 0


def test_lattice_ties_in_integer_arithmetic(inputs):
    px, pal = inputs["lattice"]
    assert px.shape == (33 ** 3, 3) and pal.shape == (125, 3)
    idx, gap, ties = nn_ref.brute(px, pal)
    assert np.array_equal(idx, nn_ref.brute_int(px, pal))          # dyadic coordinates: the f64 expression is exact
    counts = {t: int(np.sum(ties == t)) for t in (2, 4, 8)}
    print("lattice: ties", counts)
    assert counts == {2: 10092, 4: 1392, 8: 64}
    assert np.sum(ties > 1) >= 0.3 * px.shape[0]
    srt = np.sort(pal.view([("", pal.dtype)] * 3).ravel())        # shuffled: not the geometric order
    assert not np.array_equal(srt, pal.view([("", pal.dtype)] * 3).ravel())
    t8 = nn_ref.tie8_points()
    assert np.all(nn_ref.brute(t8, pal)[2] == 8)


@pytest.mark.parametrize("s", [30, 40, 50, 52])
def test_lattice_shifted_moves_winners(inputs, s):
    base = nn_ref.brute(*inputs["lattice"])[0]
    px, pal = inputs["shifted-%d" % s]
    idx, gap, ties = nn_ref.brute(px, pal)
    moved = int(np.sum(idx != base))
    print("shifted 2^-%d: %d winners change, %d ties stay, smallest gap above 0: %.3g" % (s, moved, int(np.sum(ties > 1)), gap[gap > 0].min()))
    assert moved >= 1500                                           # (about 2 150: half of the ties across x fall to the other side)
    assert np.all(np.abs(px - inputs["lattice"][0]) <= 2.0 ** -s) and px.min() >= 0.0 and px.max() <= 1.0


@pytest.mark.parametrize("box", list(nn_ref.BOXES))
def test_margin_sweep_straddles_M(box):
    px, pal, lo, hi, M = nn_ref.margin_sweep(64, box)
    assert np.array_equal(px.min(axis=0), lo) and np.array_equal(px.max(axis=0), hi)       # the device's min / max finds this box
    assert M == nn_ref.margin_M(pal, px.min(axis=0), px.max(axis=0))
    assert len({tuple(r) for r in pal}) == 64
    gap = nn_ref.brute(px, pal)[1][:-8]
    below, around, above = (float(np.mean(gap < M / 2)), float(np.mean((gap >= M / 2) & (gap < 2 * M))), float(np.mean(gap >= 2 * M)))
    print("sweep %s: M %.3g; gap < M/2 %.1f %%, [M/2, 2M) %.1f %%, >= 2M %.1f %%" % (box, M, 100 * below, 100 * around, 100 * above))
    assert below >= 0.05 and around >= 0.10 and above >= 0.50


@pytest.mark.parametrize("box", list(nn_ref.BOXES))
def test_f32_first_pass_model_stays_within_E(box):
    """The kernel trusts the f32 winner when the runner-up lies more than M = 2.5 E above it.  Here: every t_j within E of the exact
    value, and no pixel both clear and wrong."""
    px, pal, lo, hi, M = nn_ref.margin_sweep(64, box)
    t, exact = nn_ref.f32_pass(px, pal, lo, hi)
    err = float(np.max(np.abs(t.astype(np.float64) - exact)))
    Mf = np.float32(M)
    if float(Mf) < M:
        Mf = np.nextafter(Mf, np.float32(np.inf))
    two = np.partition(t, 1, axis=1)[:, :2]
    clear = (two[:, 1] - two[:, 0]) > Mf
    idx = nn_ref.brute(px, pal)[0]
    wrong = np.argmin(t, axis=1) != idx
    print("f32 pass %s: max error %.3g M (E = 0.4 M); %d of %d pixels clear, %d of them wrong" %
          (box, err / M, int(clear.sum()), px.shape[0], int(np.sum(clear & wrong))))
    assert err <= M / 2.5
    assert not np.any(clear & wrong)
    naive = wrong & (two[:, 1] > two[:, 0])                        # what a margin of 0 would get wrong: the input bites
    print("f32 pass %s: a margin of 0 would misplace %d pixels" % (box, int(naive.sum())))
    assert naive.sum() >= 20
    assert 0.5 < np.mean(clear) < 0.97                             # the sweep has pixels on either side of the margin


@pytest.mark.parametrize("G", [32, 64])
def test_cell_edges_lie_on_the_devices_boundaries(G):
    lo, hi = nn_ref.random_box()
    px = nn_ref.cell_edges(G, lo, hi)
    assert np.array_equal(px.min(axis=0), lo) and np.array_equal(px.max(axis=0), hi)
    r = hi - lo
    assert not np.any(r == np.round(r * 1024) / 1024)              # non-dyadic
    for a in range(3):
        cw, inv = r[a] / G, G / r[a]                               # nn_grid
        own = px[a * 13 * (G + 1):(a + 1) * 13 * (G + 1), a]
        cells = np.clip(((own - lo[a]) * inv).astype(np.int64), 0, G - 1)               # nn_cell
        exact = own[:G + 1]
        assert np.array_equal(exact, np.clip(lo[a] + np.arange(G + 1) * cw, lo[a], hi[a]))
        assert len(np.unique(cells)) == G
        # a boundary pixel and its two neighbours do not all fall into one cell, for most boundaries
        split = sum(len({int(cells[i]), int(cells[G + 1 + i]), int(cells[2 * (G + 1) + i])}) > 1 for i in range(1, G))
        assert split >= G // 2


def test_edge_bisectors_put_the_winner_across_the_boundary():
    lo, hi = nn_ref.random_box()
    px, pal, win = nn_ref.edge_bisectors(lo, hi)
    assert np.array_equal(px.min(axis=0), lo) and np.array_equal(px.max(axis=0), hi)
    idx, gap, ties = nn_ref.brute(px, pal)
    m = win.shape[0]
    assert m == 72 and pal.shape[0] == 48
    assert np.array_equal(idx[:m], win) and np.all(ties[:m] == 1)
    r = hi - lo
    M = nn_ref.margin_M(pal, lo, hi)
    d = np.sort(np.sum((px[:m, None, :] - pal[None, :, :]) ** 2, axis=2), axis=1)
    assert np.all(gap[:m] < M)                                     # winner and runner-up within the margin: only the exact loop tells them apart
    assert np.all(d[:, 2] - d[:, 1] > 20.0 * M)                    # every other row is clearly farther, to the first pass too
    # the f32 cell index of the LDS table (map.hip: (unsigned)(fl32(x - lo) * fl32(32 / r * (1 - 2^-18)))) falls BELOW the boundary
    for a in range(3):
        own = slice(24 * a, 24 * (a + 1))
        xf = (px[own, a] - lo[a]).astype(np.float32)
        im = np.float32(64.0 / r[a] * 0.5 * (1.0 - 2.0 ** -18))
        cell = (xf * im).astype(np.int64)
        true_cell = np.floor((px[own, a] - lo[a]) / (r[a] / 32.0)).astype(np.int64)
        assert np.array_equal(cell, true_cell - 1)
        assert np.all(pal[win[own], a] > px[own, a])


@pytest.mark.parametrize("density", nn_ref.CROWDED)
def test_crowded_counts(density):
    assert nn_ref.QUEUE == 48 and nn_ref.tile(1) == 256 and nn_ref.tile(4) == 128 and nn_ref.tile(8) == 128
    px, pal, over = nn_ref.crowded(density)
    idx, gap, ties = nn_ref.brute(px, pal)
    assert np.array_equal(ties == 8, over) and np.all(ties[~over] == 1)
    assert np.all(gap[~over] > 0.05)                               # far above any M: the first pass is clear there
    n = px.shape[0]
    if density == "none":
        assert not over.any()
    elif density == "sparse":
        assert 1 <= over.sum() <= n // 100
    elif density == "all":
        assert over.all()
    else:
        per128 = over.reshape(-1, 128).sum(axis=1)
        assert tuple(per128) == nn_ref.EXACT_COUNTS
        per256 = over.reshape(-1, 256).sum(axis=1)
        assert {48, 49, 96, 97} <= set(per128) | set(per256) and 48 in per256        # a queue filled exactly, by either tile size
