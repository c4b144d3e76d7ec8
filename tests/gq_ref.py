"""A model of the global quantiser from the 512-bucket MOMENT TABLE (the form the engine's two routes take it in), and the tables
the edge tests run: tests/test_gq_reference.py checks the model and the tables' properties on the CPU, tests/test_gpu_gq_edges.py
holds both routes of the engine to the model bit for bit.

The arithmetic is tests/independent_ref.py's (Cells' distortion / vcov / bias, should_terminate, dp_step, l_chain): this file only
builds `Cells` from a table instead of from pixels, injects the eigen-solver, keeps what the search leaves behind (every E_k, the
whole cut table, which branch of the termination test fired) and adds the bucket table and the base clusters' records
(global.c:328-335).  Plain numpy f64; np.cumsum adds in index order, as `table[i] += table[i-1]` does (cells.c:114-136).
"""
import numpy as np

from tests import independent_ref as ir

N = ir.BUCKETS
MAX_K = 12                                                            # global.c:23
RS = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]                 # quantities 4..9 of the table


class TableCells(ir.Cells):
    """independent_ref.Cells from a table (nq, 2, 512): the two parts of every entry are added first, as both routes do, then
    each quantity's inclusive prefix is one sequential chain.  `eigen(m) -> (info, w, V)` replaces LAPACK when given."""

    def __init__(self, table, counts, eigen=None):
        t = np.asarray(table, dtype=np.float64)
        t = t[:, 0, :] + t[:, 1, :]
        pre = lambda v: np.cumsum(np.concatenate(([0.0], v)))        # noqa: E731
        self.w0 = np.cumsum(np.concatenate(([0], np.asarray(counts, dtype=np.uint64)))).astype(np.uint64)
        self.w1 = np.stack([pre(t[r]) for r in range(3)])
        self.w2 = pre(t[3])
        self.wrs = {rs: pre(t[4 + i]) for i, rs in enumerate(RS)}
        self.eigen = eigen

    def axis(self, a, b):
        if self.eigen is None:
            return super().axis(a, b)
        info, _, v = self.eigen(self.vcov(a, b))
        return None if info != 0 else np.array(v[:, 2], dtype=np.float64)

    def prefix(self):
        """(10, 513): w1[0..2], w2, the six wrs -- the order of the table's quantities."""
        return np.stack([self.w1[0], self.w1[1], self.w1[2], self.w2] + [self.wrs[rs] for rs in RS])


class _Recorder:
    """What should_terminate asked of the cells, so that the branch it took can be named without restating its arithmetic."""

    def __init__(self, cells):
        self.cells, self.cd, self.cb, self.norms = cells, [], [], []

    def distortion(self, a, b):
        v = self.cells.distortion(a, b)
        self.cd.append(v)
        return v

    def bias(self, a, b, axis):
        v = self.cells.bias(a, b, axis)
        ca = self.cells.axis(a, b)
        if ca is not None:
            nrm = lambda u: np.sqrt((u[0] ** 2 + u[1] ** 2) + u[2] ** 2)     # noqa: E731
            self.norms.append(nrm(axis) * nrm(ca))
        self.cb.append(v)
        return v


def _branch(rec, stop):
    """Which way the termination test went: 'distortion' (< 1e-16), 'solver' (a cell's eigen-problem failed), 'bias' (< 0.1) or
    None (go on); plus whether a cell was skipped for cb < 0.9 and whether a cell's norms fell below 1e-16."""
    flags = dict(skipped=any(0 <= v < 0.9 for v in rec.cb), norms=any(v < ir.DELTA for v in rec.norms))
    if not rec.cb:
        return ("distortion" if stop else None), flags
    if any(v < 0 for v in rec.cb):
        return "solver", flags
    return ("bias" if stop else None), flags


def run(table, counts, weighted, K, eigen=None):
    """The global quantiser on a table.  Returns a dict:
    prefix_w0 (513,), prefix (10, 513); error; kbase; cuts; steps: per k tried, (k, branch, flags, cells before the test);
    E: {k: E_k} for k = 1 .. min(K, 12) (all of them, as the host route computes them); cut_full (13, 513): L after every step up
    to min(K, 12); cut_dev (13, 513): L after the steps the device route runs in full (2 .. kbase - 1);
    bucket_table (512,), begin / n / sw (kbase,), mean (kbase, 3)."""
    table = np.asarray(table, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.uint64)
    cells = TableCells(table, counts, eigen)
    out = dict(prefix_w0=cells.w0.copy(), prefix=cells.prefix(), error=0, kbase=0, cuts=[], steps=[], E={}, cells=cells)
    axis = cells.axis(0, N)
    if axis is None:
        out["error"] = 1
        return out
    kmax = min(MAX_K, K)
    E = np.zeros(N + 1)
    for i in range(1, N + 1):
        E[i] = cells.distortion(0, i)
    out["E"][1] = E
    L = {(i, i): i for i in range(0, MAX_K + 1)}                      # global.c:236-238
    result, stopped = ir.l_chain(L, 1), False
    for k in range(2, kmax + 1):
        if not stopped:
            rec = _Recorder(cells)
            stop = ir.should_terminate(result, axis, rec)
            branch, flags = _branch(rec, stop)
            out["steps"].append((k, branch, flags, list(result)))
            stopped = stop
        E = ir.dp_step(k, E, L, cells)                                # the host route runs every step, whatever the test said
        out["E"][k] = E
        if not stopped:
            result = ir.l_chain(L, k)
    kbase = len(result) - 1
    out.update(kbase=kbase, cuts=[int(v) for v in result], L=L)

    def dense(rows):
        m = np.zeros((MAX_K + 1, N + 1), dtype=np.int32)
        for (k, n), v in L.items():
            if k == n or k in rows:
                m[k, n] = v
        return m
    out["cut_full"] = dense(range(2, kmax + 1))
    out["cut_dev"] = dense(range(2, kbase))
    # global.c:328-335: bucket b belongs to the first cell j with b + 1 <= q[j + 1]
    owner = np.zeros(N, dtype=np.uint8)
    for b in range(N):
        for j in range(kbase):
            if b + 1 <= result[j + 1]:
                owner[b] = j
                break
    out["bucket_table"] = owner
    n = np.array([int(counts[owner == j].sum()) for j in range(kbase)], dtype=np.uint64)
    out["n"] = n
    out["begin"] = np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.uint64)
    sw, mean = np.zeros(kbase), np.zeros((kbase, 3))
    q0 = 10 if weighted else 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(kbase):
            m = owner == j
            part = lambda q: ir.seq_sum(table[q, 0, m]) + ir.seq_sum(table[q, 1, m])   # noqa: E731
            sw[j] = part(13) if weighted else float(n[j])
            inv = np.float64(1.0) / np.float64(sw[j])
            for q in range(3):
                mean[j, q] = part(q0 + q) * inv                       # an empty cluster: 0 * inf, NaN
    out["sw"], out["mean"] = sw, mean
    return out


def minima(cells, Eprev, k, n):
    """The candidates t of entry (k, n) that attain its minimum, ascending: t = n - 1 stands for E_{k-1}[n - 1] alone
    (global.c:252-253), every other t for E_{k-1}[t] + distortion(t, n)."""
    ts = np.arange(k - 1, n - 1)
    v = np.concatenate((Eprev[ts] + cells.distortion_to(ts, n), [Eprev[n - 1]]))
    return [int(t) for t in np.flatnonzero(v == v.min()) + (k - 1)]


# a grey whose channels differ a little, and (in band_image) a fiftieth of the ramp's width across it: a covariance of rank one
# exactly leaves its eigenvector's sign to the last bits of the sums (it flips with the summation order), a tie of the oracle's own
TINT = [1.0, 0.96, 0.9]


def band_image(levels, seed, weighted, w=96, h=64, width=0.001):
    """Grey bands: `levels` grey levels, one per horizontal band, each pixel `width` x random further along the grey axis.  Every
    band's own principal axis is the image's, so the global quantiser goes all the way to twelve base clusters, most of them empty.
    Returns (w, h, colours (n, 3) sRGB, weights or None)."""
    rng = np.random.default_rng(seed)
    n = w * h
    band = (np.arange(n) * levels) // n
    v = (0.15 + 0.7 * band / (levels - 1)) + width * rng.random(n)
    colors = np.ascontiguousarray(np.outer(v, TINT) + (width / 50) * rng.random((n, 3)))
    return w, h, colors, ((1.0 + 3.0 * rng.random(n)) if weighted else None)


# (levels, seed): the image-level cases of tests/test_gpu_gq_edges.py; tests/test_gq_reference.py shows the oracle tie-free on each
BAND_IMAGES = [(3, 1), (5, 2)]


# ---------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------
def table_from_pixels(c, bmap, w=None):
    """(table (10 or 14, 2, 512), counts): the buckets' moments of pixels c (n, 3) sorted into buckets bmap, everything in part 0.
    Sums run in pixel order (np.bincount), as independent_ref.Cells takes them."""
    c = np.asarray(c, dtype=np.float64)
    nq = 10 if w is None else 14
    t = np.zeros((nq, 2, N))
    bc = lambda v: np.bincount(bmap, weights=v, minlength=N)          # noqa: E731
    for r in range(3):
        t[r, 0] = bc(c[:, r])
    t[3, 0] = bc((c[:, 0] ** 2 + c[:, 1] ** 2) + c[:, 2] ** 2)
    for i, (r, s) in enumerate(RS):
        t[4 + i, 0] = bc(c[:, r] * c[:, s])
    if w is not None:
        for r in range(3):
            t[10 + r, 0] = bc(c[:, r] * w)
        t[13, 0] = bc(w)
    return t, np.bincount(bmap, minlength=N).astype(np.uint32)


def table_from_buckets(colors, counts, weights=None):
    """A table whose bucket b holds counts[b] pixels of the ONE colour colors[b] (and weight weights[b] each): every entry is
    count x a product of the colour's channels, exact when the colours are small dyadic numbers."""
    colors = np.asarray(colors, dtype=np.float64)
    cnt = np.asarray(counts, dtype=np.float64)
    nq = 10 if weights is None else 14
    t = np.zeros((nq, 2, N))
    for r in range(3):
        t[r, 0] = cnt * colors[:, r]
    t[3, 0] = cnt * ((colors[:, 0] ** 2 + colors[:, 1] ** 2) + colors[:, 2] ** 2)
    for i, (r, s) in enumerate(RS):
        t[4 + i, 0] = cnt * (colors[:, r] * colors[:, s])
    if weights is not None:
        wt = np.asarray(weights, dtype=np.float64)
        for r in range(3):
            t[10 + r, 0] = cnt * (colors[:, r] * wt)
        t[13, 0] = cnt * wt
    return t, np.asarray(counts, dtype=np.uint32)


def _sparse(occupied, colors, counts, weights=None):
    col, cnt = np.zeros((N, 3)), np.zeros(N, dtype=np.uint32)
    wt = None if weights is None else np.zeros(N)
    for i, b in enumerate(occupied):
        col[b], cnt[b] = colors[i], counts[i]
        if wt is not None:
            wt[b] = weights[i]
    return table_from_buckets(col, cnt, wt)


def _grey(v):
    return [float(v), float(v), float(v)]


def _bands(centres, spread, along, per=64, seed=0, weighted=False, target=None):
    """Pixels in bands around grey levels `centres`: within a band the pixels spread by `spread` ALONG the grey axis (the global
    axis) or ACROSS it; sorted into buckets by their position on the grey axis, as the engine's histogram would."""
    rng = np.random.default_rng(seed)
    g = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    x = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    pts = []
    for v in centres:
        u = rng.uniform(-1.0, 1.0, per)
        pts.append(np.outer(np.full(per, v), [1.0, 1.0, 1.0]) + np.outer(u * spread, g if along else x))
    c = np.concatenate(pts)
    if target is not None:                                            # scaled so that the total distortion is about `target`
        c = c * np.sqrt(target / float(np.sum((c - c.mean(axis=0)) ** 2)))
    d = c @ g
    ratio = (d - d.min()) / (d.max() - d.min())
    bmap = np.minimum((N * ratio).astype(np.int64), N - 1)
    w = rng.integers(1, 5, len(c)) / 4.0 if weighted else None
    return table_from_pixels(c, bmap, w)


def tables():
    """name -> dict(table, counts, weighted, dyadic, exact, props).  `dyadic`: every entry a small dyadic number, so that the
    records' sums are exact in any order.  `exact`: moreover every distortion and every E_k[n] of the search is exact in f64
    (tests/test_gq_reference.py proves it), so that ties are real ties.  `props`: what the table was chosen for, asserted on the
    model there (at K = 256 unless 'K' says otherwise)."""
    T = {}

    def add(name, tc, weighted=False, exact=False, dyadic=False, **props):
        T[name] = dict(table=tc[0], counts=tc[1], weighted=weighted, exact=exact, dyadic=dyadic or exact, props=props)

    # prefix stress: magnitudes over 2^+-30, signs mixed in the first moments and the off-diagonal products, both parts filled
    rng = np.random.default_rng(11)
    t = np.zeros((10, 2, N))
    for q in range(10):
        mag = np.exp2(rng.uniform(-30, 30, (2, N)))
        sign = rng.choice([-1.0, 1.0], (2, N)) if q in (0, 1, 2, 5, 7, 8) else 1.0
        t[q] = mag * sign
    add("prefix_stress", (t, rng.integers(1, 1000, N).astype(np.uint32)), differs_from_pairwise=True)
    # flat: all one colour
    add("flat_one_bucket", _sparse([7], [[0.5, 0.25, 0.125]], [4096]), exact=True, kbase=1, branch="distortion")
    add("flat_two_buckets", _sparse([0, 511], [[0.5, 0.25, 0.125]] * 2, [1024, 1024]), exact=True, kbase=1, branch="distortion", all_tie_cut=511)
    # plateau: three grey levels in buckets 1, 200, 512 (1-based); the two that are close get merged, so the one cut may sit
    # anywhere between them and the far one: a tied range of 199 (or 312) candidates, three lane wraps, t = n - 1 not in it
    add("plateau_low", _sparse([0, 199, 511], [_grey(0), _grey(8), _grey(9)], [64, 64, 64]), exact=True, K=2, cuts=[0, 199, 512],
        plateau=(1, 199))
    # ... and one wider than the 256 threads k_gq_dp strides by: there a thread holds two tied candidates of its own
    add("plateau_wide", _sparse([0, 399, 511], [_grey(0), _grey(8), _grey(9)], [64, 64, 64]), exact=True, K=2, cuts=[0, 399, 512],
        plateau=(1, 399))
    add("plateau_high", _sparse([0, 199, 511], [_grey(0), _grey(1), _grey(9)], [64, 64, 64]), exact=True, K=2, cuts=[0, 511, 512],
        plateau=(200, 511))
    # exact six colours with gaps (multiples of 27720 = lcm(1..12) over 64, so that a cell's squared sum divides by its members)
    six = [0, 100, 101, 300, 301, 511]
    sixv = [_grey(v / 64.0) for v in (0, 27720, 277200, 554400, 609840, 1108800)]
    add("six_colours", _sparse(six, sixv, [64] * 6), exact=True, kbase=6, branch="distortion", cuts=[0, 100, 101, 300, 301, 511, 512],
        K4_cuts=[0, 101, 300, 511, 512], empty_cell=False)
    add("six_colours_weighted", _sparse(six, sixv, [64] * 6, [0.5, 1.0, 2.0, 0.25, 4.0, 1.0]), weighted=True, exact=True, kbase=6,
        branch="distortion", cuts=[0, 100, 101, 300, 301, 511, 512])
    # uniform exact gradient: 512 equal buckets of evenly spaced greys
    add("gradient", table_from_buckets(np.outer(np.arange(N) / 64.0, [1.0, 1.0, 1.0]), np.full(N, 16)), exact=True, kbase=12, branch=None,
        symmetric=True)
    # carry-over: two heavy far-apart first buckets, then 510 light buckets near the middle
    col = np.zeros((N, 3))
    col[0], col[1] = _grey(-4096), _grey(4096)
    col[2:] = np.outer((np.arange(510) - 255) / 64.0, [1.0, 1.0, 1.0])
    cnt = np.full(N, 1, dtype=np.uint32)
    cnt[0] = cnt[1] = 1 << 20
    add("carry_over", table_from_buckets(col, cnt), dyadic=True, kbase=12, cuts_head=[0, 1, 3])
    # along-axis bands: every band's own axis is the global one, so the bias test never stops the search and the dynamic
    # programme runs out of occupied buckets
    add("bands3_along", _bands([0.2, 0.5, 0.8], 0.001, True, seed=1), kbase=12, empty_cell=True)
    add("bands5_along", _bands([0.1, 0.3, 0.5, 0.7, 0.9], 0.001, True, seed=2), kbase=12, empty_cell=True)
    add("bands3_along_weighted", _bands([0.2, 0.5, 0.8], 0.001, True, seed=3, weighted=True), weighted=True, kbase=12, empty_cell=True)
    # the bands' spread ACROSS the axis: each cell's axis is orthogonal to the global one, cb < 0.9, the bias sum stays 0
    add("bands2_across", _bands([0.25, 0.75], 0.01, False, seed=4), kbase=2, branch="bias", skipped=True)
    # threshold pair: one elongated cloud scaled so that the total distortion falls just either side of 1e-16
    add("threshold_below", _bands([0.5], 0.5, True, per=256, seed=5, target=0.98e-16), kbase=1, branch="distortion", total=(0.9e-16, 1e-16))
    add("threshold_above", _bands([0.5], 0.5, True, per=256, seed=5, target=1.02e-16), kbase_at_least=2, total=(1e-16, 1.1e-16))
    # a cell of a single pixel: zero covariance
    add("single_pixel_cell", _sparse([0, 255, 256, 511], [_grey(0), _grey(4), _grey(5), _grey(64)], [64, 64, 64, 1]), dyadic=True,
        single_pixel=True)
    # stop at every step: m distinct equally spaced grey levels stop on `distortion < 1e-16` with m cells
    for m in range(2, 12):
        if m == 6:
            continue
        occ = [int(round(i * 511 / (m - 1))) for i in range(m)]
        add("levels_%d" % m, _sparse(occ, [_grey(27720 * i / 64.0) for i in range(m)], [64] * m), exact=True, kbase=m, branch="distortion")
    return T
