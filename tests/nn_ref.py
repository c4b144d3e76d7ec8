"""The nearest map's reference in numpy and the constructed inputs of tests/test_nn_reference.py (CPU) and tests/test_gpu_nn_edges.py.

The reference (oracle/patolette_oracle.c: orc_nn_map) is dist = (d0*d0 + d1*d1) + d2*d2 in f64 over every palette row in ascending
order with a strict '<' from bd = +Inf: the lowest index wins a tie, and a pixel whose distances are all NaN or +Inf keeps index 0.
On the device three routes stand behind that promise (patolette_amd/csrc/map.hip); the generators aim at what each of them rests on:
exact ties and near-ties (`lattice`, `lattice_shifted`), the f32 first pass and its ambiguity margin M (`margin_sweep`, `f32_pass`),
cell boundaries of both grids (`cell_edges`, `edge_bisectors`) and the overflow queues of the LDS-table kernel (`crowded`).
Everything is deterministic.  Pixels and palettes are (n, 3) / (k, 3) float64 rows."""
import numpy as np

# ---- constants of patolette_amd/csrc/map.hip, restated from its formulas ----------------------------------------------------------
MID_LDS_FIXED = 131072 + 256 * 16 + 3 * 256 * 8          # kMidLdsFixed: the 32^3 table, the f32 records, the f64 palette


def mid_queue(waves=16, extra=0):
    """mid_queue() of map.hip: parked pixels per wavefront (28 B each) in what the table leaves of the CU's 160 KB."""
    q = (163840 - MID_LDS_FIXED - extra) // (waves * 28)
    return 64 if q > 64 else q & ~3


QUEUE = mid_queue(16)                                      # 48 for the planar source (k_nn_map_mid<.., 16, NNSrcPlanes>)
LANES = 64


def tile(elem_bytes):
    """pixels of one tile of k_nn_map_mid: 64 lanes x P, P = 4 for 1-byte map elements, 2 otherwise"""
    return LANES * (4 if elem_bytes == 1 else 2)


def margin_M(pal, lo, hi):
    """M = 2.5 * 1.001 * 2^-24 * (9 max_j |p_j - lo|^2 + 5 |hi - lo|^2), k_nn_lut_coarse's expression (lo, hi: the pixels' box)."""
    a = np.asarray(pal, dtype=np.float64) - lo
    wmax = float(np.max((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]))
    r = np.asarray(hi, dtype=np.float64) - lo
    return 2.5 * 1.001 * 2.0 ** -24 * (9.0 * wmax + 5.0 * float(np.sum(r * r)))


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def brute(px, pal, chunk=8192):
    """(index, gap, ties): the reference's arg-min per pixel, second smallest minus smallest distance (Inf for k == 1, NaN where the
    distances are not finite), and how many rows attain the minimum."""
    px = np.asarray(px, dtype=np.float64)
    pal = np.asarray(pal, dtype=np.float64)
    n, k = px.shape[0], pal.shape[0]
    idx = np.zeros(n, dtype=np.int64)
    gap = np.full(n, np.inf)
    ties = np.zeros(n, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, n, chunk):
            c = px[s:s + chunk]
            d0, d1, d2 = (c[:, None, a] - pal[None, :, a] for a in range(3))
            d = (d0 * d0 + d1 * d1) + d2 * d2
            dd = np.where(np.isnan(d), np.inf, d)                 # a NaN is never '<'
            best = np.argmin(dd, axis=1)                           # the first minimum = the lowest index
            mn = dd[np.arange(c.shape[0]), best]
            idx[s:s + chunk] = np.where(np.isinf(mn), 0, best)     # nothing was ever below +Inf: index 0 stays
            ties[s:s + chunk] = np.sum(dd == mn[:, None], axis=1)
            if k > 1:
                two = np.partition(dd, 1, axis=1)[:, :2]
                gap[s:s + chunk] = two[:, 1] - two[:, 0]
    return idx, gap, ties


def brute_int(px, pal, scale_bits=20):
    """The arg-min (lowest index on ties) in int64 arithmetic on coordinates scaled by 2^scale_bits; they must be integers then."""
    sc = float(1 << scale_bits)
    P, Q = np.asarray(px) * sc, np.asarray(pal) * sc
    assert np.all(P == np.round(P)) and np.all(Q == np.round(Q)) and max(np.abs(P).max(), np.abs(Q).max()) < 2 ** 30
    P, Q = P.astype(np.int64), Q.astype(np.int64)
    out = np.zeros(P.shape[0], dtype=np.int64)
    for s in range(0, P.shape[0], 8192):
        d = ((P[s:s + 8192, None, :] - Q[None, :, :]) ** 2).sum(axis=2)
        out[s:s + 8192] = np.argmin(d, axis=1)
    return out


# ---- exact ties ---------------------------------------------------------------------------------------------------------------------
def lattice_palette():
    """The 5^3 points on multiples of 1/4 in [0, 1]^3, rows shuffled: "lowest index" is not geometric."""
    g = np.arange(5) / 4.0
    pal = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(pal[np.random.default_rng(1234).permutation(125)])


def lattice():
    """(pixels, palette): all 33^3 corners of the 32^3 grid on the lattice palette.  Every coordinate is dyadic, the f64 distances are
    exact, and 30 % of the pixels are equidistant from 2, 4 or 8 rows -- each of them on a cell boundary of both grids."""
    g = np.arange(33) / 32.0
    px = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(px), lattice_palette()


def lattice_shifted(s):
    """The lattice's pixels moved by +-2^-s along x (random sign, clipped to [0, 1]): a few ulps to a few M off the bisectors."""
    px, pal = lattice()
    sign = np.random.default_rng(100 + s).integers(0, 2, size=px.shape[0]) * 2.0 - 1.0
    px = px.copy()
    px[:, 0] = np.clip(px[:, 0] + sign * 2.0 ** -s, 0.0, 1.0)
    return px, pal


def tie8_points():
    """The 4^3 centres of the lattice's cubes: each equidistant from eight palette rows (and a corner of eight cells of either grid)"""
    g = (2 * np.arange(4) + 1) / 8.0
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


# ---- the f32 first pass and its margin ----------------------------------------------------------------------------------------------
BOXES = {
    "unit": (np.zeros(3), np.ones(3)),
    "tiny-flat": (np.array([0.5 - 2.0 ** -21, 0.5 - 2.0 ** -21, 0.5]), np.array([0.5 + 2.0 ** -21, 0.5 + 2.0 ** -21, 0.5])),   # width 2^-20, one degenerate axis
    "shifted": (np.full(3, 1000.0), np.full(3, 1000.5)),
    "unit-far": (np.zeros(3), np.ones(3)),                                 # a quarter of the palette moved out by +5: M grows with wmax
}


def margin_sweep(k, box):
    """(pixels, palette, lo, hi, M).  Palette: k distinct rows on multiples of 2^-10 of the box.  For each row i inside the box and its
    nearest row j, 513 pixels on the line through their midpoint along j - i at offsets m * 8 t_M / 256, m = -256 .. 256, where
    t_M = M / (2 |p_j - p_i|) is the offset at which the two squared distances differ by M: the gaps run from 0 to 8 M in steps of M / 32.
    Behind them, per row, twenty pixels with gaps of +-M / 32 .. +-M / 16384 off the dyadic line (see below).
    Coordinates are rounded to multiples of 2^-40 of the box and clipped to it; the box's corners come last, so that the device's
    min / max finds this box and this M."""
    lo, hi = (np.array(v, dtype=np.float64) for v in BOXES[box])
    r = hi - lo
    rng = np.random.default_rng(77 + k)
    codes = rng.choice(1025 ** 3, size=k, replace=False)
    grid = np.stack([codes % 1025, (codes // 1025) % 1025, codes // (1025 * 1025)], axis=1).astype(np.float64)
    pal = lo + r * (grid / 1024.0)
    inside = np.ones(k, dtype=bool)
    if box == "unit-far":
        inside[::4] = False
        pal[::4] += 5.0
    M = margin_M(pal, lo, hi)
    m = np.arange(-256, 257, dtype=np.float64)
    rows, fine = [], []
    for i in np.nonzero(inside)[0]:
        d = pal - pal[i]
        d2 = np.sum(d * d, axis=1)
        d2[i] = np.inf
        j = int(np.argmin(d2))
        dist = np.sqrt(d2[j])
        t = m * (8.0 * (M / (2.0 * dist)) / 256.0)
        u = d[j] / dist
        rows.append(0.5 * (pal[i] + pal[j]) + t[:, None] * u[None, :])
        # ... and twenty finer ones, gaps of +-M / 32 down to +-M / 16384, each moved ACROSS the line by a random amount (which leaves
        # the gap alone): the palette and the line above are dyadic enough for the f32 pass to be exact, these are not
        v = np.cross(u, [0.0, 0.0, 1.0])
        if np.sum(v * v) < 1e-6:
            v = np.cross(u, [1.0, 0.0, 0.0])
        v /= np.sqrt(np.sum(v * v))
        tf = np.concatenate([sg * (M / (2.0 * dist)) * 2.0 ** -np.arange(5, 15) for sg in (-1.0, 1.0)])
        fine.append(0.5 * (pal[i] + pal[j]) + tf[:, None] * u[None, :] + (rng.uniform(-0.02, 0.02, size=20) * dist)[:, None] * v[None, :])
    px = np.concatenate(rows + fine)
    q = np.where(r > 0, r, 1.0) * 2.0 ** -40
    px = np.clip(lo + np.round((px - lo) / q) * q, lo, hi)
    corners = np.array([[lo[0] if c & 1 else hi[0], lo[1] if c & 2 else hi[1], lo[2] if c & 4 else hi[2]] for c in range(8)])
    return np.concatenate([px, corners]), pal, lo, hi, M


def f32_pass(px, pal, lo, hi):
    """numpy model of k_nn_map_mid's first pass over ALL rows: t[i, j] = fma(xf0, q0, fma(xf1, q1, fma(xf2, q2, w))) with the records
    {-2 (p - lo), |p - lo|^2} rounded to f32 (w = (a*a + b*b) + c*c in f64, rounded once), xf = fl32(x - lo), each fma taken through
    f64 (the product of two f32 is exact there).  Returns (t, exact) with exact = |x - p_j|^2 - |x - lo|^2 in f64."""
    f32, f64 = np.float32, np.float64
    a = np.asarray(pal, dtype=f64) - lo
    w = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).astype(f32)
    q = (-2.0 * a).astype(f32)
    xs = np.asarray(px, dtype=f64) - lo
    xf = xs.astype(f32)

    def fma(u, v, c):
        return (u.astype(f64) * v.astype(f64) + c.astype(f64)).astype(f32)
    t = fma(xf[:, None, 2], q[None, :, 2], np.broadcast_to(w[None, :], (xs.shape[0], a.shape[0])))
    t = fma(xf[:, None, 1], q[None, :, 1], t)
    t = fma(xf[:, None, 0], q[None, :, 0], t)
    exact = -2.0 * (xs @ a.T) + np.sum(a * a, axis=1)[None, :]
    return t, exact


# ---- cell boundaries ----------------------------------------------------------------------------------------------------------------
def random_box(seed=5):
    """a non-dyadic box: (lo, hi) with hi - lo as the device takes it from the pixels' min / max"""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-0.3, 0.2, size=3)
    hi = lo + rng.uniform(0.3, 1.1, size=3)
    return lo, hi


def box_palette(k, lo, hi, seed=9):
    return lo + (hi - lo) * np.random.default_rng(seed + k).random((k, 3))


def cell_edges(G, lo, hi):
    """Pixels on and next to every cell boundary of a G^3 grid over the box: on each axis and for every i in 0 .. G the device's own
    lo + i * (r / G), its two f64 neighbours, and lo + (i / G +- delta) * r for delta = 1e-9 .. 5e-6 (the widening of the G^3 boxes is
    1e-9, that of the LDS table 1e-5, the f32 cell index is off by up to 4e-6, all of the range); the other two coordinates random.
    Clipped to the box; its corners come last."""
    rng = np.random.default_rng(31 + G)
    r = hi - lo
    out = []
    for a in range(3):
        i = np.arange(G + 1, dtype=np.float64)
        x = lo[a] + i * (r[a] / G)
        xs = [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
        for delta in (1e-9, 1e-7, 1e-6, 3e-6, 5e-6):
            xs += [lo[a] + (i / G - delta) * r[a], lo[a] + (i / G + delta) * r[a]]
        xs = np.concatenate(xs)
        p = lo + r * rng.random((xs.shape[0], 3))
        p[:, a] = xs
        out.append(p)
    corners = np.array([[lo[0] if c & 1 else hi[0], lo[1] if c & 2 else hi[1], lo[2] if c & 4 else hi[2]] for c in range(8)])
    return np.concatenate([np.clip(np.concatenate(out), lo, hi), corners])


def edge_bisectors(lo, hi):
    """(pixels, palette, winners): a bisector just inside the NEXT cell of the LDS table.  For boundaries b = lo + i r / 32, i = 17, 19,
    .. 31, on each axis: a pair of rows at b + eps -+ r / 32 (eps = 5e-7 r; same transverse coordinates, the centre of a cell, far from
    every other pair) and pixels at b + delta, delta = 6e-7, 1e-6, 1.5e-6 of r: beyond the bisector, so the upper row wins -- but
    k_nn_map_mid's f32 cell index, (i + 32 delta / r) (1 - 2^-18), puts them into the cell BELOW b, over whose exact box the upper row is
    strictly farther than the lower one.  Only the 1e-5 widening of that table's boxes keeps the upper row in that cell's list."""
    rng = np.random.default_rng(17)
    r = hi - lo
    spots = rng.permutation(64)                                            # transverse cells of an 8 x 8 raster: pairs stay r / 8 apart
    pal, px, win = [], [], []
    for a in range(3):
        for t, i in enumerate(range(17, 33, 2)):
            u, v = divmod(int(spots[8 * a + t]), 8)
            c = lo + r * np.roll(np.array([0.0, (8 * u + 3) / 64.0, (8 * v + 3) / 64.0]), a)   # axis a takes the boundary, the other two the spot
            c[a] = lo[a] + i * (r[a] / 32.0) + 5e-7 * r[a]
            for sgn in (-1.0, 1.0):
                p = c.copy()
                p[a] += sgn * r[a] / 32.0
                pal.append(p)
            for delta in (6e-7, 1e-6, 1.5e-6):
                x = c.copy()
                x[a] = lo[a] + i * (r[a] / 32.0) + delta * r[a]
                px.append(x)
                win.append(len(pal) - 1)
    corners = np.array([[lo[0] if c & 1 else hi[0], lo[1] if c & 2 else hi[1], lo[2] if c & 4 else hi[2]] for c in range(8)])
    return np.concatenate([np.array(px), corners]), np.array(pal), np.array(win)


# ---- the overflow queues of the LDS-table kernel ------------------------------------------------------------------------------------
CROWDED = ("none", "sparse", "exact", "all")
# overflow pixels per block of 128 pixels (the 4-byte tile; two make a 1-byte tile): a queue of QUEUE filled exactly by one tile (48),
# by two halves (24 + 24), filled and one more (49), twice over and one more (48 + 49), and nearly (47 + 1 fills it at the tile's end)
EXACT_COUNTS = (QUEUE, QUEUE + 1, QUEUE // 2, QUEUE // 2, QUEUE, 0, 2 * QUEUE, 0, QUEUE - 1, 1, 64, 33)


def crowded(density, n=None):
    """(pixels, palette) on the lattice palette.  An "overflow" pixel sits on an eight-way tie (tie8_points): its cell of the LDS table
    has more than four survivors, so k_nn_map_mid parks it in its wavefront's queue.  Every other pixel sits 1/64 off a palette row in
    the middle of a cell, where the first pass is clear.  density: "none"; "sparse" (one in a thousand); "exact" (EXACT_COUNTS per
    block of 128 pixels, at random places); "all"."""
    assert density in CROWDED
    pal = lattice_palette()
    rng = np.random.default_rng(400 + CROWDED.index(density))
    if n is None:
        n = 128 * len(EXACT_COUNTS) if density == "exact" else 3000
    over = np.zeros(n, dtype=bool)
    if density == "sparse":
        over = rng.random(n) < 1e-3
        over[n // 2] = True
    elif density == "exact":
        for b in range(n // 128):
            over[128 * b + rng.permutation(128)[:EXACT_COUNTS[b % len(EXACT_COUNTS)]]] = True
    elif density == "all":
        over[:] = True
    inner = pal[rng.integers(0, 125, size=n)]
    px = np.where(inner < 1.0, inner + 1.0 / 64.0, inner - 1.0 / 64.0)
    t8 = tie8_points()
    px[over] = t8[rng.integers(0, 64, size=int(over.sum()))]
    return np.ascontiguousarray(px), pal, over
