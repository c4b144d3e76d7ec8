"""The dither's nearest-colour searches at their edges: a model of the chain, the probe / reset construction that places a query of
the test's choosing inside the real chain, the lane layout's host arithmetic restated, and the generators of
tests/test_dither_reference.py (CPU) and tests/test_gpu_dither_edges.py.

The chain (oracle/patolette_oracle.c: orc_dither_riemersma) pushes `original pixel - chosen colour` into its queue of sixteen errors;
what it diffused into the pixel is not part of that.  A pixel whose colour IS a palette row and which chooses a row of that colour
pushes exactly 0, sixteen such pixels in a row empty the queue, and the query of the step after them is exactly
(kRw p0, kGw p1, kBw p2) of its pixel p.  `layout` lays an image out along the curve as probe, 16 x anchor, probe, 16 x anchor, ...:
every seventeenth step is a nearest-colour query chosen here.  An anchor is a palette colour that every one of the sixteen queries
of the reset (the probe's error e ages through the weights w[15] .. w[0]) maps onto itself; the search for one is plain brute force.

Pixels and palettes are (n, 3) / (k, 3) float64 rows in the dither's space (linear Rec2020); "weighted" is that space scaled by the
reference's three channel weights -- the DOUBLE constants for a query, their float casts for the palette (riemersma.c:305-311,
419-425).  Everything is deterministic."""
import numpy as np

from tests import nn_ref

KW = np.array([0.51254268114958, 0.8234075540095561, 0.2435159132377184])            # riemersma.c:38-42
FW = KW.astype(np.float32).astype(np.float64)
RESET = 16                                                                             # anchors behind every probe
STRIDE = RESET + 1


def weights():
    """w_i = m^i / 16, m = 16^(1/15) (riemersma.c:360-373)"""
    m = np.exp(np.log(16.0) / (16.0 - 1))
    w = np.zeros(16)
    v = 1.0
    for i in range(16):
        w[i] = v / 16.0
        v *= m
    return w


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def queries(seq, pal, map_seq):
    """The weighted-space query of every step of the chain over the pixels `seq` (curve order) that made the choices `map_seq`: the
    errors pixel - pal[choice] of the sixteen steps before, summed in the reference's order ((0 + q0 w0) + q1 w1) + ... ."""
    seq = np.asarray(seq, dtype=np.float64)
    n = seq.shape[0]
    w = weights()
    with np.errstate(invalid="ignore", over="ignore"):
        pad = np.concatenate([np.zeros((16, 3)), seq - np.asarray(pal)[np.asarray(map_seq, dtype=np.int64)]])
        e = np.zeros((n, 3))
        for i in range(16):
            e = e + pad[i:i + n] * w[i]
        return KW * (seq + e)


def replay(seq, pal, map_seq):
    """(queries, index, gap, ties): nn_ref.brute over the replayed queries -- equals map_seq iff map_seq is the reference's chain"""
    q = queries(seq, pal, map_seq)
    if q.shape[0] <= 200000:
        return (q,) + nn_ref.brute(q, np.asarray(pal) * FW)
    uq, inv = np.unique(q, axis=0, return_inverse=True)                             # (the large images are mostly one fill colour)
    return (q,) + tuple(v[inv.reshape(-1)] for v in nn_ref.brute(uq, np.asarray(pal) * FW))


def to_sequence(flat, order):
    """planar image (3 n) -> (n, 3) pixels in curve order"""
    n = order.shape[0]
    return np.stack([flat[c * n:(c + 1) * n][order] for c in range(3)], axis=1)


# ---- probes between resets ------------------------------------------------------------------------------------------------------------
class Layout:
    """image: planar (3 n); seq: the same pixels in curve order; ranks: curve rank of every probe kept; kept: their numbers among the
    probes given; dropped: the numbers of those without an anchor (their slots hold the fill colour)."""

    def __init__(self, image, seq, ranks, kept, dropped, width, height, pal):
        self.image, self.seq, self.ranks, self.kept, self.dropped = image, seq, ranks, kept, dropped
        self.width, self.height, self.pal = width, height, pal


def default_ranks(n, m=None):
    slots = (n - RESET) // STRIDE if m is None else m
    return np.arange(slots, dtype=np.int64) * STRIDE


def sparse_ranks(n, dense=70000, scattered=3000, seed=1):
    """probes in the first `dense` curve positions, and `scattered` more at random places behind them (the 1024 x 1024 images)"""
    a = np.arange(dense // STRIDE, dtype=np.int64) * STRIDE
    cells = np.arange(dense // STRIDE + 1, (n - STRIDE) // STRIDE, dtype=np.int64)
    b = np.sort(np.random.default_rng(seed).choice(cells, size=scattered, replace=False)) * STRIDE
    return np.concatenate([a, b])


def find_anchors(probes, pal, ntry=6):
    """per probe the number of a DISTINCT colour of the palette that holds through its reset, or -1; and the distinct colours.
    Tried: the `ntry` colours that stick out furthest along the probe's error."""
    pal = np.asarray(pal, dtype=np.float64)
    ucol = np.unique(pal, axis=0)
    ucw = ucol * FW
    w = weights()
    with np.errstate(invalid="ignore", over="ignore"):
        choice = nn_ref.brute(KW * probes, pal * FW)[0]
        e = probes - pal[choice]
        score = np.nan_to_num((e * KW) @ ucw.T, nan=0.0, posinf=0.0, neginf=0.0)
    cand = np.argsort(-score, axis=1, kind="stable")[:, :min(ntry, ucol.shape[0])]
    anchor = np.full(probes.shape[0], -1, dtype=np.int64)
    for t in range(cand.shape[1]):
        todo = np.nonzero(anchor < 0)[0]
        if todo.size == 0:
            break
        c = cand[todo, t]
        with np.errstate(invalid="ignore", over="ignore"):
            cor = ucol[c][:, None, :] + e[todo][:, None, :] * w[None, :, None]       # the sum of a queue with one slot set is that slot's term
            idx, gap, ties = nn_ref.brute((KW * cor).reshape(-1, 3), ucw)
        ok = np.all((idx.reshape(-1, 16) == c[:, None]) & (ties.reshape(-1, 16) == 1), axis=1)
        anchor[todo[ok]] = c[ok]
    return anchor, ucol


def layout(probes, pal, order, width, height, ranks=None, fill=None, anchors=None):
    """The image whose chain asks for KW * probes[i] at curve rank ranks[i].  ranks: ascending, STRIDE apart at least (default: every
    seventeenth).  fill: the pixel of every other position (default: the first palette row's colour: zero error from a zero queue).
    anchors: (anchor numbers, distinct colours) where the caller has them."""
    pal = np.asarray(pal, dtype=np.float64)
    probes = np.asarray(probes, dtype=np.float64)
    n = order.shape[0]
    assert n == width * height
    ranks = default_ranks(n, probes.shape[0]) if ranks is None else np.asarray(ranks, dtype=np.int64)[:probes.shape[0]]
    probes = probes[:ranks.shape[0]]
    assert np.all(np.diff(ranks) >= STRIDE) and ranks[-1] + RESET < n
    anchor, ucol = find_anchors(probes, pal) if anchors is None else anchors
    seq = np.empty((n, 3))
    seq[:] = pal[0] if fill is None else fill
    ok = anchor >= 0
    seq[ranks[ok]] = probes[ok]
    for s in range(1, RESET + 1):
        seq[ranks[ok] + s] = ucol[anchor[ok]]
    image = np.empty(3 * n)
    for c in range(3):
        image[c * n:(c + 1) * n][order] = seq[:, c]
    return Layout(image, seq, ranks[ok], np.nonzero(ok)[0], np.nonzero(~ok)[0], width, height, pal)


# ---- the lane layout's host arithmetic (csrc/dither_host.h), restated -----------------------------------------------------------------
class Geometry:
    """lo, hi, inv (and cw, the cell widths): (3 grids, 3 axes); G: (3,); amb, amb_p, amb_x: float32"""

    def __init__(self, lo, hi, inv, G, amb, amb_p, amb_x):
        self.lo, self.hi, self.inv, self.G, self.amb, self.amb_p, self.amb_x = lo, hi, inv, G, amb, amb_p, amb_x


def _f32_up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def lane_geometry(pal, npix):
    """the three grids over the weighted palette's box (+- 1/2 extent + 1e-3; +- 1 1/2 extents + 5e-3; +- 4 extents + 1e-2) and the
    margins of the f32 first pass, expression by expression as the host forms them"""
    wp = np.asarray(pal, dtype=np.float64) * FW
    G0 = 64 if npix >= 1 << 20 else 32
    # (the host folds with std::min / std::max from +-inf, which never take a NaN: fmin / fmax, not min / max)
    lo, hi = np.fmin.reduce(np.vstack([np.full(3, np.inf), wp])), np.fmax.reduce(np.vstack([np.full(3, -np.inf), wp]))
    with np.errstate(invalid="ignore"):
        r = hi - lo
    r = np.where((r > 0) & np.isfinite(r), r, 0.0)
    glo, ghi, ginv, GG = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3)), np.array([G0, G0, 32])
    m = 0.5 * r + 1e-3
    glo[0] = lo - m
    Rg = r + 2 * m
    ginv[0] = G0 / Rg
    gcw = np.zeros((3, 3))
    gcw[0] = Rg / G0
    ghi[0] = glo[0] + Rg
    for lv in (0, 1):
        mo = (1.5 if lv == 0 else 4.0) * r + (5e-3 if lv == 0 else 1e-2)
        Ro = r + 2 * mo
        glo[lv + 1] = lo - mo
        ginv[lv + 1] = GG[lv + 1] / Ro
        gcw[lv + 1] = Ro / GG[lv + 1]
        ghi[lv + 1] = glo[lv + 1] + Ro
    t = wp - glo[0]
    wmax = float(np.fmax.reduce(np.concatenate([[0.0], ((0.0 + t[:, 0] * t[:, 0]) + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]])))
    t = ghi[0] - glo[0]
    r2 = float(((0.0 + t[0] * t[0]) + t[1] * t[1]) + t[2] * t[2])
    M = 2.5 * 1.001 * 2.0 ** -24 * (9.0 * wmax + 5.0 * r2)
    amb = np.float32(M)
    if float(amb) < M:
        amb = _f32_up(amb)
    if not M < 3.0e38:
        amb = np.float32(np.inf)
    Mp, Mx = 2.5 * 1.002 * 2.0 ** -24 * 9.0 * wmax, 2.5 * 1.002 * 2.0 ** -24 * 5.0
    amb_p, amb_x = _f32_up(Mp), _f32_up(Mx)
    if not Mp < 3.0e38:
        amb_p = np.float32(np.inf)
    geo = Geometry(glo, ghi, ginv, GG, amb, amb_p, amb_x)
    geo.cw = gcw
    return geo


# the two cuts, the layout rule and the stall rule (csrc/dither_host.h), restated from the kernels' limits: integers throughout
def lanes_possible(frames, n, k):
    """a run of 64 pixels in every frame, one tile row per 8 runs (grid.y <= 65535), the pruned search's palette sizes"""
    return frames > 0 and n >= 64 and frames <= 8 * 65535 and 8 <= k <= 256


def lane_rule(segments, lanes, npix, k):
    """the lane layout: 8 <= k <= 256, not the single chain, not switched off; from 2^23 pixels, or from 2^16 when asked for"""
    if not 8 <= k <= 256 or segments == 1 or lanes == 0:
        return False
    return npix >= (65536 if lanes > 0 else 1 << 23)


def lane_cut(segments, warm, cus, npix, nframe, frames):
    """(S, Lmax, fruns, warm) of the lane layout: 512 runs per CU, none shorter than 256 pixels unless asked for, never shorter than 64,
    8 * 65535 at the most; a stack of frames: the same per frame, every frame the same number of runs"""
    auto = min(cus * 512, npix // 256)
    S = max(1, min(segments if segments > 0 else auto, npix // 64, 8 * 65535))
    fruns = 0
    if frames > 1:
        per = -(-segments // frames) if segments > 0 else auto // frames
        fruns = max(1, min(per, nframe // 64, 8 * 65535 // frames))
        S = frames * fruns
    return S, -(-npix // S), fruns, min(warm if warm >= 0 else 256, npix // S)


def wave_cut(segments, warm, cus, npix, width, height):
    """(S, warm) of the wavefront layout: 8 runs per CU, none shorter than the warm-up (256 at least) unless asked for, never shorter
    than 128; one chain for an image under 16 pixels across"""
    warm = warm if warm >= 0 else 1024
    S = segments if segments > 0 else min(cus * 8, npix // max(warm, 256))
    S = min(S, npix // 128)
    if max(width, height) < 16:
        S = 1
    return max(S, 1), warm


def stall_steps(counts):
    """per verification pass: how many passes in a row left work that had not dropped by an eighth (one at least) of the pass before"""
    out, prev, stalled = [], None, 0
    for n in counts:
        stalled = stalled + 1 if prev is not None and n + max(1, prev // 8) >= prev else 0
        prev = n
        out.append(stalled)
    return out


def nn_cell(q, lo, inv, G):
    """nn_cell of map.hip: per axis (int)((x - lo) inv) clamped into 0 .. G - 1; the cell number (z G + y) G + x"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.trunc((q - lo) * inv)
    i = np.clip(np.nan_to_num(f, nan=0.0, posinf=float(G), neginf=-1.0), 0, G - 1).astype(np.int64)
    return (i[:, 2] * G + i[:, 1]) * G + i[:, 0]


def grid_level(q, geo):
    """0, 1, 2: the first grid that holds the query (x >= lo && x <= hi on every axis; a NaN is in none); 3: outside all three"""
    lv = np.full(q.shape[0], 3, dtype=np.int64)
    for g in (2, 1, 0):
        with np.errstate(invalid="ignore"):
            inside = np.all((q >= geo.lo[g]) & (q <= geo.hi[g]), axis=1)
        lv[inside] = g
    return lv


def query_margin(q, geo):
    """the margin of the f32 first pass per query (as f64): amb inside the first grid, amb_p + amb_x |fl32(x - lo)|^2 outside"""
    with np.errstate(invalid="ignore", over="ignore"):
        xf = (q - geo.lo[0]).astype(np.float32).astype(np.float64)
        n2 = (xf[:, 0] * xf[:, 0] + (xf[:, 1] * xf[:, 1] + (xf[:, 2] * xf[:, 2]).astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
              ).astype(np.float32).astype(np.float64)
        out = (float(geo.amb_x) * n2 + float(geo.amb_p)).astype(np.float32).astype(np.float64)
    return np.where(grid_level(q, geo) == 0, float(geo.amb), out)


class Tables:
    """the record tables as patolette_amd_debug_dither_lane_tables returns them: per grid G^3 first records, then G^3 second ones"""

    def __init__(self, raw, G):
        self.first, self.second = [], []
        at = 0
        for g in G:
            c = int(g) ** 3
            self.first.append(raw[at:at + 16 * c].reshape(c, 16))
            self.second.append(raw[at + 16 * c:at + 32 * c].reshape(c, 16))
            at += 32 * c

    def records(self, q, geo):
        """(level, count, entries (n, 30)) of the record the kernel reads for every query; level 3: none (count 255)"""
        lv = grid_level(q, geo)
        cnt = np.full(q.shape[0], 255, dtype=np.int64)
        ent = np.zeros((q.shape[0], 30), dtype=np.int64)
        for g in range(3):
            at = np.nonzero(lv == g)[0]
            if at.size:
                cell = nn_cell(q[at], geo.lo[g], geo.inv[g], int(geo.G[g]))
                cnt[at] = self.first[g][cell, 0]
                ent[at, :15] = self.first[g][cell, 1:]
                ent[at, 15:] = self.second[g][cell, :15]
        return lv, cnt, ent


# ---- coverage classes -----------------------------------------------------------------------------------------------------------------
def tie_classes(q, palw, per, into):
    """Counts, into the dict `into`, over the queries with an exact tie for the minimum: the multiplicity, and where the two lowest
    tied rows sit under k_dither's layout of `per` rows per lane (lane = row // per, sixteen lanes to a DPP row)."""
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, q.shape[0], 4096):
            c = q[s:s + 4096]
            d0, d1, d2 = (c[:, None, a] - palw[None, :, a] for a in range(3))
            d = (d0 * d0 + d1 * d1) + d2 * d2
            d = np.where(np.isnan(d), np.inf, d)
            mn = d.min(axis=1)
            tied = (d == mn[:, None]) & np.isfinite(mn)[:, None]
            mult = tied.sum(axis=1)
            for name, sel in (("tie-2", mult == 2), ("tie-4", mult == 4), ("tie-8", mult == 8), ("tie-50+", mult >= 50)):
                into[name] = into.get(name, 0) + int(sel.sum())
            rows = np.nonzero(mult >= 2)[0]
            if rows.size == 0 or per == 0:
                continue
            first = np.argmax(tied[rows], axis=1)
            rest = tied[rows].copy()
            rest[np.arange(rows.size), first] = False
            second = np.argmax(rest, axis=1)
            l1, l2 = first // per, second // per
            same = l1 == l2
            for a in range(per):
                for b in range(a + 1, per):
                    key = "per%d-same-lane-%d%d" % (per, a, b)
                    into[key] = into.get(key, 0) + int(np.sum(same & (first % per == a) & (second % per == b)))
            into["per%d-same-row" % per] = into.get("per%d-same-row" % per, 0) + int(np.sum(~same & (l1 // 16 == l2 // 16)))
            into["per%d-other-row" % per] = into.get("per%d-other-row" % per, 0) + int(np.sum(l1 // 16 != l2 // 16))


def low_word_classes(q, palw, into):
    """... over the queries whose two smallest distances share the high 32 bits and differ in the low ones: which index is nearer"""
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, q.shape[0], 4096):
            c = q[s:s + 4096]
            d0, d1, d2 = (c[:, None, a] - palw[None, :, a] for a in range(3))
            d = (d0 * d0 + d1 * d1) + d2 * d2
            d = np.where(np.isnan(d), np.inf, d)
            if d.shape[1] < 2:
                return
            two = np.argpartition(d, 1, axis=1)[:, :2]
            da, db = d[np.arange(c.shape[0]), two[:, 0]], d[np.arange(c.shape[0]), two[:, 1]]
            ok = np.isfinite(da) & np.isfinite(db) & (da != db) & ((da.view(np.uint64) >> 32) == (db.view(np.uint64) >> 32))
            near = np.where(da < db, two[:, 0], two[:, 1])
            far = np.where(da < db, two[:, 1], two[:, 0])
            into["low-word-higher-index-nearer"] = into.get("low-word-higher-index-nearer", 0) + int(np.sum(ok & (near > far)))
            into["low-word-lower-index-nearer"] = into.get("low-word-lower-index-nearer", 0) + int(np.sum(ok & (near < far)))


def gap_classes(gap, M, into):
    """... the gap between nearest and second nearest against the query's margin M"""
    with np.errstate(invalid="ignore"):
        for name, a, b in (("gap-0-M/32", 0.0, 1.0 / 32), ("gap-M/32-M", 1.0 / 32, 1.0), ("gap-M-2M", 1.0, 2.0), ("gap-2M-8M", 2.0, 8.0)):
            into[name] = into.get(name, 0) + int(np.sum((gap > a * M) & (gap <= b * M)))


def level_classes(q, geo, into):
    lv = grid_level(q, geo)
    for name, g in (("first-grid", 0), ("second-grid", 1), ("third-grid", 2), ("outside", 3)):
        into[name] = into.get(name, 0) + int(np.sum(lv == g))
    for g in range(3):
        for side, edge in (("lo", geo.lo[g]), ("hi", geo.hi[g])):
            key = "on-%s-%d" % (side, g)
            with np.errstate(invalid="ignore"):
                into[key] = into.get(key, 0) + int(np.sum((lv == g) & np.any(q == edge, axis=1)))


def f32_names_another(q, palw, geo, want):
    """queries inside the first grid where the f32 first pass (nn_ref.f32_pass relative to the first grid's lo, over all rows) names a
    row other than `want`"""
    at = np.nonzero(grid_level(q, geo) == 0)[0]
    out = 0
    for s in range(0, at.size, 4096):
        i = at[s:s + 4096]
        t, _ = nn_ref.f32_pass(q[i], palw, geo.lo[0], geo.hi[0])
        out += int(np.sum(np.argmin(t, axis=1) != want[i]))
    return out


# ---- generators: (probes, palette) ----------------------------------------------------------------------------------------------------
def per_of(k):
    """rows per lane of k_dither's register layout (0: the generic loop)"""
    return 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 0


def _lattice_colours():
    g = np.array([-0.375, -0.125, 0.125, 0.375])
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


_PAIRS4 = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def lattice_ties(k, m, arrange="shuffled"):
    """The origin-centred lattice {+-1/8, +-3/8}^3 (64 colours) as a palette of k rows, and m probes on the multiples of 1/8 in
    [-1/2, 1/2]^3.  A probe coordinate of 0 is an exact tie between the rows mirrored in that coordinate (0 times a weight is 0, the
    float-cast weights scale +d and -d alike): 2-, 4- and 8-way, times the copies of every colour.
    "shuffled": k // 64 shuffled copies of the lattice one after another, then k % 64 more rows (k = 65: one duplicate; 3201: fifty
    copies and one).  "grouped" (k from 128): lane groups of per_of(k) rows in which a colour stands twice, at every pair of places
    within the group in turn -- the two lowest rows of every tie then share a lane."""
    rng = np.random.default_rng(1234 + k)
    base = _lattice_colours()
    if arrange == "shuffled":
        rows = [base[rng.permutation(64)] for _ in range(k // 64)]
        rows.append(base[rng.permutation(64)][:k % 64])
        pal = np.concatenate(rows)
    else:
        per = per_of(k)
        assert arrange == "grouped" and per in (2, 4)
        col = base[rng.permutation(64)]
        groups = k // per
        pal = np.empty((k, 3))
        for g in range(groups):
            if per == 2:
                pal[2 * g:2 * g + 2] = col[g % 64]
            else:
                a, b = _PAIRS4[g % 6]
                other = [p for p in range(4) if p not in (a, b)]
                pal[4 * g + a] = pal[4 * g + b] = col[g % 64]
                pal[4 * g + other[0]] = pal[4 * g + other[1]] = col[(g + groups // 2) % 64]
        pal[per * groups:] = col[:k - per * groups]
    g = np.arange(-4, 5) / 8.0
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    probes = np.concatenate([pts[rng.permutation(729)] for _ in range(m // 729 + 1)])[:m]
    return probes, np.ascontiguousarray(pal)


def dyadic_palette(k, seed=77):
    """k distinct rows whose WEIGHTED coordinates are (to a rounding) the multiples of 2^-10 in [0, 1]^3 that nn_ref.margin_sweep draws"""
    codes = np.random.default_rng(seed + k).choice(1025 ** 3, size=k, replace=False)
    grid = np.stack([codes % 1025, (codes // 1025) % 1025, codes // (1025 * 1025)], axis=1).astype(np.float64)
    return (grid / 1024.0) / FW


_GAPS = np.concatenate([[0.0], 2.0 ** -np.arange(5.0, 15.0), [1 / 16, 1 / 8, 1 / 4, 1 / 2, 3 / 4, 1.0, 1.25, 1.5, 1.75, 2.0, 3.0, 4.0, 6.0, 8.0]])
_GAPS = np.concatenate([_GAPS, -_GAPS[1:]])                                         # in units of the margin; the sign says which row is nearer


def margin(k, m, npix, outer_share=0.25):
    """margin_sweep-style probes on a dyadic palette of k rows: for a row i and its nearest row j, queries on the line through their
    midpoint along j - i whose two squared distances differ by g M, g = 0, +-2^-14 .. +-2^-5, +-1/16 .. +-8 (M: the lane layout's
    margin `amb` of this palette), each moved ACROSS the line by a random amount.  A share of the probes does the same far outside
    the first grid, on the bisector of the two rows nearest to a point 1 .. 6 box extents from the centre, with that query's own
    margin amb_p + amb_x |x - lo|^2.  Probes are queries divided by the weights."""
    rng = np.random.default_rng(500 + k)
    pal = dyadic_palette(k)
    palw = pal * FW
    geo = lane_geometry(pal, npix)
    out = []
    n_out = int(m * outer_share) if k >= 2 else 0
    n_in = m - n_out
    i = np.arange(n_in) % k
    d2 = np.sum((palw[:, None, :] - palw[None, :, :]) ** 2, axis=2) if k <= 1024 else None
    if d2 is not None:
        np.fill_diagonal(d2, np.inf)
        near = np.argmin(d2, axis=1)
    else:
        near = np.array([np.argsort(np.sum((palw - palw[r]) ** 2, axis=1))[1] for r in range(k)])
    j = near[i]
    g = _GAPS[(np.arange(n_in) // k) % _GAPS.shape[0]]
    out.append(_on_bisector(palw, i, j, 0.5 * (palw[i] + palw[j]), g, float(geo.amb), rng, None))
    if n_out:
        c, ext = 0.5 * (palw.min(axis=0) + palw.max(axis=0)), palw.max(axis=0) - palw.min(axis=0)
        u = rng.normal(size=(n_out, 3))
        u /= np.sqrt(np.sum(u * u, axis=1))[:, None]
        far = c + u * ext * rng.uniform(1.0, 6.0, size=(n_out, 1))
        two = np.argsort(((far[:, None, :] - palw[None, :, :]) ** 2).sum(axis=2), axis=1)[:, :2] if k <= 1024 else \
            np.stack([np.argsort(np.sum((palw - f) ** 2, axis=1))[:2] for f in far])
        g = _GAPS[np.arange(n_out) % _GAPS.shape[0]]
        out.append(_on_bisector(palw, two[:, 0], two[:, 1], far, g, None, rng, geo))
    return np.concatenate(out) / KW, pal


def _on_bisector(palw, i, j, start, g, M, rng, geo):
    """start moved along u = (p_j - p_i) / |..| onto the bisector of rows i and j, then to the gap g M (M None: the margin of the point
    on the bisector), then (start on the midpoint only) across the line"""
    d = palw[j] - palw[i]
    dist = np.sqrt(np.sum(d * d, axis=1))
    u = d / dist[:, None]
    t0 = (np.sum((start - palw[j]) ** 2, axis=1) - np.sum((start - palw[i]) ** 2, axis=1)) / (2.0 * dist)
    x = start + t0[:, None] * u                                                   # d_j^2 - d_i^2 = 0 here (to rounding)
    if M is None:
        M = query_margin(x, geo)
    else:
        v = np.cross(u, [0.0, 0.0, 1.0])
        bad = np.sum(v * v, axis=1) < 1e-6
        v[bad] = np.cross(u[bad], [1.0, 0.0, 0.0])
        v /= np.sqrt(np.sum(v * v, axis=1))[:, None]
        x = x + (rng.uniform(-0.02, 0.02, size=x.shape[0]) * dist)[:, None] * v
    return x - (g * M / (2.0 * dist))[:, None] * u                                # g > 0: row i nearer by g M


def _straddle(face, w):
    """the two neighbouring pixel values (below, at-or-above) whose products with the weight w straddle `face`"""
    p = face / w
    for _ in range(4):
        p = np.where(w * p < face, np.nextafter(p, np.inf), p)
    for _ in range(4):
        below = np.nextafter(p, -np.inf)
        p = np.where(w * below >= face, below, p)
    return np.nextafter(p, -np.inf), p


def faces(k, npix, corner_copies=70, seed=31):
    """For each of the lane layout's three grids and each axis: every cell boundary lo + i / inv, i = 0 .. G (the two pixel values
    whose queries straddle it, and the next one on either side), and the boundary moved by +-1e-9 .. 5e-6 of the extent; the other two
    coordinates random in that grid.  Then `corner_copies` probes on each grid's lo and hi per axis -- exactly on them wherever a
    pixel value has that product.  Palette: k random rows of a random box."""
    rng = np.random.default_rng(seed + k)
    lo, hi = nn_ref.random_box()
    pal = nn_ref.box_palette(k, lo, hi) / FW
    geo = lane_geometry(pal, npix)
    out = []
    for g in range(3):
        G = int(geo.G[g])
        ext = geo.hi[g] - geo.lo[g]
        for a in range(3):
            i = np.arange(G + 1, dtype=np.float64)
            f = geo.lo[g][a] + i / geo.inv[g][a]
            f[0], f[-1] = geo.lo[g][a], geo.hi[g][a]
            below, at = _straddle(f, KW[a])
            xs = [below, at, np.nextafter(below, -np.inf), np.nextafter(at, np.inf)]
            for delta in (1e-9, 1e-7, 1e-6, 3e-6, 5e-6):
                xs += [(f - delta * ext[a]) / KW[a], (f + delta * ext[a]) / KW[a]]
            below, at = _straddle(np.repeat(np.array([geo.lo[g][a], geo.hi[g][a]]), corner_copies), KW[a])
            xs.append(at)
            xs = np.concatenate(xs)
            p = (geo.lo[g] + ext * rng.random((xs.shape[0], 3))) / KW
            p[:, a] = xs
            out.append(p)
    probes = np.concatenate(out)
    return probes[rng.permutation(probes.shape[0])], pal


CLUSTERS = ((40, 1e-4), (31, 2e-2), (16, 1e-4), (20, 2e-2), (30, 1e-4), (31, 1e-4), (40, 2e-2), (16, 2e-2), (30, 2e-2), (20, 1e-4))


def crowded(k, m, seed=900):
    """Clusters of 16, 20, 30, 31 and 40 rows (CLUSTERS in turn, each that still fits into k; below 16 rows the whole palette is one
    cluster) on spheres of radius 1e-4 and 2e-2 of the weighted space -- below a cell of the 32^3 grid over the unit box (1/16), and on
    either side of the margin (about 2e-5 there; the gaps between a cluster's rows go with the square of the radius): a probe at
    the centre of a small sphere sees the whole cluster within the margin, a probe half a radius towards a row of a large one is clear.
    Clusters of more than thirty rows take their rows from the four strides of 64 of the index range in turn, so that every quarter of
    the whole-wavefront scan holds winners.  The rest of the palette is random rows.  Probes: each cluster's centre, and from it
    towards each of its rows by 0.5 and 0.9 radii; repeated with a jitter of 1e-6 until there are m."""
    rng = np.random.default_rng(seed + k)
    palw = rng.random((k, 3))
    plan, left = [], k
    for size, rad in (CLUSTERS if k >= 16 else ((k, 1e-4),)):
        if size <= left:
            plan.append((size, rad))
            left -= size
    free = np.ones(k, dtype=bool)
    g = np.array([0.2, 0.5, 0.8])
    centres = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(27)] + rng.uniform(-0.03, 0.03, size=(27, 3))
    probes = []
    for ci, (size, rad) in enumerate(plan):
        rows = []
        for t in range(size):
            if size > 30 and k >= 200:
                q = t % 4
                cand = np.nonzero(free[64 * q:64 * q + 64])[0]
                j = 64 * q + int(cand[0]) if cand.size else int(np.nonzero(free)[0][0])
            else:
                j = int(np.nonzero(free)[0][0])
            free[j] = False
            rows.append(j)
        u = rng.normal(size=(size, 3))
        u /= np.sqrt(np.sum(u * u, axis=1))[:, None]
        palw[np.array(rows)] = centres[ci] + rad * u
        probes.append(centres[ci][None, :])
        for s in (0.5, 0.9):
            probes.append(centres[ci] + s * rad * u)
    probes = np.concatenate(probes)
    reps = m // probes.shape[0] + 1
    jit = np.concatenate([np.zeros(probes.shape)] + [rng.normal(size=probes.shape) * 1e-6 for _ in range(reps - 1)])
    return (np.concatenate([probes] * reps) + jit)[:m] / KW, palw / FW


def tiny_box(k, m, size, seed=1300):
    """k rows inside a box of edge `size` (weighted space) at the middle of [0, 1]^3, probes all over [0, 1]^3 in pixel space: most
    queries fall in the second or third grid or outside all three"""
    rng = np.random.default_rng(seed + k)
    palw = 0.35 + size * rng.random((k, 3))
    return rng.random((m, 3)), palw / FW


def degenerate(k, m, flat_axes, seed=1700):
    """palette extent zero on `flat_axes` axes (3: k copies of one colour -- r = 0, every grid a cube of its fixed margin); probes within
    a few extents (a few margins) of it, a fifth of them with the flat coordinates exactly the palette's"""
    rng = np.random.default_rng(seed + k + flat_axes)
    pal = 0.2 + 0.5 * rng.random((k, 3))
    pal[:, :flat_axes] = pal[0, :flat_axes]
    probes = pal[rng.integers(0, k, size=m)] + rng.normal(size=(m, 3)) * np.where(np.arange(3) < flat_axes, 0.01, 0.5)
    same = rng.random(m) < 0.2
    probes[same, :flat_axes] = pal[0, :flat_axes]
    return probes, pal


def mixed(k, m, npix, seed=2100):
    """crowded(k)'s palette under four kinds of probe shuffled along the curve, so that the lanes of one step of k_dither_lanes (64
    consecutive runs) differ in class: crowded's own, margin-style near-ties of that palette, points all over the box +- 1 extent,
    and points 2 .. 9 extents out (the third grid, and outside all three), half of them near-ties of their two nearest rows"""
    rng = np.random.default_rng(seed + k)
    a, pal = crowded(k, m // 2)
    palw = pal * FW
    geo = lane_geometry(pal, npix)
    d2 = np.sum((palw[:, None, :] - palw[None, :, :]) ** 2, axis=2)
    np.fill_diagonal(d2, np.inf)
    nb = m // 8
    i = rng.integers(0, k, size=nb)
    j = np.argmin(d2, axis=1)[i]
    b = _on_bisector(palw, i, j, 0.5 * (palw[i] + palw[j]), _GAPS[np.arange(nb) % _GAPS.shape[0]], float(geo.amb), rng, None) / KW
    c = rng.uniform(-1.0, 2.0, size=(m // 8, 3)) / KW
    u = rng.normal(size=(m - a.shape[0] - nb - c.shape[0], 3))
    u /= np.sqrt(np.sum(u * u, axis=1))[:, None]
    far = 0.5 + u * rng.uniform(2.0, 9.0, size=(u.shape[0], 1))
    half = far.shape[0] // 2                                                        # ... half of them moved onto the bisector of their two nearest rows
    two = np.argsort(((far[:half, None, :] - palw[None, :, :]) ** 2).sum(axis=2), axis=1)[:, :2]
    far[:half] = _on_bisector(palw, two[:, 0], two[:, 1], far[:half], _GAPS[np.arange(half) % _GAPS.shape[0]], None, rng, geo)
    probes = np.concatenate([a, b, c, far / KW])
    return probes[rng.permutation(probes.shape[0])], pal


NONFINITE = (("nan", 1, np.nan), ("plus-inf", 0, np.inf), ("minus-inf", 2, -np.inf), ("1e200", 0, 1e200), ("1e39", 1, 1e39),
             ("1e308-pair", 0, 1e308))                                   # two finite pixels in a row whose errors SUM to +Inf


def with_nonfinite(lay, order, variant, places):
    """a copy of the layout's image with one plane of the pixels at the curve ranks `places` (a "-pair": and at the ranks behind them)
    set to the variant's value"""
    name, plane, value = [v for v in NONFINITE if v[0] == variant][0]
    n = order.shape[0]
    image = lay.image.copy()
    places = np.asarray(places, dtype=np.int64)
    if name.endswith("-pair"):
        places = np.concatenate([places, places + 1])
    image[plane * n + order[places]] = value
    return image


def nonfinite_places(lay, locate, runs=16):
    """Curve ranks for a pixel that is not finite, with the image cut into `runs` runs (patolette_amd_dither_config(runs)): a probe
    slot; mid-reset; within the last sixteen pixels of a run and inside the next run's warm-up -- for the lane layout, whose run b
    starts at rank n b / runs, and for the wavefront layout, whose run b starts at the aligned 64-position block that holds that rank:
    locate(t) -> the in-image pixels before that block (patolette_amd_debug_dither_locate's c)."""
    n = lay.seq.shape[0]
    return np.array([lay.ranks[40], lay.ranks[400] + 7, n * 5 // runs - 5, n * 9 // runs - 100,
                     locate(n * 7 // runs) - 5, locate(n * 11 // runs) - 40])


# ---- the named cases of both test files -----------------------------------------------------------------------------------------------
WAVE_K = (5, 64, 65, 128, 129, 256, 257, 700, 3200, 3201)                              # every threshold of k_dither's layouts, either side
LANE_K = (8, 9, 64, 255, 256)
TINY_SIZE = {8: 1e-3, 9: 1e-2, 64: 0.1, 255: 1e-3, 256: 1e-2}
BIG = ("ties", "margin", "faces", "crowded", "tiny", "flat")                           # 1024 x 1024: the lane layout's 64^3 grids


def wave_cases():
    out = []
    for k in WAVE_K:
        out.append("ties-%d-shuffled" % k)
        if per_of(k) in (2, 4):
            out.append("ties-%d-grouped" % k)
        out.append("margin-%d" % k)
    return out


def lane_cases():
    out = []
    for k in LANE_K:
        out += ["ties-%d-shuffled" % k, "margin-%d" % k, "faces-%d" % k, "crowded-%d" % k, "tiny-%d" % k]
        out += ["flat-%d-%d" % (k, a) for a in (1, 2, 3)]
    out += ["ties-256-grouped", "ties-128-grouped", "mixed-256"]
    return out


def big_cases():
    return ["big-" + f for f in BIG]


def case_size(name):
    f = name.split("-")[0]
    return (1024, 1024) if f == "big" else (300, 230) if f in ("margin", "tiny") else (512, 300) if f == "faces" else (256, 256)


def make(name, order):
    """the Layout of a named case; order: the curve order of case_size(name) (oracle.binding.hilbert_order)"""
    w, h = case_size(name)
    n = w * h
    part = name.split("-")
    big = part[0] == "big"
    fam, k = (part[1], 256) if big else (part[0], int(part[1]))
    ranks = sparse_ranks(n) if big else default_ranks(n)
    m = ranks.shape[0]
    if fam == "ties":
        probes, pal = lattice_ties(k, m, "grouped" if big else part[2])
    elif fam == "margin":
        probes, pal = margin(k, m if k <= 256 else 1200, n)                         # (the anchor search is brute force over k rows)
    elif fam == "mixed":
        probes, pal = mixed(k, m, n)
    elif fam == "faces":
        probes, pal = faces(k, n)
    elif fam == "crowded":
        probes, pal = crowded(k, m)
    elif fam == "tiny":
        probes, pal = tiny_box(k, m, TINY_SIZE[k])
    else:
        assert fam == "flat"
        probes, pal = degenerate(k, m, 1 if big else int(part[2]))
    assert probes.shape[0] <= m or fam == "faces", (name, probes.shape[0], m)
    return layout(probes[:m], pal, order, w, h, ranks=ranks[:probes.shape[0]])


class Evaluated:
    """a case with the oracle's map (`want`, pixel order; `chain`, curve order) and, worked out when first asked for, the replayed
    chain: the query q, brute index idx, gap and ties of every step.  Made once per session (`evaluated`)."""

    def _replayed(self):
        if not hasattr(self, "_rep"):
            self._rep = replay(self.lay.seq, self.lay.pal, self.chain)
        return self._rep

    q = property(lambda self: self._replayed()[0])
    idx = property(lambda self: self._replayed()[1])
    gap = property(lambda self: self._replayed()[2])
    ties = property(lambda self: self._replayed()[3])


_orders, _evaluated = {}, {}


def curve_order(ob, width, height):
    if (width, height) not in _orders:
        _orders[(width, height)] = ob.hilbert_order(width, height).astype(np.int64)
    return _orders[(width, height)]


def evaluated(ob, name):
    if name not in _evaluated:
        w, h = case_size(name)
        order = curve_order(ob, w, h)
        ev = Evaluated()
        ev.name, ev.order = name, order
        ev.lay = make(name, order)
        ev.want = ob.dither(ev.lay.image, w, h, ev.lay.pal).astype(np.int64)
        ev.chain = ev.want[order]
        ev.probe = np.zeros(order.shape[0], dtype=bool)
        ev.probe[ev.lay.ranks] = True
        _evaluated[name] = ev
    return _evaluated[name]
