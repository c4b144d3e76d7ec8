"""An independent model of the KMeans stage (numpy; no GPU, no oracle): what refine.c and the patched faiss Clustering.cpp compute
in one call, without subsampling (callers keep n <= k * (max(max_samples, 65536) // k)), and the deterministic generators of
tests/test_km_reference.py and tests/test_gpu_kmeans_edges.py.

Every f32 operation is rounded once: sums and products of two f32 values by numpy's own f32 arithmetic, a fused multiply-add by
an exact product in f64, TwoSum, round-to-odd and one cast (53 >= 2 * 24 + 2 bits: the cast then rounds as if from the exact value).

The two places where the product departs from the reference because the reference does not return (include/patolette_amd.h,
patolette_amd_kmeans_refine) are modelled as the header states them: no donor with a size above 1 -> the remaining empty clusters
stay (0, 0); the finite domain is the caller's business (in_domain)."""
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = f32(3.402823466e+38)


# ------------------------------------------------------------------------------------------------ arithmetic
def fma32(a, b, c):
    """round_f32(a * b + c), one rounding; a, b, c f32 arrays (or scalars)."""
    a, b, c = np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32)
    with np.errstate(all="ignore"):
        p = a.astype(f64) * b.astype(f64)                       # exact: 48 bits
        c64 = c.astype(f64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                       # TwoSum: p + c64 = s + err exactly
        odd = (np.atleast_1d(s).view(np.int64) & 1).reshape(np.shape(s)) != 0
        fix = (err != 0) & ~odd & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def norm3(v0, v1, v2):
    """|v|^2 = fma(v2, v2, fma(v0, v0, v1 * v1))"""
    return fma32(v2, v2, fma32(v0, v0, np.asarray(v1, f32) * np.asarray(v1, f32)))


class MT19937:
    """std::mt19937: raw 32-bit outputs; `refills` counts generated blocks of 624 words."""

    def __init__(self, seed):
        mt = np.zeros(624, np.uint64)
        mt[0] = seed
        for i in range(1, 624):
            mt[i] = (1812433253 * (int(mt[i - 1]) ^ (int(mt[i - 1]) >> 30)) + i) & 0xFFFFFFFF
        self.mt = mt.astype(np.uint32)
        self.out = np.zeros(0, np.uint32)
        self.pos = 0
        self.refills = 0

    def _twist(self):
        mt = self.mt.copy()

        def tw(cur, nxt, far):
            y = (cur & np.uint32(0x80000000)) | (nxt & np.uint32(0x7fffffff))
            return far ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908b0df), np.uint32(0))
        mt[0:227] = tw(mt[0:227], mt[1:228], mt[397:624])
        mt[227:454] = tw(mt[227:454], mt[228:455], mt[0:227])
        mt[454:623] = tw(mt[454:623], mt[455:624], mt[227:396])
        mt[623:624] = tw(mt[623:624], mt[0:1], mt[396:397])
        self.mt = mt
        y = mt.copy()
        y ^= y >> np.uint32(11)
        y ^= (y << np.uint32(7)) & np.uint32(0x9d2c5680)
        y ^= (y << np.uint32(15)) & np.uint32(0xefc60000)
        y ^= y >> np.uint32(18)
        self.refills += 1
        return y

    def take(self, m):
        """the next m outputs WITHOUT consuming them"""
        while self.out.size - self.pos < m:
            self.out = np.concatenate([self.out[self.pos:], self._twist()])
            self.pos = 0
        return self.out[self.pos:self.pos + m]

    def consume(self, m):
        self.pos += m


# ------------------------------------------------------------------------------------------------ one iteration
def assign(x, cent, stats=False):
    """Nearest centre of every sample, exhaustive_L2sqr_fused_cmax<3,6,1> (simdlib_based.cpp:59-277) as km_assign_one writes it.
    x (n,3) f32, cent (k,3) f32 -> int64 (n,); 0xFFFFFFFF where nothing was accepted.  stats: also the per-centre clamped
    distances' winners: (assign, nwin, nneg) -- centres sharing the winning clamped distance, centres negative before the clamp."""
    n, k = x.shape[0], cent.shape[0]
    x0, x1, x2 = x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy()
    yw = norm3(cent[:, 0], cent[:, 1], cent[:, 2])
    with np.errstate(all="ignore"):
        m0, m1, m2 = f32(-2) * x0, f32(-2) * x1, f32(-2) * x2
        xn = norm3(x0, x1, x2)
        ld = np.tile(FLT_MAX - xn, (8, 1))
        li = np.zeros((8, n), np.int64)
        nyp = (k // 8) * 8
        dall = np.empty((k, n), f32) if stats else None
        ncl = np.zeros(n, np.int64)
        for j in range(nyp):
            dp = m0 * cent[j, 0]
            dp = fma32(m1, cent[j, 1], dp)
            dp = fma32(m2, cent[j, 2], dp)
            dp = dp + yw[j]
            l = j & 7
            better = dp < ld[l]
            ld[l] = np.where(better, dp, ld[l])
            li[l] = np.where(better, j, li[l])
            if stats:
                d = dp + xn
                ncl += d < 0
                dall[j] = np.where(d < 0, f32(0), d)
        cur_d = np.full(n, FLT_MAX, f32)
        cur_i = np.full(n, 0xFFFFFFFF, np.int64)
        for l in range(8):
            cand = ld[l] + xn
            cand = np.where(cand < 0, f32(0), cand)
            take = (cur_d > cand) | ((cur_d == cand) & (cur_i > li[l]))
            cur_i = np.where(take, li[l], cur_i)
            cur_d = np.where(cur_d > cand, cand, cur_d)
        for j in range(nyp, k):
            dp = fma32(x2, cent[j, 2], fma32(x1, cent[j, 1], x0 * cent[j, 0]))
            d = (xn + yw[j]) - f32(2) * dp
            if stats:
                ncl += d < 0
            d = np.where(d < 0, f32(0), d)
            if stats:
                dall[j] = d
            take = cur_d > d
            cur_d = np.where(take, d, cur_d)
            cur_i = np.where(take, j, cur_i)
    if stats:
        return cur_i, (dall == dall.min(axis=0)[None, :]).sum(axis=0), ncl
    return cur_i


def _groups(a, k):
    order = np.argsort(a, kind="stable")
    cnt = np.bincount(a, minlength=k)
    return order, cnt, np.concatenate([[0], np.cumsum(cnt)])


def update(x, w, a, k, trace_of=None):
    """compute_centroids (Clustering.cpp:135-204): per centroid and component ONE sequential f32 chain over its members in sample
    order: acc += x, or acc = fma(x, w, acc) and h += w.  -> cent (k,3) f32, h (k,) f32 [, trace (members, 4) of centroid trace_of:
    the accumulators after every member (x, y, z, h)]"""
    order, cnt, start = _groups(a, k)
    acc = np.zeros((k, 3), f32)
    h = np.zeros(k, f32)
    trace = None
    if w is None:
        for j in range(k):
            m = order[start[j]:start[j + 1]]
            if m.size:
                cs = np.add.accumulate(x[m], axis=0, dtype=f32)              # sequential, f32 at every step
                acc[j] = cs[-1]
                if trace_of == j:
                    trace = np.concatenate([cs, np.minimum(np.arange(1, m.size + 1), 1 << 24).astype(f32)[:, None]], axis=1)
        h = np.minimum(cnt, 1 << 24).astype(f32)                            # h += 1.0f sticks at 2^24
    else:
        by = np.argsort(-cnt, kind="stable")                                 # longest clusters first: step r works on a prefix
        cs = cnt[by]
        A = np.zeros((k, 3), f32)
        H = np.zeros(k, f32)
        if trace_of is not None:
            trace = np.zeros((cnt[trace_of], 4), f32)
            tpos = int(np.nonzero(by == trace_of)[0][0])
        for r in range(int(cs[0]) if k else 0):
            live = int(np.searchsorted(-cs, -r, side="left"))                # clusters with more than r members
            m = order[start[by[:live]] + r]
            wm = w[m]
            H[:live] = H[:live] + wm
            A[:live] = fma32(x[m], wm[:, None], A[:live])
            if trace_of is not None and tpos < live:
                trace[r, :3] = A[tpos]
                trace[r, 3] = H[tpos]
        acc[by] = A
        h[by] = H
    cent = acc.copy()
    with np.errstate(all="ignore"):
        nz = h != 0
        norm = f32(1) / h[nz]
        cent[nz] = acc[nz] * norm[:, None]
    if trace_of is not None:
        return cent, h, trace
    return cent, h


def split_clusters(cent, h, n, counters=None):
    """Clustering.cpp:216-263 with std::mt19937(1234) restarted at every call; in place.  The product's termination rule: once no
    cluster has a size above 1 (or n <= k) the remaining empty clusters stay as they are."""
    k = h.shape[0]
    rng = MT19937(1234)
    denom = f64(f32(n - k)) if n > k else f64(0)
    nsplit = 0
    for ci in range(k):
        if h[ci] != 0:
            continue
        if not (n > k) or not np.any(h > f32(1)):
            break
        with np.errstate(all="ignore"):
            p = ((h.astype(f64) - 1.0) / denom).astype(f32)
        cj0 = 0
        while True:
            y = rng.take(k)
            r = y.astype(f32) / f32(4294967296.0)
            hit = r < np.roll(p, -cj0)
            if hit.any():
                t = int(np.argmax(hit))
                rng.consume(t + 1)
                cj = (cj0 + t) % k
                break
            rng.consume(k)                                               # k draws later the walk is at cj0 again
        up, dn = f64(1 + 1 / 1024.), f64(1 - 1 / 1024.)
        src = cent[cj].astype(f64)
        cent[ci] = (src * np.array([up, dn, up])).astype(f32)
        cent[cj] = (src * np.array([dn, up, dn])).astype(f32)
        h[ci] = h[cj] / f32(2)
        h[cj] = h[cj] - h[ci]
        nsplit += 1
    if counters is not None:
        counters["splits"] = counters.get("splits", 0) + nsplit
        counters["refills"] = max(counters.get("refills", 0), rng.refills)
    return nsplit


def km_fix(bound_x, bound_w, weighted, nx):
    """KmFix as kmeans_iterate derives it: (quantum_x, quantum_w) as exponents of two"""
    ex = int(np.frexp(max(bound_x, 1e-300) * (max(bound_w, 1e-300) if weighted else 1.0))[1])
    ew = int(np.frexp(max(bound_w, 1e-300))[1])
    P = 1
    while (1 << P) < nx:
        P += 1
    P = max(P + 1, 12)
    return ex + P - 62, ew + P - 62


def update_sums(x, w, a, k, qx, qw):
    """the order-free update: integer sums of rint(v / quantum), f32(sum * quantum) * (1 / h)"""
    xd = x.astype(f64) * (w.astype(f64)[:, None] if w is not None else 1.0)
    q = np.rint(np.ldexp(xd, -qx)).astype(np.int64)
    sums = np.zeros((k, 3), np.int64)
    np.add.at(sums, a, q)
    if w is not None:
        hw = np.zeros(k, np.int64)
        np.add.at(hw, a, np.rint(np.ldexp(w.astype(f64), -qw)).astype(np.int64))
        h = np.array([np.ldexp(float(int(v)), qw) for v in hw], f64).astype(f32)
    else:
        h = np.bincount(a, minlength=k).astype(f64).astype(f32)
    cent = np.array([[np.ldexp(float(int(v)), qx) for v in row] for row in sums], f64).reshape(k, 3).astype(f32)
    with np.errstate(all="ignore"):
        nz = h != 0
        cent[nz] = cent[nz] * (f32(1) / h[nz])[:, None]
    return cent, h


def refine(colors, weights, centers, niter, order_free=False, counters=None):
    """patolette_amd_kmeans_refine without subsampling.  colors (n,3) f64, weights (n,) f64 or None, centers (k,3) f64 -> (k,3) f32"""
    x = np.ascontiguousarray(colors, f64).astype(f32)
    w = None if weights is None else np.asarray(weights, f64).astype(f32)
    cent = np.asarray(centers, f64).astype(f32)
    n, k = x.shape[0], cent.shape[0]
    if n < k:
        return cent
    if n == k:
        return x.copy()
    if order_free:
        bx = float(np.max(np.abs(colors)))
        bw = max(1.0, float(np.max(np.abs(weights)))) if weights is not None else 1.0
        qx, qw = km_fix(bx, bw, w is not None, n)
    for _ in range(niter):
        a = assign(x, cent)
        cent, h = update_sums(x, w, a, k, qx, qw) if order_free else update(x, w, a, k)
        split_clusters(cent, h, n, counters)
    return cent


def in_domain(colors, weights, centers):
    """the finite domain of patolette_amd_kmeans_refine (include/patolette_amd.h), for n samples used"""
    x = np.asarray(colors, f64).astype(f32).astype(f64)
    c = np.asarray(centers, f64).astype(f32).astype(f64)
    if not (np.isfinite(x).all() and np.isfinite(c).all()):
        return False
    B = max(1.0, float(np.abs(x).max()), float(np.abs(c).max()))
    m = float(min(x.shape[0], 1 << 25))
    wmax, Cb = 1.0, 8.0 * B
    if weights is not None:
        w = np.asarray(weights, f64).astype(f32).astype(f64)
        if not (np.isfinite(w).all() and (w >= 0).all()):
            return False
        wmax = max(1.0, float(w.max()))
        pos = w[w > 0]
        if pos.size and pos.min() < 2.0 ** -126:
            return False
        by_n = float(np.exp(min(x.shape[0] * 2.0 ** -23, 700.0))) * B
        Cb = 4.0 * (min(by_n, 4.0 * m * (wmax / pos.min()) * B) if pos.size else by_n)
    Cb += 8.0
    return 16.0 * Cb * Cb <= float(FLT_MAX) and 4.0 * m * wmax * B <= float(FLT_MAX)


# ------------------------------------------------------------------------------------------------ block classifier
OUTCOMES = ("whole", "quarters", "tie", "upper", "lower", "range")


def _block_exact(acc, add, margins=None):
    """km_block_exact on the exact addends `add` (f64: x, or the exact product x * w): None if it holds, else why it does not.
    margins: a list that gets (units left below the upper bound, units left above the lower bound) of every tie-free evaluation"""
    aa = abs(float(acc))
    if not (aa >= float(f32(1e-30)) and aa < float(f32(1e30))):
        return "range"
    ex = int(np.frexp(aa)[1])
    scale = np.ldexp(-1.0 if acc < 0 else 1.0, 24 - ex)
    M0 = aa * abs(scale)
    t = add * scale
    r = np.rint(t)
    tot, mag = float(r.sum()), float(np.abs(r).sum())               # integers far below 2^53: exact in any order
    if np.any(np.abs(t - r) >= 0.5):
        return "tie"
    if margins is not None:
        margins.append((16777215.0 - (M0 + 0.5 * (tot + mag)), (M0 + 0.5 * (tot - mag)) - 8388609.0))
    if not (M0 + 0.5 * (tot - mag) >= 8388609.0):
        return "lower"
    if not (M0 + 0.5 * (tot + mag) <= 16777215.0):
        return "upper"
    return None


def classify_blocks(add, trace, margins=None):
    """km_block_step over one chain: add (m,) the exact addends in member order, trace (m,) the f32 accumulator after each member.
    -> {outcome: count}: blocks that pass whole, blocks that fail whole and are taken by quarters, and the quarters (or short last
    blocks) replayed in order, by the first condition that fails."""
    out = dict.fromkeys(OUTCOMES, 0)
    m = add.shape[0]
    for b0 in range(0, m, 1024):
        ln = min(1024, m - b0)
        acc = f32(0) if b0 == 0 else trace[b0 - 1]
        why = _block_exact(acc, add[b0:b0 + ln], margins)
        if why is None:
            out["whole"] += 1
        elif ln == 1024:
            out["quarters"] += 1
            for q in range(4):
                a0 = b0 + 256 * q
                why = _block_exact(f32(0) if a0 == 0 else trace[a0 - 1], add[a0:a0 + 256], margins)
                if why is not None:
                    out[why] += 1
        else:
            out[why] += 1
    return out


# ------------------------------------------------------------------------------------------------ generators
STAIR_COUNTS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 511, 512, 513, 575, 0, 576, 577, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193,
                12289, 0]                                                 # empty clusters first, in the middle and last


def _lattice_centres(k, spacing=8.0):
    """k distinct points of a cubic lattice with the given spacing, around 24 per axis"""
    side = int(np.ceil(k ** (1.0 / 3.0)))
    j = np.arange(k)
    return np.stack([j % side, (j // side) % side, j // (side * side)], axis=1).astype(f64) * spacing + 16.0


def _offsets(m, salt):
    """m offsets in (-1/4, 1/4)^3 on the 2^-20 lattice (centre + offset exact in f32 near 2^5 .. 2^8: 2^-16 .. 2^-19 is the ulp,
    so the sum is rounded by the f32 cast of the sample -- what matters is that consecutive members differ in their low bits, and
    running sums of a few of them round differently in another order)."""
    i = np.arange(m, dtype=np.int64)[:, None] * np.array([2654435761, 40503, 2246822519], dtype=np.int64)[None, :] + salt * 977
    v = ((i >> 3) % (1 << 19)).astype(f64) - (1 << 18) + 0.5
    return v * 2.0 ** -20


def staircase(counts, layout, weighted, k_pad=0):
    """Clusters with prescribed member counts: counts[j] members around lattice centre j (spacing 8, offsets in (-1/4, 1/4)), so
    the first assignment is known by construction; k_pad further centres get one member each.
    layout: "shuffled" (a fixed permutation), "runs" (each centroid's members contiguous), "striped" (round robin over the
    centroids that still have members left: never two members of a centroid adjacent.  A 64-sample step holds at most one member
    of a centroid only while 64 or more centroids are left -- with STAIR_COUNTS (25 non-empty clusters) it holds 2 to 3 of each;
    striped_even is the case with at most one).
    -> colors (n,3) f64, weights (n,) or None, centers (k,3) f64"""
    counts = list(counts) + [1] * k_pad
    k = len(counts)
    cent = _lattice_centres(k)
    owner = np.repeat(np.arange(k), counts)
    n = owner.shape[0]
    rank = np.concatenate([np.arange(c) for c in counts]) if n else np.zeros(0, np.int64)
    off = _offsets(n, 1)
    pts = (cent[owner] + off).astype(f32).astype(f64)
    if layout == "runs":
        perm = np.arange(n)
    elif layout == "striped":
        perm = np.lexsort((owner, rank))                               # rank-major: member r of every centroid, then r + 1
    elif layout == "shuffled":
        perm = np.argsort(((np.arange(n, dtype=np.int64) * 2654435761) >> 7) % 1000003, kind="stable")
    else:
        raise ValueError(layout)
    pts = pts[perm]
    w = None
    if weighted:
        w = (((np.arange(n, dtype=np.int64) * 40503) % 4093) + 3).astype(f64) * 2.0 ** -12      # 12-bit weights in (0, 1)
    return pts, w, cent



def counts_case(nx, k=24, weighted=False):
    """an order-sensitive staircase of k clusters and nx samples: uneven counts (proportional to j^2), shuffled"""
    wgt = np.arange(1, k + 1, dtype=f64) ** 2
    counts = np.floor(wgt / wgt.sum() * nx).astype(np.int64)
    counts[-1] += nx - counts.sum()
    return staircase([int(c) for c in counts], "shuffled", weighted)


def end255():
    """262 145 samples in runs: the last cluster's 4096th member is sample 262 143, the last record of block 255 of 1024 samples,
    its 4097th is alone in block 256"""
    return staircase([262145 - 4097 - 22 * 1000, *([1000] * 22), 4097], "runs", False)


def striped_even(weighted, k=200, each=40):
    """k > 64 clusters of equal size, striped: every window of 64 consecutive samples holds at most ONE member of a centroid"""
    return staircase([each] * k, "striped", weighted)


PLAN_BLOCKS = 13


def _planned_blocks():
    """The exact addends (f64) of 13 blocks of 1024 members of ONE sign each, planned so that whole blocks of km_block_exact end one
    unit inside, on and one unit beyond each bound.  u = 2^-20 is the accumulator's unit in [8, 16), 2u its unit in [16, 32); every
    partial sum is a multiple of the unit of its binade, so the f32 chain is exact and the plan is what the kernel sees:
      0 -> 8 + 8u | -> 16 - 2u (upper bound: 1 unit left) | -4 | -> 16 - u (0 left) | -4 | -> 16 (1 beyond: fails, its last quarter
      too) | +4 | -> 16 + 4u (lower bound, units of 2u: 1 left) | +4 | -> 16 + 2u (0 left) | +4 | -> 16 (1 beyond) | -16 -> 0"""
    u = 2.0 ** -20
    U = 1 << 20
    ends = [8 * U + 8, 16 * U - 2, 12 * U - 2, 16 * U - 1, 12 * U - 1, 16 * U, 20 * U, 16 * U + 4, 20 * U + 4, 16 * U + 2, 20 * U + 2, 16 * U, 0]
    out, at = [], 0
    for e in ends:
        total = e - at
        step = 2 if at >= 16 * U and e >= 16 * U else 1                      # in [16, 32) only even multiples of u
        q, r = divmod(abs(total) // step, 1024)
        blk = (np.full(1024, q, dtype=np.int64) + (np.arange(1024) < r)) * step
        out.append(np.sign(total) * blk.astype(f64) * u)
        at = e
    return np.concatenate(out)


def binade_walk(weighted, m=20000 + 1024 * PLAN_BLOCKS):
    """One cluster at the origin with m members of mixed sign, the other centres far away: the running sums cross zero, walk up and
    down over several binades (subnormal magnitudes included), meet addends that are odd multiples of half an ulp of the
    accumulator (exact ties) and -- the first 13 blocks of the y chain, _planned_blocks -- whole blocks whose integer totals end
    one unit inside, on and one unit beyond both bounds of km_block_exact, weighted (products of weights 1/2 and 1) and not.
    -> colors, weights, centers (k = 8)"""
    i = np.arange(m, dtype=np.int64)
    v = np.zeros((m, 3), f64)
    # x: long stretches of one sign with slowly changing magnitude -> whole blocks and quarters inside one binade, binade
    # crossings every few thousand members, zero crossings between stretches
    seg = i // 2500
    sign = np.where(seg % 2 == 0, 1.0, -1.0)
    mant = 1.0 + ((i * 2654435761) % (1 << 23)).astype(f64) * 2.0 ** -23
    v[:, 0] = sign * mant * np.ldexp(1.0, (-(seg % 4)).astype(np.int64) - 3)
    # y, after the planned blocks (the chain is back at 0 there; iy counts from their end): constant addends 2^-12 and stretches of
    # exact ties: the accumulator reaches 2^-12 * r, and from r = 2^12 on an addend of 2^-12 is below its ulp's half .. at r in
    # [2^11, 2^12) addends of 2^-36 * odd are half-ulp ties against even and odd sums
    off = 1024 * PLAN_BLOCKS
    iy = i - off
    v[:, 1] = 2.0 ** -12
    tie = (iy >= 2048) & (iy < 4096)
    v[tie, 1] = np.where(iy[tie] % 2 == 0, 2.0 ** -12 + 2.0 ** -25, 2.0 ** -25)    # half an ulp of [1/2, 1): ulp = 2^-24
    v[iy >= 12000, 1] = -(2.0 ** -11)                                          # back down through the binades and across zero
    # z: subnormal and tiny magnitudes, then a block that ends within one unit of the upper bound
    v[:, 2] = np.where(i < 4096, 2.0 ** -140 * (1 + (i % 7)), np.where(i < 8192, 2.0 ** -100, 2.0 ** -110 * np.where(i % 2 == 0, 3.0, -1.0)))
    w = None
    if weighted:
        w = (1.0 + ((i * 40503) % (1 << 23)).astype(f64) * 2.0 ** -23) * 0.5       # 24-bit weights in [1/2, 1): 24 x 24-bit products
        w[:off] = np.where(i[:off] % 2 == 0, 0.5, 1.0)                             # the planned blocks: products exact by design
    v[:off, 1] = _planned_blocks() / (w[:off] if weighted else 1.0)
    far = np.array([[64, 0, 0], [0, 64, 0], [0, 0, 64], [-64, 0, 0], [0, -64, 0], [0, 0, -64], [64, 64, 64]], f64)
    pts = np.concatenate([v, np.repeat(far, 3, axis=0) + _offsets(21, 5) * 4])
    # the far members interleaved so that the origin cluster's members are not contiguous in memory
    order = np.argsort(np.concatenate([np.arange(m) * 2 + 1, np.arange(21) * 2 * (m // 21)]), kind="stable")
    pts = pts[order].astype(f32).astype(f64)
    if w is not None:
        w = np.concatenate([w, np.full(21, 0.75)])[order]
    cent = np.concatenate([np.zeros((1, 3)), far])
    return pts, w, cent


TIES_K = [2, 7, 8, 9, 15, 16, 17, 24, 32, 61, 64, 203, 255, 256]      # (32: chunks of 64 samples = 2 k, the paired scatter's limit)


def ties(k):
    """Samples on the 1/4 lattice around centres on lattice points, with duplicated centres in one SIMD lane (3 and 11), in
    different lanes (4 and 13), across the lane and leftover ranges (1 and k - 1 when k % 8 != 0), samples on a centre and midway
    between two, three and four centres; and a group far from the origin (coordinates near 6000) where the rounded distance to two
    centres 1/16 apart is negative before the clamp.  -> colors, None, centers"""
    side = int(np.ceil(k ** (1.0 / 3.0)))
    j = np.arange(k)
    cent = np.stack([j % side, (j // side) % side, j // (side * side)], axis=1).astype(f64) * 2.0
    if k > 13:
        cent[11] = cent[3]
        cent[13] = cent[4]
    if k % 8 != 0 and k > 2:
        cent[k - 1] = cent[1]
    p0, p1 = (5, 6) if k >= 7 else (0, 1)                                   # two centres 1/16 apart near 6000: both clamp to 0
    cent[p0] = [6000.0, 6000.0, 6000.0]
    cent[p1] = [6000.0625, 6000.0, 6000.0]
    g = np.arange(-2, 2 * side + 1, dtype=f64) * 0.5                        # the half lattice: on centres, midway on edges, faces, cells
    gx, gy, gz = np.meshgrid(g, g, g, indexing="ij")
    pts = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    t = np.arange(512, dtype=f64)                                          # the 1/64 lattice around the pair
    near = np.stack([6000.0 + (t % 16) / 64.0 - 3 / 32.0, 6000.0 + ((t // 16) % 8) / 64.0 - 1 / 16.0, 6000.0 + (t // 128) / 64.0 - 1 / 32.0], axis=1)
    pts = np.concatenate([pts, near, cent])
    perm = np.argsort(((np.arange(pts.shape[0], dtype=np.int64) * 40503) >> 2) % 10007, kind="stable")
    return pts[perm].astype(f32).astype(f64), None, cent


def degenerate_box(kind, k=24, n=3000):
    """All samples equal in one, two or three coordinates ("flat1", "flat2", "flat3"), ranges of 1e-30 and 1e-40 ("tiny30", "tiny40"),
    magnitudes of 1e15 and 1e-20 ("huge", "small"); some centres outside the samples' box.  -> colors, None, centers"""
    i = np.arange(n, dtype=np.int64)
    u = np.stack([((i * 2654435761) >> 5) % 4096, ((i * 40503) >> 3) % 4096, ((i * 2246822519) >> 7) % 4096], axis=1).astype(f64) / 4096.0
    scale, base = 1.0, 0.0
    if kind == "flat1":
        u[:, 1] = 0.375
    elif kind == "flat2":
        u[:, 1] = 0.375
        u[:, 2] = 0.625
    elif kind == "flat3":
        u[:] = [0.25, 0.375, 0.625]
    elif kind == "tiny30":
        scale, base = 1e-30, 0.5
    elif kind == "tiny40":
        scale, base = 1e-40, 0.0
    elif kind == "huge":
        scale = 1e15
    elif kind == "small":
        scale = 1e-20
    else:
        raise ValueError(kind)
    pts = (u * scale + base).astype(f32).astype(f64)
    jj = np.arange(k, dtype=f64)
    cu = np.stack([(jj * 0.37) % 1.0, (jj * 0.61) % 1.0, (jj * 0.83) % 1.0], axis=1)
    cu[::5] += 1.5                                                         # outside the box
    cu[1::7] -= 2.0
    cent = (cu * scale + base).astype(f32).astype(f64)
    return pts, None, cent


def starved(k, ncol, n=None):
    """ncol < k distinct colours (each many times): most clusters are empty in every iteration, those at index 0 and k - 1 among
    them.  -> colors, None, centers"""
    n = n if n is not None else max(4 * k, 40 * ncol)
    col = _lattice_centres(ncol, 4.0)
    pts = col[(np.arange(n, dtype=np.int64) * 7919) % ncol] + 0.0
    cent = _lattice_centres(k, 4.0) + 1000.0                                # far from every sample ...
    own = 1 + (np.arange(ncol) * max(1, (k - 2) // max(ncol, 1))) % max(k - 2, 1)
    own = np.unique(own)                                                   # ... except these, never index 0 or k - 1
    cent[own] = col[:own.shape[0]] + 0.125
    return pts, None, cent


def no_donor():
    """600 samples of 3 colours, k = 8 with five centres far away, weights 2^-10: every cluster weight sum is below 1"""
    col = np.array([[1.0, 2.0, 3.0], [5.0, 1.0, 2.0], [2.0, 6.0, 1.0]])
    pts = col[np.arange(600) % 3] + _offsets(600, 3)
    cent = np.concatenate([col[:1] + 0.1, np.full((2, 3), 500.0) + np.arange(2)[:, None], col[1:] + 0.1,
                           np.full((3, 3), -700.0) - np.arange(3)[:, None]])
    return pts.astype(f32).astype(f64), np.full(600, 2.0 ** -10), cent


def exact_sums_mean(x, w, members, qx, qw):
    """The order-free centroid of one cluster from Python Fractions: x (n,3) f32, members: indices -> three f32 and h"""
    sx = [0, 0, 0]
    sw = 0
    for i in members:
        wi = Fraction(float(w[i])) if w is not None else Fraction(1)
        for c in range(3):
            sx[c] += round(Fraction(float(x[i, c])) * wi / Fraction(2) ** qx)           # Fraction rounds half to even
        sw += round(wi / Fraction(2) ** qw) if w is not None else 1
    h = f32(float(Fraction(sw) * Fraction(2) ** qw)) if w is not None else f32(float(sw))
    c = np.array([f32(np.ldexp(float(s), qx)) for s in sx], f32)
    if h != 0:
        c = c * (f32(1) / h)
    return c, h
