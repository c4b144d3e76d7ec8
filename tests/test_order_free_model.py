"""The order-free sums (devutil.h `make_bink` / `bin_split` / `bin_add`) as a numpy model (tests/split_model.py), at the grids the
code really builds: what they promise inside their limits, where the promise ends, and an input on which it does end.

Every addend v (|v| <= 2^E, at most 2^P of them) becomes v0, a multiple of g0 = 2^(E-B), and v1, a multiple of g1 = g0 2^-B
(B = 51 - P, clamped to 8 .. 40).  |v0| <= 2^B units of g0 and |v1| <= 2^(B-1) units of g1, so a sum of 2^P parts stays below
2^51 units: inside the 53-bit significand with a factor of four to spare, hence exact in any order.  The exact sums are taken
here as int64 counts of grid units (|sum| < 2^52: no overflow), and the f64 sums are held to them bit for bit.

The last tests are about the grids `convert_plan` (pipeline.hip) builds from the colour spaces' a-priori bounds, and about an
image far outside [0, 1]: CIELuv, 256 x 256, every sRGB channel in [7.5, 9].  Decoded without a clamp that would be L ~ 560 .. 600,
2^16 products L^2 ~ 3.4e5 against a bound of 2^16, a sum of 2.2e10 beyond 2^53 g0 = 2^34 -- and such addends DO give different
bits in two orders (test_addends_five_times_the_bound_break_the_model).  But no finite input gets there: the reference's
companding clamps the decoded channel to [0, 1], so every converted pixel is a point of the unit cube's image and the bounds hold
for whatever comes in (test_no_finite_input_leaves_the_a_priori_bounds); that image is plain white.  GPU test D therefore runs
as a check that nothing else gives way beyond [0, 1], not as a demonstration of order-dependence."""
import numpy as np
import pytest

from tests import color_ref as cr
from tests.split_model import bin_split, make_bink

# (E, P): the clamps of B first -- P < 11 gives B = 40, P > 43 gives B = 8 --
CLAMPS = [(0, 3), (0, 10), (-5, 10), (3, 11), (3, 43), (0, 44), (7, 50)]
# then what the code builds.  rootP = ceil(log2(pixels)): 13 for 97 x 61 and 2731 x 3, 14 for 5461 x 3, 16 for 2^16 - 1 and 2^16,
# 17 for 2^16 + 1, 19 for 512 x 513.  (1, rootP): ICtCp sums and moments; (8, rootP), (16, rootP): CIELuv sums and moments
# (pipeline.hip convert_plan).  read_bounds with a weight of 1000: e_lin = exp_bound(wmax max(cmax, 1)), e_quad =
# exp_bound(3 wmax max(range, cmax)^2) -- (10, 12) for ICtCp (cmax, range <= 1), (18, 28) for CIELuv (cmax ~ 180, range ~ 260),
# (10, 12) for sRGB; P = ceil(log2(pixels of the node)), any value up to rootP.  saliency.hip: kE_lab = 8, kE_cov = 17 with
# P = ceil(log2(pixels of the largest border band)).
USED = [(1, 13), (1, 14), (1, 16), (1, 17), (1, 19), (8, 13), (8, 16), (8, 17), (8, 19), (16, 13), (16, 16), (16, 17), (16, 19),
        (10, 13), (12, 13), (10, 19), (12, 19), (18, 13), (28, 13), (18, 19), (28, 19), (12, 1), (28, 5),
        (8, 9), (17, 9), (8, 15), (17, 15)]
MAX_ADDENDS_LOG2 = 18


def grid(E, P):
    B = min(40, max(8, 51 - P))
    return B, E - B, E - 2 * B                                     # B, log2 g0, log2 g1


def units(parts, log2_g):
    """The parts as int64 counts of their grid unit; asserts that they ARE on the grid."""
    u = np.ldexp(parts, -log2_g)
    assert np.array_equal(u, np.rint(u)) and float(np.max(np.abs(u), initial=0.0)) < 2.0 ** 62
    return u.astype(np.int64)


def pairwise(a):
    a = np.array(a, dtype=np.float64)
    while a.size > 1:
        if a.size & 1:
            a = np.concatenate([a, [0.0]])
        a = a[0::2] + a[1::2]
    return a[0]


def orders(parts, rng):
    """One f64 sum per order: front to back, back to front, shuffled (np.cumsum adds strictly in sequence), and by halves."""
    return {"forward": np.cumsum(parts)[-1], "reverse": np.cumsum(parts[::-1])[-1],
            "shuffled": np.cumsum(parts[rng.permutation(parts.size)])[-1], "pairwise": pairwise(parts)}


def addend_sets(E, n, rng):
    top = np.ldexp(1.0, E)
    yield "all +2^E", np.full(n, top)
    yield "all -2^E", np.full(n, -top)
    yield "alternating", top * np.where(np.arange(n) & 1, -1.0, 1.0)
    yield "random", top * (2.0 * rng.random(n) - 1.0)
    yield "random positive", top * rng.random(n)
    yield "tiny and huge", top * rng.random(n) * np.ldexp(1.0, -rng.integers(0, 90, size=n))


@pytest.mark.parametrize("E,P", CLAMPS + USED, ids=lambda v: str(v))
def test_sums_of_split_addends_are_exact_in_any_order(E, P):
    B, lg0, lg1 = grid(E, P)
    assert B == (40 if P < 11 else 8 if P > 43 else 51 - P)
    bink = make_bink(E, P)
    assert bink == (np.ldexp(1.5, 52 + lg0), np.ldexp(1.5, 52 + lg1))
    n = 1 << min(P, MAX_ADDENDS_LOG2)
    rng = np.random.default_rng(1000 * P + E + 50)
    for name, v in addend_sets(E, n, rng):
        v0, v1 = bin_split(v, bink)
        # the split itself: v0 is v rounded to the coarse grid, v1 the remainder rounded to the fine grid
        assert np.all(np.abs(v - v0) <= np.ldexp(0.5, lg0)) and np.all(np.abs((v - v0) - v1) <= np.ldexp(0.5, lg1)), name
        for parts, lg in ((v0, lg0), (v1, lg1)):
            total = int(units(parts, lg).sum())
            assert abs(total) <= 1 << 51, name
            exact = np.ldexp(float(total), lg)                      # |total| < 2^53: float(total) and the scaling are exact
            for order, s in orders(parts, rng).items():
                assert s.view(np.uint64) == exact.view(np.uint64) or (s == 0.0 and exact == 0.0), (name, order, s, exact)


@pytest.mark.parametrize("E,P", [(16, 16), (1, 13), (8, 17)], ids=lambda v: str(v))
def test_exactness_ends_at_four_times_the_bound(E, P):
    """The headroom of the design: 2^P addends of up to s 2^E stay exact in every order for s = 1, 2, 3 and 4 -- the sums reach
    2^53 units and every partial sum is still a 53-bit integer -- and no further: at s = 4 1/8 the partial sums pass 2^53 units,
    odd counts are rounded, and the sequential sums leave the exact value that the sum by halves still finds (its partial sums are
    the addend times a power of two).  The addends are an odd count of units just inside s 2^E, so nothing hides in trailing zeros."""
    B, lg0, _ = grid(E, P)
    bink = make_bink(E, P)
    n = 1 << P
    rng = np.random.default_rng(7)
    differs = {}
    for s in (1.0, 2.0, 3.0, 4.0, 4.125):
        v = np.full(n, np.ldexp(s, E) - np.ldexp(1.0, lg0))        # (s 2^B - 1) units of g0: odd
        v0, v1 = bin_split(v, bink)
        assert np.array_equal(v0, v) and not v1.any()              # on the coarse grid already: the split still works at 4x
        exact_units = int(units(v0, lg0).sum())
        got = orders(v0, rng)
        differs[s] = len({float(x) for x in got.values()}) > 1
        if s <= 4.0:
            assert exact_units < 1 << 53
            assert all(x == np.ldexp(float(exact_units), lg0) for x in got.values()), (s, got)
        else:
            assert exact_units > 1 << 53 and got["pairwise"] == np.ldexp(float(exact_units), lg0)
            assert got["forward"] != got["pairwise"], (s, got)
    assert differs == {1.0: False, 2.0: False, 3.0: False, 4.0: False, 4.125: True}


# ---- beyond the a-priori bounds: the images of GPU test D (tests/test_gpu_order_free.py) ----
BEYOND_W, BEYOND_H = 256, 256                                      # 2^16 pixels: rootP = 16, B = 35, g0 = 2^-19 for the CIELuv moments


def beyond_unit_image(kind):
    """(n, 3) row-major sRGB outside [0, 1].  "far": every channel uniform in [7.5, 9] (seed 20) -- had the conversion no clamp, L
    would be 560 .. 600.  "wide": uniform in [-0.25, 1.25] (seed 21), a sixth of the channels beyond either end: not flat once
    converted, the clamp at work on a third of the values."""
    n = BEYOND_W * BEYOND_H
    if kind == "far":
        return 7.5 + 1.5 * np.random.default_rng(20).random((n, 3))
    return -0.25 + 1.5 * np.random.default_rng(21).random((n, 3))


def test_addends_five_times_the_bound_break_the_model():
    """What `convert_plan`'s CIELuv moment grid, make_bink(16, 16), does with 2^16 products L^2 for L in 560 .. 600 -- the L that
    116 cbrt(Y) - 16 gives for linear Y ~ 130, i.e. for sRGB channels of 7.5 .. 9 decoded WITHOUT a clamp: every addend is beyond
    four times the bound, the coarse parts sum to 2.2e10 > 2^53 g0 = 2^34, and the forward and the reverse sum of the same parts
    differ in their bits.  Addends like these must never reach grids built for 2^16."""
    rng = np.random.default_rng(20)
    L = 560.0 + 40.0 * rng.random(BEYOND_W * BEYOND_H)
    B, lg0, _ = grid(16, 16)
    assert (B, lg0) == (35, -19)
    prod = L * L
    assert prod.min() > 4.0 * 2.0 ** 16
    v0, _ = bin_split(prod, make_bink(16, 16))
    assert np.all(np.abs(prod - v0) <= np.ldexp(0.5, lg0))         # the split is still a split: it is the SUM that leaves the grid
    exact_units = int(units(v0, lg0).sum())
    assert exact_units > 1 << 53
    fwd, rev = np.cumsum(v0)[-1], np.cumsum(v0[::-1])[-1]
    print("sum of L^2 coarse parts: exact %d units of 2^-19, forward %r, reverse %r" % (exact_units, fwd, rev))
    assert fwd.view(np.uint64) != rev.view(np.uint64)


def _extreme_srgb():
    """Finite sRGB far outside [0, 1], (n, 3): the two images of GPU test D, every corner of the cubes [-s, s]^3 and [0, s]^3 for
    s up to the largest double, and noise over sixty binades of either sign."""
    rng = np.random.default_rng(22)
    corners = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)], dtype=np.float64)
    big = [s * c for s in (1.0, 1.5, 9.0, 1e10, 1e300, np.finfo(np.float64).max) for c in (corners, 2.0 * corners - 1.0)]
    spread = (2.0 * rng.random((20000, 3)) - 1.0) * np.ldexp(1.0, rng.integers(-30, 30, size=(20000, 3)))
    return np.concatenate([beyond_unit_image("far"), beyond_unit_image("wide")] + big + [spread])


@pytest.mark.parametrize("name,e_sum,e_mom", [("srgb_to_cieluv", 8, 16), ("srgb_to_ictcp", 1, 1)])
def test_no_finite_input_leaves_the_a_priori_bounds(ob, name, e_sum, e_mom):
    """Why the out-of-bound input of the issue behind tests/test_gpu_order_free.py does NOT break the sums that ride with the colour
    conversion: sRGB.c:70-89 clamps the decoded channel to [0, 1] (`gamma_decode`, the device's too: color_device.h), so whatever
    finite value comes in, the conversions see a point of the unit cube -- L <= 100.000004, |u|, |v| < 2^8; |I|, |Ct|, |Cp| < 2^1 --
    and every product stays inside the bound `convert_plan` built the moment grid for.  The image with channels in [7.5, 9] is
    plain white, 65 536 times.  Both orders of the binned sums of values and products are the exact sum, bit for bit."""
    colors = _extreme_srgb()
    n = colors.shape[0]
    out = cr.convert_f64(name, np.ascontiguousarray(colors.T).reshape(-1)).reshape(3, n)
    assert np.all(np.isfinite(out))
    assert float(np.abs(out).max()) < 2.0 ** e_sum
    far = out[:, :BEYOND_W * BEYOND_H]
    assert np.all(far == far[:, :1])                               # the "far" image: one colour
    if name == "srgb_to_cieluv":
        assert 100.0 <= far[0, 0] < 100.00001
    P = int(np.ceil(np.log2(n)))
    rng = np.random.default_rng(23)
    ja, jb = (0, 1, 2, 1, 2, 2), (0, 0, 0, 1, 1, 2)                # xx, yx, zx, yy, zy, zz as k_convert takes them
    for E, addends in [(e_sum, out[j]) for j in range(3)] + [(e_mom, out[a] * out[b]) for a, b in zip(ja, jb)]:
        assert float(np.abs(addends).max()) < 2.0 ** E
        _, lg0, lg1 = grid(E, P)
        for parts, lg in zip(bin_split(addends, make_bink(E, P)), (lg0, lg1)):
            exact = np.ldexp(float(int(units(parts, lg).sum())), lg)
            for order, s in orders(parts, rng).items():
                assert s == exact, (E, order, s, exact)
