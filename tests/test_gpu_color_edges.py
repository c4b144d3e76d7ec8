"""The colour stage at its edges: `pamd_pow` in ulps, and the conversions where their branches, clamps and loops turn.

Part one, `patolette_amd_pow` against pow in long double (within 0.002 ulp of exact, tests/test_color_reference.py), one upload per
exponent, for the eight exponents of the conversions.  Input classes (tests/color_ref.py `pow_inputs`): the 129 edges of the log
table's intervals in every binade the call site reaches plus 2^-40 and 2^14, x next to 1, the x at which rint(Ph * 64) flips, 200 000
uniform x in the call site's range and 200 000 log-uniform in [2^-40, 2^15), each structured point with three doubles on each side.

  * normal results: <= 0.52 ulp, the figure color_device.h documents.  Its basis is the routine's host model against binary128
    (worst 0.5149 ulp over 24 M inputs) plus 0.005 for what sampling does not find -- not the device's own figures.
  * subnormal results: <= 0.76 of the subnormal spacing: 0.5 from ldexp's rounding plus 0.515 ulp of a normal result whose ulp is
    at most half that spacing.
  * incorrectly rounded results: <= 0.5 % of a random class, <= 1.5 % of a structured one (host model: 0.24 %, 0.46 % for edges and
    ties, 0.96 % next to 1).  Where the long double cannot tell which double is nearest, mpmath does (color_ref.correctly_rounded).
  * +0, -0, inf, NaN, -1, -0.25: what libm answers.

Part two, `patolette_amd_convert` against the oracle on the edge sets of tests/color_ref.py and on random content at n = 1, 255, 256,
257 and 1 048 576 + 300 (the grid is capped at 1 048 576 threads: some threads take the grid-stride loop's second turn with its
prefetched pixel, others do not).  NaN exactly where the oracle has it; routes without pow equal bit for bit; elsewhere per plane
|got - want| <= 4 D_ref max|want|, D_ref (tests/golden/color_dref.json) being the oracle's own distance from the exact chain on
the same kind of input: a last-ulp pow neighbour is noise of that kind and size, and 4 leaves room for the nine of an ICtCp chain.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import color_ref as cr

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

POW_BOUND = 0.52                 # color_device.h, DESIGN.md 4.1, include/patolette_amd.h
SUBNORMAL_BOUND = 0.76
SHARE_RANDOM, SHARE_STRUCTURED = 0.005, 0.015
SPECIALS = (0.0, -0.0, math.inf, math.nan, -1.0, -0.25)
BIG = 1048576 + 300
SHAPES = (1, 255, 256, 257, BIG)


def _d(a):
    return a.ctypes.data_as(dp)


# ----------------------------------------------------------------------------------------------------------------------
# part one: pamd_pow
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pow_run(name):
    """One upload for the exponent: class -> (x, got, reference in long double), read-only."""
    from patolette_amd import _native
    y = cr.POW_SITES[name][0]
    classes = dict(cr.pow_inputs(name))
    classes["special"] = np.array(SPECIALS)
    x = np.concatenate(list(classes.values()))
    got = np.zeros_like(x)
    assert _native.lib().patolette_amd_pow(_d(x), y, _d(got), x.size) == 0
    out, at = {}, 0
    for key, xs in classes.items():
        g = got[at:at + xs.size].copy()
        at += xs.size
        ref = cr.pow_reference(xs, y) if key != "special" else None
        for a in (g, ref):
            if a is not None:
                a.setflags(write=False)
        out[key] = (xs, g, ref)
    return out


def _split(x, got, ref):
    """(ulp error, normal mask, subnormal mask, overflow mask) of one class."""
    with np.errstate(over="ignore"):
        rounded = ref.astype(np.float64)
    overflow = np.isinf(rounded)
    normal = ~overflow & (ref >= np.longdouble(2.0) ** -1022)
    err = cr.ulp_error(np.where(overflow, 0.0, got), ref)
    return err, normal, ~overflow & ~normal, overflow


def _interval(x):
    m, _ = math.frexp(x)
    return int((2 * m - 1) * 128) & 127


@pytest.mark.parametrize("name", list(cr.POW_SITES))
def test_pow_normal_results_within_the_documented_bound(gpu, name):
    run = _pow_run(name)
    failures = []
    for key in cr.POW_STRUCTURED + cr.POW_RANDOM + ("tiny",):
        x, got, ref = run[key]
        err, normal, _, overflow = _split(x, got, ref)
        assert np.all(np.isinf(got[overflow]) & (got[overflow] > 0)), key
        sel = np.ones_like(normal) if key == "tiny" else normal     # the tiny x are held to the bound whatever they give
        if not sel.any():
            continue
        w = int(np.argmax(np.where(sel, err, -1.0)))
        print("pow y = %-5s %-10s n = %7d  worst %.4f ulp at x = %s (log interval %d)" % (name, key, int(sel.sum()), err[w], float(x[w]).hex(), _interval(x[w])))
        if not err[w] <= POW_BOUND:
            bad = sel & ~(err <= POW_BOUND)
            failures.append((key, float(err[w]), float(x[w]).hex(), "log intervals %s" % sorted({_interval(v) for v in x[bad]})[:8], int(bad.sum())))
    assert not failures, failures


@pytest.mark.parametrize("name", list(cr.POW_SITES))
def test_pow_subnormal_results_within_three_quarters_of_their_spacing(gpu, name):
    """Results in [2^-1074, 2^-1022) (x chosen for them with y = 3 and 2.4) and, in every class, whatever else falls below 2^-1022."""
    run = _pow_run(name)
    assert ("subnormal" in run) == (name in ("3", "2.4"))
    seen = 0
    for key in cr.POW_STRUCTURED + cr.POW_RANDOM + (("subnormal",) if "subnormal" in run else ()):
        x, got, ref = run[key]
        err, _, sub, _ = _split(x, got, ref)
        if not sub.any():
            continue
        seen += int(sub.sum())
        w = int(np.argmax(np.where(sub, err, -1.0)))
        print("pow y = %-5s %-10s subnormal results n = %6d  worst %.4f of the spacing at x = %s" % (name, key, int(sub.sum()), err[w], float(x[w]).hex()))
        assert err[w] <= SUBNORMAL_BOUND, (key, float(err[w]), float(x[w]).hex())
    if "subnormal" in run:
        x, got, ref = run["subnormal"]
        assert seen >= x.size and np.count_nonzero(got) > 0.99 * x.size


@pytest.mark.parametrize("name", list(cr.POW_SITES))
def test_pow_share_of_incorrectly_rounded_results(gpu, name):
    run = _pow_run(name)
    failures = []
    for key in cr.POW_STRUCTURED + cr.POW_RANDOM:
        x, got, ref = run[key]
        _, normal, _, _ = _split(x, got, ref)
        share = float(np.mean(got[normal] != cr.correctly_rounded(x[normal], cr.POW_SITES[name][0], ref[normal])))
        print("pow y = %-5s %-10s incorrectly rounded %.3f %% of %d" % (name, key, 100 * share, int(normal.sum())))
        if share > (SHARE_RANDOM if key in cr.POW_RANDOM else SHARE_STRUCTURED):
            failures.append((key, share))
    assert not failures, failures


@pytest.mark.parametrize("name", list(cr.POW_SITES))
def test_pow_special_values_are_libm_s(gpu, name):
    """-0 and +0 compare equal: pow(-0, 3) is +0 on the device and -0 in libm, and no call site can ask for it (the one integer
    exponent is reached with (L + 16) / 116, L > 8)."""
    y = cr.POW_SITES[name][0]
    x, got, _ = _pow_run(name)["special"]
    for xi, gi in zip(x, got):
        try:
            want = math.pow(xi, y)
        except ValueError:                                          # a negative base with a non-integer exponent
            want = math.nan
        assert (math.isnan(want) and math.isnan(gi)) or gi == want, (xi, y, gi, want)


# ----------------------------------------------------------------------------------------------------------------------
# part two: the conversions
# ----------------------------------------------------------------------------------------------------------------------
def _gpu_convert(gpu, name, src):
    got = np.array(src, dtype=np.float64, copy=True)
    assert gpu.patolette_amd_convert(cr.CONV_ID[name], _d(got), got.size // 3) == 0
    return got


def _same(got, want):
    """Equal as doubles, NaN matching NaN (the sign of a zero, which fmax(-0, 0) leaves open in C, is not compared)."""
    return (got == want) | (np.isnan(got) & np.isnan(want))


def _check(name, key, got, want, label):
    """NaN positions, infinities, and the per-plane bar 4 D_ref max|want|; returns the measured ratios to D_ref."""
    got, want = got.reshape(3, -1), want.reshape(3, -1)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, "NaN at", np.argwhere(np.isnan(got) != np.isnan(want))[:4].tolist())
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and not np.any(np.isinf(got) & ~inf), label
    ratios, failures = [], []
    for p in range(3):
        fin = np.isfinite(want[p])
        dref, scale = cr.load_dref()[name][key][p], cr.plane_scale(want[p])
        dist = float(np.max(np.abs(got[p][fin] - want[p][fin]))) if fin.any() else 0.0
        ratios.append(dist / (dref * scale) if dref * scale > 0 else (0.0 if dist == 0 else math.inf))
        if not dist <= 4 * dref * scale:
            i = int(np.argmax(np.where(fin, np.abs(got[p] - want[p]), -1.0)))
            failures.append(dict(plane=p, pixel=i, got=float(got[p][i]), want=float(want[p][i]), dist=dist, bar=4 * dref * scale))
    print("convert %-18s %-22s distance / (D_ref max|want|) per plane: %s" % (name, label, ", ".join("%.3f" % r for r in ratios)))
    assert not failures, (label, failures)
    return ratios


def _edge_cases():
    return [("srgb_to_ictcp", "edges"), ("srgb_to_cieluv", "edges"), ("srgb_to_rec2020", "edges"), ("rec2020_to_srgb", "edges"),
            ("cieluv_to_rec2020", "edges"), ("cieluv_to_ictcp", "edges"), ("ictcp_to_rec2020", "edges"), ("ictcp_to_rec2020", "extreme")]


@pytest.mark.parametrize("name,key", _edge_cases(), ids=lambda v: v)
def test_convert_edge_sets(gpu, name, key):
    assert sorted(k for n, k in _edge_cases() if n == name) == sorted(cr.edge_sets()[name])
    src = cr.edge_sets()[name][key]
    _check(name, key, _gpu_convert(gpu, name, src), cr.oracle_convert(name, key), key)


def _lin_srgb(rec2020):
    """rec2020_to_srgb up to the companding, operation by operation as sRGB.c:32-59 + xyz.c:42-64 in f64."""
    r2, g2, b2 = rec2020
    x = r2 * 0.63695351 + g2 * 0.14461919 + b2 * 0.16885585
    y = r2 * 0.26269834 + g2 * 0.67800877 + b2 * 0.0592929
    z = g2 * 0.02807314 + b2 * 1.06082723
    return (x * 3.2404542 - y * 1.5371385 - z * 0.4985314, -x * 0.9692660 + y * 1.8760108 + z * 0.0415560,
            x * 0.0556434 - y * 0.2040259 + z * 1.0572252)


def _pow_free(name, src):
    """The pixels of a planar input whose conversion evaluates no pow: decided on the same f64 values as the C code."""
    px = src.reshape(3, -1)
    with np.errstate(invalid="ignore"):
        if name in ("srgb_to_rec2020", "srgb_to_cieluv"):
            sel = np.all(px <= 0.0404500, axis=0)
            if name == "srgb_to_cieluv":                           # ... and yr <= 216/24389 (xyz.c:27-39 on the companded values)
                r, g, b = (np.fmin(np.fmax(px[p] / 12.92, 0.0), 1.0) for p in range(3))
                sel &= (r * 0.2126729 + g * 0.7151522 + b * 0.0721750) / 1.0 <= 216.0 / 24389.0
            return sel
        if name == "rec2020_to_srgb":
            return np.all(np.array(_lin_srgb(px)) <= 0.0031308, axis=0)
        assert name == "cieluv_to_rec2020"
        return px[0] <= 8.0


@pytest.mark.parametrize("name", ["srgb_to_rec2020", "srgb_to_cieluv", "rec2020_to_srgb", "cieluv_to_rec2020"])
def test_convert_pow_free_routes_bit_for_bit(gpu, name):
    """c / 12.92 and v / 10000 go through div_const (Markstein's three-instruction division), the rest is plain f64: nothing here
    may differ from the oracle.  The edge set's pow-free pixels, and for sRGB in 100 000 uniform values in [0, 0.04045] per channel."""
    src = cr.edge_sets()[name]["edges"]
    want = cr.oracle_convert(name, "edges").reshape(3, -1)
    got = _gpu_convert(gpu, name, src).reshape(3, -1)
    sel = _pow_free(name, src)
    assert sel.sum() >= 100, int(sel.sum())
    bad = ~np.all(_same(got, want), axis=0) & sel
    print("pow-free %-18s edge pixels %d, differing %d" % (name, int(sel.sum()), int(bad.sum())))
    assert not bad.any(), (int(bad.sum()), src.reshape(3, -1)[:, bad][:, :3].tolist(), got[:, bad][:, :3].tolist(), want[:, bad][:, :3].tolist())
    if name.startswith("srgb"):
        dark = np.random.default_rng(9).random(3 * 100000) * 0.04045
        dark[:3] = (0.04045, 0.0, 0.04045)
        assert _pow_free(name, dark).sum() > (0 if name == "srgb_to_cieluv" else dark.size // 3 - 1)
        want, got = cr.convert_f64(name, dark), _gpu_convert(gpu, name, dark)
        sel = _pow_free(name, dark)
        bad = ~np.all(_same(got, want).reshape(3, -1), axis=0) & sel
        print("pow-free %-18s uniform [0, 0.04045]: %d pixels, differing %d" % (name, int(sel.sum()), int(bad.sum())))
        assert not bad.any(), (int(bad.sum()), dark.reshape(3, -1)[:, bad][:, :3].tolist())


KNEE_CASES = [("srgb_to_rec2020", "companding"), ("srgb_to_cieluv", "companding"), ("srgb_to_ictcp", "companding"),
              ("srgb_to_cieluv", "yr"), ("rec2020_to_srgb", "encoding"), ("cieluv_to_rec2020", "L"), ("cieluv_to_ictcp", "L")]


def _knee_pixels(label):
    """Planar input right at a knee: 0.04045 and its neighbours in every channel, the located greys, L around 8."""
    k = cr.knees()
    if label == "companding":
        return cr._pixels(cr.neighbours(0.04045, 2))
    if label == "yr":
        return cr._planar([[g, g, g] for g in k["srgb_grey"]])
    if label == "encoding":
        return cr._cat(*[cr._planar([[g, g, g] for g in gs]) for gs in k["rec2020_grey"]])
    return cr._planar([[L, u, v] for L in k["L"] for (u, v) in ((0.0, 0.0), (3.0, -2.0))])


@pytest.mark.parametrize("name,label", KNEE_CASES, ids=lambda v: v)
def test_convert_knees_take_the_oracle_s_side(gpu, name, label):
    """Only the pixels at a knee, so that max|want| is theirs: the companding is not continuous at 0.04045 and at 0.0031308, and a
    `<` for a `<=` moves exactly one double across."""
    src = _knee_pixels(label)
    _check(name, "edges", _gpu_convert(gpu, name, src), cr.convert_f64(name, src), "knee " + label)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("name", cr.CONVERSIONS)
def test_convert_shapes(gpu, name, n):
    """Random content held to the bars of the random set.  At 1 048 576 + 300 the first 300 threads convert two pixels each."""
    src = cr.random_input(name, n, 77 + n % 13)
    want = cr.convert_f64(name, src)
    got = _gpu_convert(gpu, name, src)
    _check(name, "random", got, want, "n = %d" % n)
    if n == BIG:                                                    # where a wrong second turn would show first
        assert np.all(_same(got.reshape(3, n)[:, 1048576:], want.reshape(3, n)[:, 1048576:]).mean(axis=1) > 0.9)
