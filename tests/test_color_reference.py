"""The references that tests/test_gpu_color_edges.py holds the device to, checked on the CPU.

* The long-double pow that measures `pamd_pow` in ulps, against mpmath at 40 digits.
* The oracle's own distance from the exact conversions (tests/color_ref.py), per conversion, input set and output plane: the
  committed table tests/golden/color_dref.json must not be smaller than what this machine measures.
"""
import json

import numpy as np
import pytest

from tests import color_ref as cr

mpmath = pytest.importorskip("mpmath")


@pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="long double is no wider than double on this platform")
@pytest.mark.parametrize("name", list(cr.POW_SITES))
def test_longdouble_pow_is_within_two_thousandths_of_an_ulp(name):
    """2 000 points per exponent, 400 from each input class of the device test (and the subnormal results): np.power on long double
    against mpmath.power, in ulps of the f64 result."""
    y = cr.POW_SITES[name][0]
    classes = cr.pow_inputs(name)
    rng = np.random.default_rng(11)
    per = 2000 // len(cr.POW_STRUCTURED + cr.POW_RANDOM)
    x = np.concatenate([rng.choice(classes[c], per) for c in cr.POW_STRUCTURED + cr.POW_RANDOM] + [classes.get("subnormal", np.zeros(0))[:200]])
    ref = cr.pow_reference(x, y)
    spacing = cr.f64_spacing(ref)
    ctx = mpmath.mp.clone()
    ctx.dps = 40
    worst = 0.0
    for xi, ri, si in zip(x, ref, spacing):
        exact = ctx.power(ctx.mpf(float(xi)), ctx.mpf(y))
        m, e = np.frexp(ri)                                        # long double -> mpf exactly: a 64-bit integer and a scale
        got = ctx.ldexp(ctx.mpf(int(np.ldexp(m, 64))), int(e) - 64)
        worst = max(worst, float(abs(got - exact) / ctx.mpf(float(si))))
    print("long double pow, y = %s: worst %.5f ulp of the f64 result over %d points" % (name, worst, x.size))
    assert worst <= 0.002


@pytest.mark.parametrize("name", cr.CONVERSIONS)
def test_oracle_distance_is_within_the_committed_table(name):
    """D_ref regenerated on the edge sets and on 20 000 random pixels; the committed table is not smaller, NaN lies where the exact
    chain has it, and the exact chain is the oracle's function: 1e-12 apart at the most where the chain is well conditioned."""
    committed = cr.load_dref()[name]
    sets = list(cr.edge_sets()[name]) + ["random"]
    assert sorted(committed) == sorted(sets)
    for key in sets:
        d, nan_mismatch = cr.measure_dref(name, key)
        print("D_ref %s / %s: measured %s, committed %s" % (name, key, ["%.3g" % v for v in d], committed[key]))
        assert nan_mismatch == 0, (key, nan_mismatch)
        assert all(c >= v for c, v in zip(committed[key], d)), (key, d, committed[key])
        if key != "extreme":
            assert max(d) <= 1e-12, (key, d)


def test_committed_table_is_what_the_generator_writes():
    """Plain numbers, three per set, rounded up to two digits by color_ref.round_up (so never below a measurement)."""
    with open(cr.DREF_PATH) as f:
        table = json.load(f)
    assert sorted(table) == sorted(cr.CONVERSIONS)
    for name, sets in table.items():
        for key, d in sets.items():
            assert len(d) == 3 and all(isinstance(v, float) and 0 <= v < 1e-9 for v in d), (name, key, d)
            assert all(cr.round_up(v) == v for v in d), (name, key, d)
    assert cr.round_up(1.234e-15) == 1.3e-15 and cr.round_up(1.2e-15) == 1.2e-15 and cr.round_up(9.91e-16) == 1e-15


def test_edge_sets_hold_what_they_are_for():
    """The knees sit between consecutive doubles of the sets, and the zero denominators are exact zeros in f64."""
    from oracle import binding as ob
    k = cr.knees()
    g = np.array(k["srgb_grey"])
    L = np.array([ob.convert("srgb_to_cieluv", np.array([v, v, v]))[0] for v in g])
    assert np.all(np.diff(g) > 0) and g.size == 128 and L[63] <= 8.0 < L[64]
    for ch, gs in enumerate(k["rec2020_grey"]):
        out = np.array([ob.convert("rec2020_to_srgb", np.array([v, v, v]))[ch] for v in gs])
        assert len(gs) == 128 and out[63] <= 0.0031308 * 12.92 < out[64]
    srgb = cr.edge_sets()["srgb_to_ictcp"]["edges"].reshape(3, -1)
    for v in (0.04045, 1e-200, 1.0, 17 / 255.0):
        assert np.any(srgb[0] == v) and np.any(srgb[1] == v) and np.any(srgb[2] == v)
    luv = cr.edge_sets()["cieluv_to_rec2020"]["edges"].reshape(3, -1)
    u0 = (4.0 * 0.95047) / (0.95047 + 15.0 * 1.0 + 3.0 * 1.08883)
    assert np.sum((luv[1] + 13.0 * luv[0] * u0 == 0.0) & (luv[0] > 0)) >= 8
