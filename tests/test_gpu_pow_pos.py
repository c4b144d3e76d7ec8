"""`pamd_pow_pos`, the branch-free pow of the common domain, against `pamd_pow`, bit for bit (color_device.h).

The reference throughout is `pamd_pow` (patolette_amd_debug_pow mode 0, patolette_amd_debug_convert general = 1), the routine the
ulp tests of tests/test_gpu_color_edges.py hold to 0.52 ulp.

(i)   `pamd_pow_pos` (mode 1) on its whole domain -- x positive, normal and finite, -1200 <= y log2(x) <= 1100 -- for the eight
      exponents of the conversions, about 2^22 inputs each: 2^21 log-uniform x over the part of the normal range that keeps the
      power in bounds, the 2^21 x = k / 2^21 of (0, 1], the 129 edges 1 + i/128 of the log table's intervals with two doubles on
      each side in every binade, the smallest and the largest x of the domain (the smallest and the largest normal numbers where
      the exponent admits them), and the x at which rint(Ph * 64) flips -- y log2(x) = (k + 1/2) / 64 for every k in bounds --
      with three doubles on each side.  A class is cut to the domain (the margin: 1e-6 in y log2(x), a billion times the rounding
      of the host's log2) and never empty.
(ii)  The vote.  Wavefronts of in-domain lanes with one lane outside -- 0, -0, a negative number, a subnormal, +inf, NaN, a power
      just above 1100 and one just below -1200 -- in lane 0, 31, 32 or 63, then a partial last wavefront with such a lane and one
      without: mode 2 (what `patolette_amd_pow` and the conversions run) equals mode 0 in every lane.
(iii) `k_convert` on 64 x 67 pixels, the eight conversions (the plain copy among them), from planar f64 and from 8-bit rows: the
      product's planes equal those of the run whose every vote is forced to fail.  The f64 sources hold values below 0, above 1,
      exactly 0 and 0.04045, and one NaN pixel.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import color_ref as cr

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

PH_LO, PH_HI, MARGIN = -1200.0, 1100.0, 1e-6
DBL_MIN, DBL_MAX = 2.2250738585072014e-308, 1.7976931348623157e308
W, H = 64, 67
CONVERSIONS = list(range(7)) + [100]                   # include/patolette_amd.h; 100: the plain copy (color_device.h PAMD_COPY)
SOURCE_OF = {0: "srgb_to_ictcp", 1: "srgb_to_cieluv", 2: "ictcp_to_rec2020", 3: "cieluv_to_rec2020", 4: "srgb_to_rec2020", 5: "rec2020_to_srgb",
             6: "cieluv_to_ictcp", 100: "srgb_to_rec2020"}          # color_ref.random_input: uniform sRGB taken into the conversion's source space


def _d(a):
    return a.ctypes.data_as(dp)


def _pow(gpu, x, y, mode):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    assert gpu.patolette_amd_debug_pow(_d(x), y, _d(out), x.size, mode) == 0
    return out


def _same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def _in_domain(x, y):
    with np.errstate(all="ignore"):
        p = y * np.log2(x)
        return (x >= DBL_MIN) & (x <= DBL_MAX) & (p >= PH_LO + MARGIN) & (p <= PH_HI - MARGIN)


def _t_range(y):
    """log2(x) over the domain: the normal range cut to the bounds of the power."""
    return max(-1022.0, (PH_LO + MARGIN) / y), min(1024.0 * (1 - 2.0 ** -52), (PH_HI - MARGIN) / y)


@functools.lru_cache(maxsize=None)
def _classes(name):
    y = cr.POW_SITES[name][0]
    assert y > 0
    rng = np.random.default_rng(500 + sorted(cr.POW_SITES).index(name))
    t_lo, t_hi = _t_range(y)
    out = {}
    with np.errstate(all="ignore"):
        return _cut(out, y, rng, t_lo, t_hi)


def _cut(out, y, rng, t_lo, t_hi):
    out["loguniform"] = np.exp2(t_lo + (t_hi - t_lo) * rng.random(1 << 21))
    out["unit"] = np.arange(1, (1 << 21) + 1, dtype=np.float64) / float(1 << 21)
    edges = np.concatenate([np.ldexp(1.0 + np.arange(129) / 128.0, e) for e in range(math.ceil(t_lo) - 1, math.floor(t_hi) + 1)])
    out["edges"] = cr._with_neighbours(edges, 2)
    ends = np.array([np.exp2(t_lo), np.exp2(t_hi), DBL_MIN, DBL_MAX])
    out["ends"] = cr._with_neighbours(ends, 3)
    k = np.arange(math.ceil(PH_LO * 64), math.floor(PH_HI * 64), dtype=np.float64)
    out["ties"] = cr._with_neighbours(np.exp2((k + 0.5) / (64 * y)), 3)
    for key in out:
        a = out[key]
        a = a[_in_domain(a, y)]
        a.setflags(write=False)
        out[key] = a
    return out


@pytest.mark.parametrize("name", list(cr.POW_SITES))
def test_pow_pos_returns_the_bits_of_pow_on_its_domain(gpu, name):
    y = cr.POW_SITES[name][0]
    classes = _classes(name)
    floors = {"loguniform": 2000000, "unit": 1000000, "edges": 129 * 5 * 20, "ends": 8, "ties": 10000}
    for key, least in floors.items():
        assert classes[key].size >= least, (key, classes[key].size)
    if y <= 1100.0 / 1024.0:                            # the whole normal range is inside: its two ends are
        assert DBL_MIN in classes["ends"] and DBL_MAX in classes["ends"]
    x = np.concatenate(list(classes.values()))
    pos, ref = _pow(gpu, x, y, 1), _pow(gpu, x, y, 0)
    same = _same_bits(pos, ref)
    at = 0
    for key, xs in classes.items():
        bad = ~same[at:at + xs.size]
        print("pow_pos y = %-5s %-10s n = %8d  differing %d" % (name, key, xs.size, int(bad.sum())))
        at += xs.size
    assert x.size > 3 << 20
    w = np.flatnonzero(~same)[:4]
    assert same.all(), [(float(x[i]).hex(), float(pos[i]).hex(), float(ref[i]).hex()) for i in w]
    assert not np.isnan(ref).any() and np.count_nonzero(ref) > 0.5 * x.size


def _odd_values(y):
    """lane values outside the domain -> why; the two powers beyond the bounds exist where |y| lets a normal x reach them."""
    odd = {"zero": 0.0, "minus zero": -0.0, "negative": -0.5, "subnormal": 1e-310, "inf": math.inf, "nan": math.nan}
    if (PH_HI + 0.5) / y < 1023.0:
        odd["above"] = 2.0 ** ((PH_HI + 0.5) / y)
    if (PH_LO - 0.5) / y > -1022.0:
        odd["below"] = 2.0 ** ((PH_LO - 0.5) / y)
    return odd


@pytest.mark.parametrize("name", list(cr.POW_SITES))
def test_one_lane_outside_the_domain_sends_its_wavefront_through_pow(gpu, name):
    y, lo, hi = cr.POW_SITES[name]
    odd = _odd_values(y)
    assert ("above" in odd and "below" in odd) == (y > 1200.5 / 1022.0), (name, sorted(odd))
    rng = np.random.default_rng(700 + sorted(cr.POW_SITES).index(name))
    fill = lambda n: max(lo, 1e-6) + (hi - max(lo, 1e-6)) * (1.0 - rng.random(n))          # noqa: E731  (in-domain lanes: the call site's range)
    waves, labels = [], []
    for why, v in odd.items():
        for lane in (0, 31, 32, 63):
            w = fill(64)
            w[lane] = v
            waves.append(w)
            labels.append((why, lane))
        waves.append(fill(64))                                    # a clean wavefront between the groups
        labels.append(("clean", -1))
    for why, v in odd.items():                                    # ... and as the partial last wavefront: 37 lanes hold 0, 31 and 32
        for lane in (0, 31, 32):
            w = fill(37)
            w[lane] = v
            x = np.concatenate(waves + [w])
            got, ref = _pow(gpu, x, y, 2), _pow(gpu, x, y, 0)
            same = _same_bits(got, ref)
            assert same.all(), (why, lane, [(labels[i // 64] if i // 64 < len(labels) else "tail", i % 64, float(x[i]).hex()) for i in np.flatnonzero(~same)[:4]])
    x = np.concatenate(waves + [fill(37)])                        # a partial last wavefront with every lane inside
    assert np.all(_in_domain(x[-37:], y))
    got, ref, pub = _pow(gpu, x, y, 2), _pow(gpu, x, y, 0), np.zeros_like(x)
    assert _same_bits(got, ref).all()
    assert gpu.patolette_amd_pow(_d(x), y, _d(pub), x.size) == 0 and _same_bits(pub, got).all()
    # the odd lanes got what pow answers there, the others a number
    assert np.isnan(got[labels.index(("nan", 0)) * 64]) and got[labels.index(("zero", 31)) * 64 + 31] == 0.0
    assert np.isfinite(got[-37:]).all()


def _convert(gpu, which, planar, bytes_, channels, general):
    n = W * H
    out = np.zeros(3 * n)
    rc = gpu.patolette_amd_debug_convert(which, _d(planar) if planar is not None else None,
                                         bytes_.ctypes.data_as(C.c_void_p) if bytes_ is not None else None, channels, _d(out), n, general)
    assert rc == 0
    return out


@functools.lru_cache(maxsize=None)
def _f64_source(which):
    n = W * H
    src = np.array(cr.random_input(SOURCE_OF[which], n, 90 + which), dtype=np.float64).reshape(3, n).copy()
    special = [-0.25, -1e-3, 1.5, 7.0, 0.0, -0.0, 0.04045, float(np.nextafter(0.04045, 1.0)), 1.0, 1e-310, 1e-200]
    for j, v in enumerate(special):                               # every special in each channel in turn, and in all three: the first
        for ch in range(3):                                       # wavefront; the rest of the image keeps whole wavefronts inside
            src[ch, 4 * j + ch] = v
        src[:, 4 * j + 3] = v
    src[:, 1000] = (math.nan, 0.5, 0.25)                          # one NaN pixel
    src[:, 2000] = 0.0                                            # black
    src.setflags(write=False)
    return src.reshape(-1)


@pytest.mark.parametrize("which", CONVERSIONS)
def test_convert_f64_equals_the_general_route(gpu, which):
    src = _f64_source(which)
    px = src.reshape(3, -1)
    assert (px < 0).any() and (px > 1).any() and (px == 0).any() and (px == 0.04045).any() and np.isnan(px).sum() == 1
    fast, general = _convert(gpu, which, src, None, 0, 0), _convert(gpu, which, src, None, 0, 1)
    same = _same_bits(fast, general)
    assert same.all(), [(int(i % (W * H)), int(i // (W * H)), float(fast[i]).hex(), float(general[i]).hex()) for i in np.flatnonzero(~same)[:4]]
    if which != 100:
        pub = src.copy()
        assert gpu.patolette_amd_convert(which, _d(pub), W * H) == 0 and _same_bits(pub, fast).all()
        assert np.isfinite(fast).mean() > 0.9
    else:
        assert _same_bits(fast, src).all()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("which", CONVERSIONS)
def test_convert_u8_equals_the_general_route(gpu, which, channels):
    rng = np.random.default_rng(60 + which + channels)
    px = rng.integers(0, 256, size=(W * H, channels), dtype=np.uint8)
    px[:6, :3] = [[0, 0, 0], [255, 255, 255], [10, 11, 10], [0, 255, 0], [11, 0, 10], [1, 1, 1]]     # 10 / 255 < 0.04045 < 11 / 255
    px[640:704, :3] = 0                                           # a black wavefront
    fast, general = _convert(gpu, which, None, px, channels, 0), _convert(gpu, which, None, px, channels, 1)
    same = _same_bits(fast, general)
    assert same.all(), [(int(i % (W * H)), int(i // (W * H)), float(fast[i]).hex(), float(general[i]).hex()) for i in np.flatnonzero(~same)[:4]]
    if which == 100:
        assert np.array_equal(fast.reshape(3, -1).T, px[:, :3] / 255.0)
