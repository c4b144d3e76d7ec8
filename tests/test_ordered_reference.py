"""The ordered remap's definition (tests/ordered_ref.py) and the parts of its surface that need no GPU.

  * the Bayer function is a permutation of 0..63 with the two rows the header quotes;
  * ordered_spread is the header's formula: on a byte palette, on a float palette with trailing fill, 1/3 for four even greys, 0.0
    for one row.  Two summation orders of at most a few hundred f64 terms: compared to 1e-12 relative;
  * on a grey ramp with those four greys the reference's 8x8 block means are closer to the image's at the default spread than at
    spread 0 (what an ordered dither is for);
  * remap() rejects an unknown dither name and a negative or NaN spread before the library is touched; so do the two composed
    entries; the two symbols are declared and bound."""
import os

import numpy as np
import pytest

from tests import ordered_ref
from tests.util import ROOT

GREYS = np.array([[0, 0, 0], [85, 85, 85], [170, 170, 170], [255, 255, 255]], dtype=np.uint8)


def test_bayer_is_a_permutation_with_the_quoted_rows():
    yy, xx = np.mgrid[0:8, 0:8]
    b = ordered_ref.bayer8(xx, yy)
    assert sorted(b.reshape(-1).tolist()) == list(range(64))
    assert b[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42]
    assert b[1].tolist() == [48, 16, 56, 24, 50, 18, 58, 26]
    assert np.array_equal(ordered_ref.bayer8(xx + 8, yy + 16), b)                 # taken on (x & 7, y & 7)
    t = ordered_ref.threshold(8, 8)
    assert t.min() == -0.5 + 0.5 / 64 and t.max() == 0.5 - 0.5 / 64 and t.sum() == 0.0


def test_ordered_spread_is_the_formula():
    import patolette_amd
    assert "ordered_spread" in patolette_amd.__all__
    rng = np.random.default_rng(3)
    pal8 = rng.integers(0, 256, size=(37, 3), dtype=np.uint8)
    assert patolette_amd.ordered_spread(pal8) == pytest.approx(ordered_ref.ordered_spread(pal8), rel=1e-12)
    palf = np.full((12, 3), -1.0)
    palf[:9] = rng.random((9, 3))
    palf[4] = -1.0                                                                # an inner -1 row is a colour
    want = ordered_ref.ordered_spread(palf)
    assert want == ordered_ref.ordered_spread(palf[:9])                           # the trailing fill is not a colour
    for form in (palf, np.asfortranarray(palf), palf[:9]):
        assert patolette_amd.ordered_spread(form) == pytest.approx(want, rel=1e-12)
    assert patolette_amd.ordered_spread(GREYS) == pytest.approx(1.0 / 3.0, rel=1e-12)
    assert patolette_amd.ordered_spread(GREYS.astype(np.float64) / 255.0) == pytest.approx(1.0 / 3.0, rel=1e-12)
    assert patolette_amd.ordered_spread(GREYS[:1]) == 0.0
    one = np.full((5, 3), -1.0)
    one[0] = 0.25
    assert patolette_amd.ordered_spread(one) == 0.0
    with pytest.raises(ValueError):
        patolette_amd.ordered_spread(np.zeros((4, 4), dtype=np.uint8))


def test_the_default_spread_brings_block_means_closer_on_a_grey_ramp(ob):
    import patolette_amd
    h, w = 64, 256
    ramp = np.repeat(np.arange(w, dtype=np.uint8)[None, :, None], h, axis=0).repeat(3, axis=2)
    spread = patolette_amd.ordered_spread(GREYS)
    _, q0, _ = ordered_ref.remap(ob, ramp, GREYS, 0.0)
    _, qs, _ = ordered_ref.remap(ob, ramp, GREYS, spread)
    _, q1, _ = ordered_ref.remap(ob, ramp, GREYS, 1.0)
    e0, es, e1 = (ordered_ref.block_rmse(ramp, q) for q in (q0, qs, q1))
    print("8x8 block-mean RMSE on the ramp: nearest %.2f, spread %.4f: %.2f, spread 1: %.2f" % (e0, spread, es, e1))
    assert es < e0


def test_spread_zero_is_the_nearest_recipe(ob):
    from tests import remap_ref
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(24, 40, 4), dtype=np.uint8)
    pal = rng.integers(0, 256, size=(16, 3), dtype=np.uint8)
    m, q, _ = ordered_ref.remap(ob, img, pal, 0.0)
    m_nn, q_nn = remap_ref.remap(ob, img, pal, dither=False)
    assert np.array_equal(m, m_nn) and np.array_equal(q, q_nn)
    frames = rng.integers(0, 256, size=(3, 37, 53, 3), dtype=np.uint8)           # 37 * 53 is no multiple of 64: the origin is the frame's
    maps, _, _ = ordered_ref.remap(ob, frames, pal, 0.3)
    for i in range(3):
        assert np.array_equal(maps[i], ordered_ref.remap(ob, frames[i], pal, 0.3)[0])
    stacked, _, _ = ordered_ref.remap(ob, frames.reshape(3 * 37, 53, 3), pal, 0.3)
    assert np.any(stacked.reshape(3, 37, 53) != maps)


def test_bad_arguments_raise_before_the_library_is_touched(monkeypatch):
    import patolette_amd
    from patolette_amd import _native

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_native, "lib", no_library)
    good = np.zeros((4, 5, 3), dtype=np.uint8)
    pal = np.arange(12, dtype=np.uint8).reshape(4, 3)
    for dither in ("bayer", "Ordered", "", None, 2, 0.5):
        with pytest.raises(ValueError):
            patolette_amd.remap(good, pal, dither=dither)
    for spread in (-0.1, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError):
            patolette_amd.remap(good, pal, dither="ordered", spread=spread)
        with pytest.raises(ValueError):
            patolette_amd.quantize_u8(good, 4, dither="ordered", spread=spread)
        with pytest.raises(ValueError):
            patolette_amd.quantize_frames(good[None], 4, dither="ordered", spread=spread)
    with pytest.raises(ValueError):
        patolette_amd.quantize_frames(good[None], 4, dither="bayer")
    with pytest.raises(ValueError):
        patolette_amd.quantize_u8(good, 4, dither="bayer")


def test_symbols_declared_and_bound():
    from patolette_amd import _native
    with open(os.path.join(ROOT, "include", "patolette_amd.h")) as fh:
        header = fh.read()
    for name in ("patolette_amd_remap_ordered_u8", "patolette_amd_remap_ordered_u8_device"):
        assert name + "(" in header
        assert name in _native.SYMBOLS
    args = _native.SYMBOLS["patolette_amd_remap_ordered_u8"][1]
    assert len(args) == 13 and args == _native.SYMBOLS["patolette_amd_remap_ordered_u8_device"][1]
    import ctypes as C
    assert args[8] is C.c_double                                                  # spread, where the other remap has its dither flag


def test_symbols_exported(native):
    L = native.lib()                                                              # loading needs no GPU
    assert L.patolette_amd_remap_ordered_u8 and L.patolette_amd_remap_ordered_u8_device
