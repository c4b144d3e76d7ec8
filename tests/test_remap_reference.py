"""The remap recipe (tests/remap_ref.py) checked against the CPU oracle alone, and the parts of the surface that need no GPU.

  * idempotence, exact: the quantized image of an oracle patolette() run, remapped onto that run's byte palette, is itself, and the
    map is the run's own (a pixel on an entry is at distance 0; the dither's error stays 0);
  * a fixed palette (the 216 web-safe colours): more than one index, and the dithered map is not the nearest one;
  * three frames: each frame's map is the recipe on that frame alone, and with dithering NOT the recipe on the stacked image;
  * the two symbols are declared and bound; remap() rejects bad shapes and dtypes before the library is touched."""
import os

import numpy as np
import pytest

from tests import remap_ref
from tests.util import ROOT, scene


def _scene_u8(h, w, seed):
    return np.round(scene(h, w, seed) * 255).astype(np.uint8)


def _websafe():
    v = np.array([0, 51, 102, 153, 204, 255], dtype=np.uint8)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)


@pytest.mark.parametrize("run_dither", [True, False])
def test_idempotence_on_the_oracle(ob, run_dither):
    h, w, K = 48, 72, 32
    img = _scene_u8(h, w, 3)
    flat = ob.planar(img.reshape(-1, 3).astype(np.float64) / 255.0)
    ec, pal, pmap = ob.patolette(w, h, flat, None, K, dither=run_dither, color_space=2, kmeans_niter=4, kmeans_max_samples=1024)
    assert ec == 0
    p8 = remap_ref.pal8(pal)
    assert len({tuple(r) for r in p8}) == K                       # distinct byte rows: an index is defined by its colour
    own = pmap.astype(np.int64).reshape(h, w)
    q = p8[own]
    for dither in (True, False):
        m, quant = remap_ref.remap(ob, q, p8, dither=dither)
        assert np.array_equal(p8[m], q) and np.array_equal(quant, q)
        assert np.array_equal(m, own)


def test_fixed_palette(ob):
    img = _scene_u8(48, 72, 3)
    pal = _websafe()
    assert pal.shape == (216, 3)
    m_nn, q_nn = remap_ref.remap(ob, img, pal, dither=False)
    m_di, q_di = remap_ref.remap(ob, img, pal, dither=True)
    assert len(np.unique(m_nn)) > 1 and len(np.unique(m_di)) > 1
    assert np.any(m_nn != m_di)
    assert np.array_equal(q_nn, pal[m_nn]) and np.array_equal(q_di, pal[m_di])
    assert m_nn.max() < 216 and m_di.max() < 216


def test_three_frames_are_mapped_one_by_one(ob):
    f, h, w = 3, 40, 56
    frames = np.stack([_scene_u8(h, w, 11 + i) for i in range(f)])
    pal = _websafe()
    for dither in (True, False):
        maps, quant = remap_ref.remap(ob, frames, pal, dither=dither)
        assert maps.shape == (f, h, w) and quant.shape == (f, h, w, 3)
        for i in range(f):
            mi, qi = remap_ref.remap(ob, frames[i], pal, dither=dither)
            assert np.array_equal(maps[i], mi) and np.array_equal(quant[i], qi)
        stacked, _ = remap_ref.remap(ob, frames.reshape(f * h, w, 3), pal, dither=dither)
        if dither:
            assert np.mean(stacked.reshape(f, h, w) != maps) > 0.05              # one curve through the stack is another walk
        else:
            assert np.array_equal(stacked.reshape(f, h, w), maps)


def test_float_palette_rows(ob):
    pal = np.full((6, 3), -1.0)
    pal[:3] = [[0.1, 0.2, 0.3], [1.0, 0.0, 0.5], [-1.0, -1.0, -1.0]]            # an inner -1 row is a colour; only trailing ones go
    pal[3] = [0.9, 0.9, 0.9]
    rows = remap_ref.palette_rows(np.asfortranarray(pal))
    assert rows.shape == (4, 3) and np.array_equal(rows, pal[:4])
    assert np.array_equal(remap_ref.pal8(pal), [[25, 51, 76], [255, 0, 127], [0, 0, 0], [229, 229, 229], [0, 0, 0], [0, 0, 0]])


def test_symbols_declared_and_bound():
    from patolette_amd import _native
    with open(os.path.join(ROOT, "include", "patolette_amd.h")) as fh:
        header = fh.read()
    for name in ("patolette_amd_remap_u8", "patolette_amd_remap_u8_device", "patolette_amd_debug_remap_two_pass"):
        assert name + "(" in header
        assert name in _native.SYMBOLS
    assert len(_native.SYMBOLS["patolette_amd_remap_u8"][1]) == 13
    assert _native.SYMBOLS["patolette_amd_remap_u8"][1] == _native.SYMBOLS["patolette_amd_remap_u8_device"][1]


def test_symbols_exported(native):
    L = native.lib()                                               # loading needs no GPU
    assert L.patolette_amd_remap_u8 and L.patolette_amd_remap_u8_device and L.patolette_amd_debug_remap_two_pass


def test_bad_arguments_raise_before_the_library_is_touched(monkeypatch):
    import patolette_amd
    from patolette_amd import _native

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_native, "lib", no_library)
    assert "remap" in patolette_amd.__all__
    good = np.zeros((4, 5, 3), dtype=np.uint8)
    pal = np.zeros((4, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        patolette_amd.remap(good.astype(np.float64), pal)         # a float image
    with pytest.raises(ValueError):
        patolette_amd.remap(good, np.zeros((4, 4), dtype=np.uint8))   # a (K, 4) palette
    with pytest.raises(ValueError):
        patolette_amd.remap(np.zeros((4, 5), dtype=np.uint8), pal)    # a 2-D image
    with pytest.raises(ValueError):
        patolette_amd.remap(np.zeros((4, 5, 2), dtype=np.uint8), pal)
    with pytest.raises(ValueError):
        patolette_amd.remap(good, np.zeros((0, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        patolette_amd.remap(good, np.zeros((4, 3), dtype=bool))
    with pytest.raises(ValueError):
        patolette_amd.remap(good, np.zeros((4, 3), dtype=np.int64))   # integers other than uint8: neither bytes nor sRGB in [0, 1]
