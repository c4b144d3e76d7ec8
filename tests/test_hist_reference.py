"""ColorHistogram without a GPU: the symbols, the checks made before the library is touched, and the unit model.

  * every patolette_amd_hist_* symbol is declared in the header, bound in _native.SYMBOLS and exported by the library;
  * every Python-side ValueError of `add`, `merge` and of a closed histogram is raised before anything crosses into C: the library
    is replaced by a stub that answers the table's allocation and clear and fails the test on any other call;
  * the unit model the GPU tests hold the kernels to (tests/hist_ref.py): rint(w * 2^32), ties to even."""
import os

import numpy as np
import pytest

from tests import hist_ref
from tests.util import ROOT

NAMES = ("patolette_amd_hist_bytes", "patolette_amd_hist_clear", "patolette_amd_hist_add_u8", "patolette_amd_hist_add_u8_device",
         "patolette_amd_hist_merge", "patolette_amd_hist_totals", "patolette_amd_hist_export", "patolette_amd_hist_palette")


def test_symbols_declared_bound_and_exported(native):
    with open(os.path.join(ROOT, "include", "patolette_amd.h")) as fh:
        header = fh.read()
    L = native.lib()
    for name in NAMES:
        assert name + "(" in header
        assert name in native.SYMBOLS
        assert hasattr(L, name)
    assert native.SYMBOLS["patolette_amd_hist_add_u8"] == native.SYMBOLS["patolette_amd_hist_add_u8_device"]
    assert len(native.SYMBOLS["patolette_amd_hist_add_u8"][1]) == 11
    # the table's size needs no device: a 64-byte header, 2^24 counts, and as many unit sums when weighted
    assert L.patolette_amd_hist_bytes(0) == 64 + 8 * 2 ** 24
    assert L.patolette_amd_hist_bytes(1) == 64 + 16 * 2 ** 24
    import patolette_amd as p
    assert "ColorHistogram" in p.__all__


class _Stub:
    """Stands in for the library: the table's life and nothing else."""

    def __init__(self):
        self.freed = []

    def patolette_amd_hist_bytes(self, weighted):
        return 64 + (16 if weighted else 8) * 2 ** 24

    def patolette_amd_malloc(self, n):
        return 0x1000

    def patolette_amd_hist_clear(self, ptr, weighted):
        return 0

    def patolette_amd_free(self, ptr):
        self.freed.append(ptr)

    def __getattr__(self, name):
        raise AssertionError("the library was touched: " + name)


@pytest.fixture
def stub(monkeypatch):
    from patolette_amd import _native
    s = _Stub()
    monkeypatch.setattr(_native, "lib", lambda: s)
    return s


class _FakeDevice:
    def __init__(self, index):
        self.index = index

    def __str__(self):
        return "cuda:%d" % self.index


class _FakeTensor:
    """Just enough of a CUDA uint8 tensor for the checks ahead of the library."""
    is_cuda = True

    def __init__(self, shape, index):
        import torch
        self.shape, self.device, self.dtype = shape, _FakeDevice(index), torch.uint8

    def contiguous(self):
        return self

    def data_ptr(self):
        raise AssertionError("the tensor's memory was asked for")


def test_value_errors_come_before_the_library(stub):
    import patolette_amd as p
    rgb = np.zeros((4, 5, 3), dtype=np.uint8)
    rgba = np.zeros((2, 4, 5, 4), dtype=np.uint8)
    with p.ColorHistogram() as h, p.ColorHistogram(weighted=True) as hw:
        assert not h.weighted and hw.weighted
        for bad in (rgb.astype(np.float32), rgb.astype(np.int8), np.zeros((4, 5), dtype=np.uint8), np.zeros((4, 5, 2), dtype=np.uint8),
                    np.zeros((1, 2, 4, 5, 3), dtype=np.uint8), np.zeros((4, 5, 5), dtype=np.uint8)):
            with pytest.raises(ValueError):
                h.add(bad)                                                  # dtype or shape
        with pytest.raises(ValueError):
            h.add(rgb, weights=np.ones(20))                                 # weights given to an unweighted histogram
        with pytest.raises(ValueError):
            h.add(rgb, tile_size=64)                                        # ... or a tile size to derive them
        with pytest.raises(ValueError):
            hw.add(rgb)                                                     # neither given to a weighted one
        with pytest.raises(ValueError):
            hw.add(rgb, tile_size=0)
        with pytest.raises(ValueError):
            hw.add(rgb, tile_size=-1)
        with pytest.raises(ValueError):
            hw.add(rgb, weights=np.ones(19))                                # one weight per pixel
        with pytest.raises(ValueError):
            hw.add(rgba, weights=np.ones(20))
        for thr in (-1, 256, 1.5, True, "128"):
            with pytest.raises(ValueError):
                h.add(rgba, alpha_threshold=thr)                            # outside 0..255
        with pytest.raises(ValueError):
            h.add(rgb, alpha_threshold=128)                                 # 3-channel pixels have no alpha
        with pytest.raises(ValueError):
            h.add(_FakeTensor((4, 5, 3), 1))                                # a tensor on another device than the histogram's (0)
        with pytest.raises(ValueError):
            h.merge(hw)                                                     # another mode
        with pytest.raises(ValueError):
            h.merge(h)
        with pytest.raises(ValueError):
            h.merge(rgb)
    assert len(stub.freed) == 2


def test_use_after_close(stub):
    import patolette_amd as p
    rgb = np.zeros((4, 5, 3), dtype=np.uint8)
    h, other = p.ColorHistogram(), p.ColorHistogram()
    h.close()
    h.close()                                                               # twice is fine
    assert len(stub.freed) == 1
    for use in (lambda: h.add(rgb), lambda: h.clear(), lambda: h.merge(other), lambda: other.merge(h), lambda: h.pixels, lambda: h.colors,
                lambda: h.export(), lambda: h.palette(16)):
        with pytest.raises(ValueError):
            use()
    other.close()
    assert len(stub.freed) == 2


def test_unit_model():
    u = hist_ref.units(np.array([2.0 ** -33, 3 * 2.0 ** -33, 1.0, 2.0 ** 20, 0.0, 5 * 2.0 ** -33, 0.5 + 2.0 ** -33]))
    assert u.dtype == np.uint64
    assert [int(v) for v in u] == [0, 2, 2 ** 32, 2 ** 52, 0, 2, 2 ** 31]       # ties go to even
    assert not hist_ref.weights_ok(np.array([1.0, np.nan])) and not hist_ref.weights_ok(np.array([np.inf]))
    assert not hist_ref.weights_ok(np.array([-2.0 ** -40])) and not hist_ref.weights_ok(np.array([2.0 ** 20 + 1]))
    assert hist_ref.weights_ok(np.array([0.0, 2.0 ** 20]))


def test_model_counts_and_sums():
    px = np.array([[[1, 2, 3], [1, 2, 3], [0, 0, 9]], [[255, 0, 0], [1, 2, 3], [0, 0, 9]]], dtype=np.uint8)
    w = np.array([0.5, 0.25, 1.0, 2.0, 2.0 ** -33, 0.0])
    colors, counts, weights = hist_ref.model(px)
    assert colors.tolist() == [[0, 0, 9], [1, 2, 3], [255, 0, 0]] and counts.tolist() == [2, 3, 1]
    assert weights.tolist() == [2.0, 3.0, 1.0]
    colors, counts, weights = hist_ref.model(px, w)
    assert counts.tolist() == [2, 3, 1] and weights.tolist() == [1.0, 0.75, 2.0]
    rgba = np.concatenate([px, np.array([[[0], [127], [128]], [[255], [200], [3]]], dtype=np.uint8)], axis=2)
    colors, counts, _ = hist_ref.model(rgba, alpha_threshold=128)
    assert colors.tolist() == [[0, 0, 9], [1, 2, 3], [255, 0, 0]] and counts.tolist() == [1, 1, 1]
