"""tests/measure_ref.py, the reference of measure, checked against the contract's consequences on the CPU oracle -- and the argument
checks `patolette_amd.measure` makes before it crosses into C, `psnr`, and the exported symbols.  No GPU."""
import functools

import numpy as np
import pytest

import patolette_amd
from tests import delta_ref, measure_ref, remap_ref
from tests.test_gpu_remap import _palette

SIZES = [((40, 56), 1), ((37, 53), 3)]


@functools.lru_cache(maxsize=None)
def _case(size, F, rows, kind):
    from oracle import binding as ob
    frames, pal = delta_ref.clip(size[0], size[1], F), _palette(rows, seed=2)
    maps = delta_ref.maps_of(ob, frames, pal, kind)
    for a in (frames, pal, maps):
        a.setflags(write=False)
    return frames, pal, maps


@pytest.mark.parametrize("kind", ["nearest", "ordered"])
@pytest.mark.parametrize("rows", [2, 16, 255])
@pytest.mark.parametrize("size,F", SIZES)
def test_consequences(ob, size, F, rows, kind):
    frames, pal, maps = _case(size, F, rows, kind)
    N = F * size[0] * size[1]
    for skip in (None, rows, int(maps[0, 0, 0])):                     # none; one that no element holds; a used row
        ent, per, dist = measure_ref.measure(ob, frames, maps, pal, skip_index=skip)
        skipped = 0 if skip is None else int(np.sum(maps == skip))
        assert skip != int(maps[0, 0, 0]) or skipped > 0
        assert ent.shape == (rows, 3) and per.shape == (F, 3) and dist.shape == (F, 2)
        assert ent[:, 0].sum() == per[:, 0].sum() == N - skipped
        assert ent[:, 1].sum() == per[:, 1].sum()
        assert ent[:, 2].max() == per[:, 2].max()
        counts = np.bincount(maps.reshape(-1), minlength=rows)
        if skip is not None and skip < rows:
            counts[skip] = 0
        assert np.array_equal(ent[:, 0], counts)
        assert np.all(ent[ent[:, 0] == 0] == 0)                       # rows that nothing names hold 0
        assert np.all(dist[:, 1] <= dist[:, 0]) and np.all(dist[:, 0] <= dist[:, 1] * per[:, 0])
        again = measure_ref.measure(ob, frames, maps, pal, skip_index=skip, ictcp=False)
        assert again[2] is None and np.array_equal(again[0], ent) and np.array_equal(again[1], per)


@pytest.mark.parametrize("dither", [False, True])
def test_frame_sse_is_the_error_of_the_quantized_image(ob, dither):
    frames = delta_ref.clip(37, 53, 3)
    for pal in (_palette(16, seed=2), _palette(16, seed=2).astype(np.float64) / 255.0 * 0.999):
        maps, quant = remap_ref.remap(ob, frames, pal, dither=dither)
        ent, per, _ = measure_ref.measure(ob, frames, maps, pal, ictcp=False)
        err = (frames.astype(np.int64) - quant.astype(np.int64)) ** 2
        assert np.array_equal(per[:, 1], err.reshape(3, -1).sum(axis=1))
        assert np.array_equal(per[:, 2], err.sum(axis=-1).reshape(3, -1).max(axis=1))


def test_a_quantized_image_on_its_own_map_has_no_error(ob):
    frames, pal, maps = _case((37, 53), 3, 16, "nearest")
    quant = pal[maps]
    ent, per, dist = measure_ref.measure(ob, quant, maps, pal)
    assert np.all(ent[:, 1:] == 0) and np.all(per[:, 1:] == 0) and np.all(dist == 0.0)
    assert np.all(np.isinf(patolette_amd.psnr(per)))


def test_two_by_two_by_hand(ob):
    """Every number written out.  Palette rows 0: (10, 20, 30), 1: (200, 100, 0), 2: unused by the map."""
    pal = np.array([[10, 20, 30], [200, 100, 0], [1, 2, 3]], dtype=np.uint8)
    image = np.array([[[10, 20, 30], [13, 16, 30]], [[200, 100, 0], [190, 100, 5]]], dtype=np.uint8)
    maps = np.array([[0, 0], [1, 1]], dtype=np.uint8)
    ent, per, dist = measure_ref.measure(ob, image, maps, pal)
    # e: 0, 9 + 16 = 25, 0, 100 + 25 = 125
    assert ent.tolist() == [[2, 25, 25], [2, 125, 125], [0, 0, 0]]
    assert per.tolist() == [[4, 150, 125]]
    assert dist.shape == (1, 2) and dist[0, 0] > dist[0, 1] > 0
    ent, per, dist = measure_ref.measure(ob, image, maps, pal, skip_index=1)          # a skip index that names a used row
    assert ent.tolist() == [[2, 25, 25], [0, 0, 0], [0, 0, 0]] and per.tolist() == [[2, 25, 25]]
    maps3 = np.array([[0, 3], [3, 1]], dtype=np.uint8)                                # ... and one beyond the rows
    ent, per, dist = measure_ref.measure(ob, image, maps3, pal, skip_index=3)
    assert ent.tolist() == [[1, 0, 0], [1, 125, 125], [0, 0, 0]] and per.tolist() == [[2, 125, 125]]
    ent, per, dist = measure_ref.measure(ob, image, np.full((2, 2), 3), pal, skip_index=3)
    assert not ent.any() and per.tolist() == [[0, 0, 0]] and dist.tolist() == [[0.0, 0.0]]
    # a float palette: pal8 truncates, the ICtCp part takes the rows as given; trailing -1 rows are dropped but counted as rows
    palf = np.array([[10.9 / 255, 20.5 / 255, 30.5 / 255], [200.5 / 255, 100.2 / 255, 0.0], [-1, -1, -1], [-1, -1, -1]])
    ent, per, dist_f = measure_ref.measure(ob, image, maps, palf)
    assert ent.tolist() == [[2, 25, 25], [2, 125, 125], [0, 0, 0], [0, 0, 0]] and per.tolist() == [[4, 150, 125]]
    assert dist_f[0, 0] != measure_ref.measure(ob, image, maps, pal)[2][0, 0]


def test_psnr():
    p = patolette_amd.psnr(np.array([[4, 150, 125], [7, 0, 0], [0, 0, 0]]))
    assert p.shape == (3,)
    assert p[0] == 10.0 * np.log10(3.0 * 255.0 * 255.0 * 4 / 150) and np.isposinf(p[1]) and np.isnan(p[2])
    one = patolette_amd.psnr(np.array([4, 150, 125]))
    assert isinstance(one, float) and one == p[0]
    assert patolette_amd.psnr(np.zeros((0, 3), dtype=np.int64)).shape == (0,)
    with pytest.raises(ValueError, match="count, sse, max_se"):
        patolette_amd.psnr(np.zeros((3, 2)))


def test_measure_checks_its_arguments_before_any_library_call(monkeypatch):
    """Every ValueError below is raised before libpatolette_amd.so is asked for anything."""
    from patolette_amd import _native

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "lib", no_library)
    maps = np.zeros((2, 4, 5), dtype=np.uint8)
    frames = np.zeros((2, 4, 5, 3), dtype=np.uint8)
    pal = _palette(16, seed=2)
    with pytest.raises(ValueError, match="image must be"):             # the image: type, dimensions, channels
        patolette_amd.measure(frames.astype(np.float64), maps, pal)
    with pytest.raises(ValueError, match="image must be"):
        patolette_amd.measure(frames[0, 0], maps, pal)
    with pytest.raises(ValueError, match="image must be"):
        patolette_amd.measure(frames[..., :2], maps, pal)
    with pytest.raises(ValueError, match="maps must be"):              # the maps: type, dimensions
        patolette_amd.measure(frames, maps.astype(np.int64), pal)
    with pytest.raises(ValueError, match="maps must be"):
        patolette_amd.measure(frames, maps[0, 0], pal)
    with pytest.raises(ValueError, match="maps must be"):
        patolette_amd.measure(frames, [[0]], pal)
    with pytest.raises(ValueError, match="do not match"):              # the two together
        patolette_amd.measure(frames, maps[:, :3], pal)
    with pytest.raises(ValueError, match="do not match"):
        patolette_amd.measure(frames, maps[:1], pal)
    with pytest.raises(ValueError, match="do not match"):
        patolette_amd.measure(frames[0], maps[:1], pal)
    with pytest.raises(ValueError, match="do not match"):
        patolette_amd.measure(frames[:1], maps[0], pal)
    with pytest.raises(ValueError, match="palette must be"):           # the palette
        patolette_amd.measure(frames, maps, 16)
    with pytest.raises(ValueError, match="palette must be"):
        patolette_amd.measure(frames, maps, pal.astype(np.int32))
    with pytest.raises(ValueError, match="palette must be"):
        patolette_amd.measure(frames, maps, pal[:0])
    for bad in (-1, -7, 1.0, "0", True):                               # skip_index
        with pytest.raises(ValueError, match="skip_index"):
            patolette_amd.measure(frames, maps, pal, skip_index=bad)


def test_the_surface():
    assert "measure" in patolette_amd.__all__ and "psnr" in patolette_amd.__all__
    assert "measure" in patolette_amd.__doc__ and "psnr" in patolette_amd.__doc__


def test_both_symbols_are_exported(native):
    L = native.lib()
    for name in ("patolette_amd_measure", "patolette_amd_measure_device"):
        assert name in native.SYMBOLS and hasattr(L, name)
