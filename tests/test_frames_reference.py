"""The frames recipe (tests/frames_ref.py) is the reference's own path, checked against the CPU oracle alone.

  * one frame: the recipe -- palette in the quantisation space from a palette_only call, then the map stage by hand -- equals the
    monolithic oracle.binding.patolette call, palette and map, ICtCp and CIELuv, dither on and off;
  * three frames, dither on: the maps differ from the stacked call's map (the recipe does not silently dither the stack), and
    dither off they equal it."""
import numpy as np
import pytest

from tests import frames_ref
from tests.util import scene


def _frames(f, h, w, seed):
    return np.stack([np.round(scene(h, w, seed + i) * 255).astype(np.uint8) for i in range(f)])


KW = dict(kmeans_niter=4, kmeans_max_samples=1024)


@pytest.mark.parametrize("cs", [2, 1])
@pytest.mark.parametrize("dither", [True, False])
def test_one_frame_is_the_monolithic_call(ob, cs, dither):
    h, w, K = 40, 56, 24
    fr = _frames(1, h, w, 3)
    pal, maps = frames_ref.quantize_frames(ob, fr, K, dither=dither, color_space=cs, **KW)
    flat = ob.planar(frames_ref.u8_frames(fr)[0])
    ec, pal_o, map_o = ob.patolette(w, h, flat, None, K, dither=dither, color_space=cs, **KW)
    assert ec == 0
    assert np.array_equal(maps[0].reshape(-1), map_o.astype(np.int64))
    assert np.max(np.abs(pal - pal_o)) == 0.0


@pytest.mark.parametrize("cs", [2, 1])
def test_three_frames_are_not_the_dithered_stack(ob, cs):
    f, h, w, K = 3, 40, 56, 24
    fr = _frames(f, h, w, 11)
    stacked = ob.planar(frames_ref.u8_frames(fr).reshape(-1, 3))
    pal, maps = frames_ref.quantize_frames(ob, fr, K, dither=True, color_space=cs, **KW)
    ec, pal_o, map_o = ob.patolette(w, f * h, stacked, None, K, dither=True, color_space=cs, **KW)
    assert ec == 0
    assert np.max(np.abs(pal - pal_o)) == 0.0                      # one palette ...
    differ = np.mean(maps.reshape(-1) != map_o.astype(np.int64))
    assert differ > 0.05, differ                                   # ... but not one curve through all frames
    # without dithering the map is position-independent: the recipe IS the stacked call
    pal, maps = frames_ref.quantize_frames(ob, fr, K, dither=False, color_space=cs, **KW)
    ec, pal_o, map_o = ob.patolette(w, f * h, stacked, None, K, dither=False, color_space=cs, **KW)
    assert np.array_equal(maps.reshape(-1), map_o.astype(np.int64)) and np.max(np.abs(pal - pal_o)) == 0.0
