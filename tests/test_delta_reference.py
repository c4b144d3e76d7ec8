"""tests/delta_ref.py, the reference of frame_deltas, checked against the contract's consequences on the CPU oracle -- and the
argument checks `patolette_amd.frame_deltas` makes before it crosses into C.  No GPU."""
import functools

import numpy as np
import pytest

import patolette_amd
from tests import delta_ref
from tests.test_gpu_remap import _palette

SIZES = [((40, 56), 5), ((37, 53), 4)]


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
@pytest.mark.parametrize("tolerance", [0.0, 0.02, 0.05])
def test_consequences(ob, tolerance, size, F, rows, kind):
    frames, pal, maps = _case(size, F, rows, kind)
    T = rows
    deltas, shown, rects, changed, gap, tested, kept = delta_ref.frame_deltas(ob, maps, pal, frames=frames, tolerance=tolerance)
    h, w = size
    # replaying the deltas gives back `shown`
    assert np.array_equal(delta_ref.replay(deltas, T), shown)
    assert np.array_equal(deltas[0], maps[0]) and tuple(rects[0]) == (0, 0, w, h) and changed[0] == h * w
    if tolerance == 0.0:
        assert np.array_equal(shown, maps) and tested == 0
        assert np.array_equal(deltas[1:] != T, maps[1:] != maps[:-1])
    else:
        # every shown entry is the frame's own choice or within `tolerance` of that frame's source pixel
        dist2 = delta_ref.distances2(ob, frames, pal, shown)
        assert np.all((shown == maps) | (dist2 <= np.float64(tolerance) * np.float64(tolerance)))
        assert tested >= kept and (rows < 16 or 0 < kept < tested)
    # rectangles are tight and nothing outside them differs from T
    for f in range(1, F):
        x0, y0, rw, rh = (int(v) for v in rects[f])
        move = deltas[f] != T
        assert changed[f] == int(np.sum(move))
        assert tuple(rects[f]) == delta_ref.rect_of(move)
        outside = np.ones((h, w), dtype=bool)
        outside[y0:y0 + rh, x0:x0 + rw] = False
        assert not np.any(move & outside)
        if changed[f]:
            assert move[y0].any() and move[y0 + rh - 1].any() and move[:, x0].any() and move[:, x0 + rw - 1].any()


def test_the_lossy_rectangle_is_the_moving_block(ob):
    """(40, 56), 16 rows: with the exact mode the noise dirties the whole frame; at tolerance 0.05 frame 1's rectangle lies strictly
    inside the exact one."""
    frames, pal, maps = _case((40, 56), 5, 16, "ordered")
    exact = delta_ref.frame_deltas(ob, maps, pal)
    lossy = delta_ref.frame_deltas(ob, maps, pal, frames=frames, tolerance=0.05)
    (ex, ey, ew, eh), (lx, ly, lw, lh) = (tuple(int(v) for v in r[2][1]) for r in (exact, lossy))
    print("frame 1: exact rect %s changed %d, lossy rect %s changed %d" % ((ex, ey, ew, eh), exact[3][1], (lx, ly, lw, lh), lossy[3][1]))
    assert lw > 0 and lh > 0
    assert lx >= ex and ly >= ey and lx + lw <= ex + ew and ly + lh <= ey + eh
    assert lw * lh < ew * eh and lossy[3][1] < exact[3][1]


def test_an_unchanged_frame_and_an_explicit_index(ob):
    frames, pal, maps = _case((37, 53), 4, 16, "nearest")
    twice = np.concatenate([maps[:2], maps[1:2], maps[2:]])
    deltas, shown, rects, changed, *_ = delta_ref.frame_deltas(ob, twice, 16, T=255)
    assert tuple(rects[2]) == (0, 0, 0, 0) and changed[2] == 0 and np.all(deltas[2] == 255)
    assert np.array_equal(delta_ref.replay(deltas, 255), twice) and np.array_equal(shown, twice)


def test_frame_deltas_checks_its_arguments_before_any_library_call(monkeypatch):
    """Every ValueError below is raised before libpatolette_amd.so is asked for anything."""
    from patolette_amd import _native

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "lib", no_library)
    maps = np.zeros((2, 4, 5), dtype=np.uint8)
    frames = np.zeros((2, 4, 5, 3), dtype=np.uint8)
    pal256 = _palette(256, seed=2)
    with pytest.raises(ValueError, match="one row less"):              # no free index in the map's dtype
        patolette_amd.frame_deltas(maps, pal256)
    with pytest.raises(ValueError, match="one row less"):
        patolette_amd.frame_deltas(maps, 256)
    with pytest.raises(ValueError, match="one row less"):
        patolette_amd.frame_deltas(maps, pal256[:16], transparent_index=256)
    with pytest.raises(ValueError, match="at least"):                  # an index some entry uses
        patolette_amd.frame_deltas(maps, pal256[:16], transparent_index=15)
    with pytest.raises(ValueError, match="do not match"):              # a shape mismatch
        patolette_amd.frame_deltas(maps, pal256[:16], frames=frames[:, :3], tolerance=0.05)
    with pytest.raises(ValueError, match="do not match"):
        patolette_amd.frame_deltas(maps, pal256[:16], frames=frames[:1], tolerance=0.05)
    with pytest.raises(ValueError, match="frames"):
        patolette_amd.frame_deltas(maps, pal256[:16], frames=frames[0], tolerance=0.05)
    with pytest.raises(ValueError, match="frames"):                    # the lossy mode without pixels
        patolette_amd.frame_deltas(maps, pal256[:16], tolerance=0.05)
    for bad in (-0.01, float("nan"), float("inf"), "much"):            # a bad tolerance
        with pytest.raises(ValueError, match="tolerance"):
            patolette_amd.frame_deltas(maps, pal256[:16], frames=frames, tolerance=bad)
    with pytest.raises(ValueError, match="row count"):                 # an int palette with tolerance > 0
        patolette_amd.frame_deltas(maps, 16, frames=frames, tolerance=0.05)
    with pytest.raises(ValueError, match="maps must be"):
        patolette_amd.frame_deltas(maps.astype(np.int64), 16)
    with pytest.raises(ValueError, match="maps must be"):
        patolette_amd.frame_deltas(maps[0], 16)
    assert "frame_deltas" in patolette_amd.__all__
