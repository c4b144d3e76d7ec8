"""tests/rgba_delta_ref.py, the reference of frame_deltas_rgba, checked against the contract's consequences (include/patolette_amd.h),
against delta_ref on fully opaque maps, against a case written out by hand and against PIL -- and the argument checks
`patolette_amd.frame_deltas_rgba` and `write_gif`'s per-frame disposal make before they cross into C.  No GPU."""
import numpy as np
import pytest

import patolette_amd
from tests import delta_ref, lzw_ref, rgba_delta_ref
from tests.test_gpu_remap import _palette


def _random_maps(rng, trial):
    """Up to 6 frames of up to 11 x 11 with indices 1 .. 4: a moving sprite, random holes, static holes, fully opaque."""
    F, h, w = int(rng.integers(1, 7)), int(rng.integers(1, 12)), int(rng.integers(1, 12))
    kind = trial % 4
    maps = rng.integers(1, 5, size=(F, h, w))
    if kind == 0:
        sprite = np.zeros_like(maps)
        sh, sw = max(1, h // 3), max(1, w // 3)
        for f in range(F):
            y, x = (2 * f) % h, (3 * f) % w
            sprite[f, y:y + sh, x:x + sw] = maps[f, y:y + sh, x:x + sw]
        maps = sprite
    elif kind == 1:
        maps = np.where(rng.random((F, h, w)) < 0.4, 0, maps)
    elif kind == 2:
        maps = np.where(rng.random((1, h, w)) < 0.4, 0, maps[:1].repeat(F, 0))
        maps = np.where((maps != 0) & (rng.random((F, h, w)) < 0.3), 1 + maps % 4, maps)          # colours change, visibility does not
    return kind, maps


def test_consequences_on_random_small_maps():
    rng = np.random.default_rng(1)
    seen_two, seen_v_only = 0, 0
    for trial in range(240):
        kind, maps = _random_maps(rng, trial)
        F, h, w = maps.shape
        loop = bool(trial & 4)
        for lossy in (False, True):
            near = rng.random((F, h, w)) < 0.5 if lossy else None
            d, s, r, disp, c, *_ = rgba_delta_ref.frame_deltas(None, maps, 5, loop=loop, near=near)
            assert np.array_equal(s != 0, maps != 0)                   # transparency is never lossy
            if not lossy:
                assert np.array_equal(s, maps)
            assert np.all((disp == 1) | (disp == 2))
            passes = 2 if loop else 1
            for reset in (False, True):                                # the viewer shows `shown`, on every pass, reset or not
                shows = rgba_delta_ref.replay(d, r, disp, passes, reset)
                for k in range(passes):
                    assert np.array_equal(shows[k * F:(k + 1) * F], s), (trial, k, reset)
            for f in range(F):
                assert c[f] == int(np.sum(d[f] != 0))
                empty = tuple(r[f]) == (0, 0, 0, 0)
                assert not (empty and disp[f] == 2)                    # an empty rectangle only occurs with disposal 1
                assert empty == (c[f] == 0 and disp[f] == 1)
                nxt = f + 1 if f + 1 < F else (0 if loop else None)
                V = delta_ref.rect_of((maps[f] != 0) & (maps[nxt] == 0)) if nxt is not None else (0, 0, 0, 0)
                assert (disp[f] == 2) == (V[2] != 0)
                assert tuple(r[f]) == rgba_delta_ref.union(delta_ref.rect_of(d[f] != 0), V)
                seen_v_only += int(c[f] == 0 and not empty)
            seen_two += int(np.any(disp == 2))
            if kind in (2, 3):                                         # static holes, fully opaque: nothing ever vanishes
                assert np.all(disp == 1)
    assert seen_two > 50 and seen_v_only > 0                           # (a frame whose deltas are all 0 can still have a rectangle)


@pytest.mark.parametrize("tolerance", [0.0, 0.05])
@pytest.mark.parametrize("loop", [False, True])
def test_fully_opaque_maps_are_delta_ref_with_the_index_read_as_0(ob, tolerance, loop):
    size, F, rows = (37, 53), 4, 16
    frames, pal = delta_ref.clip(size[0], size[1], F), _palette(rows, seed=2)
    maps = 1 + delta_ref.maps_of(ob, frames, pal[1:], "ordered")       # row 0 is the transparent entry, which nothing names
    d, s, r, disp, c, gap, tested, kept = rgba_delta_ref.frame_deltas(ob, maps, pal, frames=frames, tolerance=tolerance, loop=loop)
    d_ref, s_ref, r_ref, c_ref, gap_ref, tested_ref, kept_ref = delta_ref.frame_deltas(ob, maps, pal, T=rows, frames=frames, tolerance=tolerance)
    assert np.all(disp == 1)
    assert np.array_equal(d[1:], np.where(d_ref[1:] == rows, 0, d_ref[1:])) and np.array_equal(s, s_ref)
    assert np.array_equal(r[1:], r_ref[1:]) and np.array_equal(c[1:], c_ref[1:])
    assert np.array_equal(d[0], maps[0]) and tuple(r[0]) == (0, 0, size[1], size[0]) and c[0] == size[0] * size[1]
    assert (tested, kept) == (tested_ref, kept_ref) and gap == gap_ref
    assert tolerance == 0 or 0 < kept < tested


@pytest.mark.parametrize("loop", [False, True])
def test_a_case_written_out_by_hand(loop):
    """3 x 3, three frames.  Frame 1 changes the centre only, but its successor makes the top left corner transparent: the rectangle
    grows from the centre to (0, 0, 2, 2) and is disposed to background; frame 2 must draw its three unchanged positions inside that
    rectangle again, while the bottom right corner, outside it, stays on the canvas."""
    maps = np.array([[[1, 1, 0], [1, 2, 0], [0, 0, 3]],
                     [[1, 1, 0], [1, 3, 0], [0, 0, 3]],
                     [[0, 1, 0], [1, 3, 0], [0, 0, 3]]])
    d, s, r, disp, c, *_ = rgba_delta_ref.frame_deltas(None, maps, 4, loop=loop)
    assert d.tolist() == [[[1, 1, 0], [1, 2, 0], [0, 0, 3]],
                          [[0, 0, 0], [0, 3, 0], [0, 0, 0]],
                          [[0, 1, 0], [1, 3, 0], [0, 0, 0]]]
    assert s.tolist() == maps.tolist()
    assert r.tolist() == [[0, 0, 3, 3], [0, 0, 2, 2], [0, 0, 2, 2]]
    assert disp.tolist() == [1, 2, 1]
    assert c.tolist() == [5, 1, 3]
    shows = rgba_delta_ref.replay(d, r, disp, 2)
    assert np.array_equal(shows[:3], maps) and np.array_equal(shows[3:], maps)


def test_pil_shows_the_reference_s_deltas_as_shown(ob):
    """The reference's deltas, compressed by lzw_ref and wrapped by the tests' own container with one disposal per frame: PIL composes
    the frames to palette[shown], transparent where shown is 0 -- at tolerance 0 and in the lossy mode, and on random maps."""
    size, F, rows = (23, 31), 6, 16
    frames, pal = rgba_delta_ref.clip(size[0], size[1], F), _palette(rows, seed=2)
    maps = rgba_delta_ref.maps_of(ob, frames, pal, "ordered")
    cases = [(maps, dict(frames=frames, tolerance=tol)) for tol in (0.0, 0.05)]
    rng = np.random.default_rng(7)
    for trial in range(12):
        cases.append((_random_maps(rng, trial)[1], dict(near=rng.random((6, 11, 11)) < 0.5)))
    for m, kw in cases:
        if "near" in kw:
            kw["near"] = kw["near"][:m.shape[0], :m.shape[1], :m.shape[2]]
        d, s, r, disp, c, *_ = rgba_delta_ref.frame_deltas(ob, m, pal, **kw)
        r1 = r.copy()
        r1[r1[:, 2] == 0] = (0, 0, 1, 1)                               # an empty rectangle: one delta, which is 0
        data, offsets = lzw_ref.encode_frames(d.astype(np.uint8), r1, m=4)
        streams = [bytes(data[offsets[f]:offsets[f + 1]]) for f in range(m.shape[0])]
        blob = rgba_delta_ref.wrap_gif(streams, r1, disp, m.shape[1:], pal, 4)
        head, parsed = lzw_ref.parse_gif(blob)
        assert [fr["disposal"] for fr in parsed] == disp.tolist()
        assert np.array_equal(rgba_delta_ref.replay_parsed(head, parsed, 1), s)
        assert rgba_delta_ref.same_picture(rgba_delta_ref.pil_frames(blob), rgba_delta_ref.rgba_of(pal, s))


def test_arguments_are_checked_before_any_library_call(monkeypatch):
    """Every ValueError of frame_deltas_rgba, and of write_gif's per-frame disposal, is raised before libpatolette_amd.so is asked for
    anything."""
    from patolette_amd import _native

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "lib", no_library)
    maps = np.zeros((2, 4, 5), dtype=np.uint8)
    frames = np.zeros((2, 4, 5, 4), dtype=np.uint8)
    pal = _palette(16, seed=2)
    rgba = np.concatenate([pal, np.full((16, 1), 255, dtype=np.uint8)], axis=1)
    rgba0 = rgba.copy()
    rgba0[0] = 0
    # a palette without a transparent entry points to frame_deltas
    for args in ((pal,), (pal, None, 0.0, True, False, -1), (rgba,), (16, None, 0.0, True, False, -1), (pal.astype(np.float64) / 255.0,)):
        with pytest.raises(ValueError, match="go to frame_deltas"):
            patolette_amd.frame_deltas_rgba(maps, *args)
    with pytest.raises(ValueError, match="contradicts"):
        patolette_amd.frame_deltas_rgba(maps, rgba0, transparent_index=-1)
    with pytest.raises(ValueError, match="transparent_index"):
        patolette_amd.frame_deltas_rgba(maps, pal, transparent_index=3)
    with pytest.raises(ValueError, match="transparent_index"):
        patolette_amd.frame_deltas_rgba(maps, 16, transparent_index=1)
    with pytest.raises(ValueError, match="alpha"):                     # a second transparent row
        patolette_amd.frame_deltas_rgba(maps, np.concatenate([rgba0[:1], rgba0[:1], rgba0[2:]]))
    with pytest.raises(ValueError, match="no opaque row"):
        patolette_amd.frame_deltas_rgba(maps, pal[:1], transparent_index=0)
    with pytest.raises(ValueError, match="palette must be"):
        patolette_amd.frame_deltas_rgba(maps, pal.astype(np.int32), transparent_index=0)
    with pytest.raises(ValueError, match="row count"):
        patolette_amd.frame_deltas_rgba(maps, 0)
    with pytest.raises(ValueError, match="row count"):                 # an int palette with tolerance > 0
        patolette_amd.frame_deltas_rgba(maps, 16, frames=frames, tolerance=0.05)
    for bad in (-0.01, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="tolerance"):
            patolette_amd.frame_deltas_rgba(maps, rgba0, frames=frames, tolerance=bad)
    for bad in (2, -1, "yes", None, 1.0):
        with pytest.raises(ValueError, match="loop"):
            patolette_amd.frame_deltas_rgba(maps, rgba0, loop=bad)
    with pytest.raises(ValueError, match="do not match"):
        patolette_amd.frame_deltas_rgba(maps, rgba0, frames=frames[:, :3], tolerance=0.05)
    with pytest.raises(ValueError, match="do not match"):
        patolette_amd.frame_deltas_rgba(maps, rgba0, frames=frames[:1], tolerance=0.05)
    with pytest.raises(ValueError, match="frames"):
        patolette_amd.frame_deltas_rgba(maps, rgba0, frames=frames[0], tolerance=0.05)
    with pytest.raises(ValueError, match="frames"):                    # the lossy mode without pixels
        patolette_amd.frame_deltas_rgba(maps, rgba0, tolerance=0.05)
    with pytest.raises(ValueError, match="maps must be"):
        patolette_amd.frame_deltas_rgba(maps.astype(np.int64), 16)
    with pytest.raises(ValueError, match="maps must be"):
        patolette_amd.frame_deltas_rgba(maps[0], 16)
    # write_gif: one disposal per frame
    for bad in ([1], [1, 2, 1], [1, 4], [1, -1], [1.0, 2.0], [True, False], np.array([[1, 2]]), (1, None), np.array(1)):
        with pytest.raises(ValueError, match="disposal"):
            patolette_amd.write_gif(None, maps, pal, disposal=bad)
    for bad in (4, -1, True, 1.0, None, "1"):                          # a scalar as before
        with pytest.raises(ValueError, match="disposal must be 0, 1, 2 or 3$"):
            patolette_amd.write_gif(None, maps, pal, disposal=bad)
    assert "frame_deltas_rgba" in patolette_amd.__all__


def test_write_gif_reaches_the_library_with_a_disposal_per_frame(monkeypatch):
    """A valid sequence (list, tuple, int32 array as frame_deltas_rgba returns it) passes every check: the next thing write_gif does is
    to ask the library for the streams."""
    from patolette_amd import _native

    class Reached(Exception):
        pass

    def the_library():
        raise Reached()
    monkeypatch.setattr(_native, "lib", the_library)
    maps = np.zeros((2, 4, 5), dtype=np.uint8)
    for good in ([1, 2], (0, 3), np.array([2, 1], dtype=np.int32), 1, np.int64(2)):
        with pytest.raises(Reached):
            patolette_amd.write_gif(None, maps, _palette(16, seed=2), transparent_index=0, disposal=good)
