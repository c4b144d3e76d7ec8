"""tests/local_delta_ref.py, the reference of frame_deltas_local, against tests/delta_ref.py where the two must agree; the argument
checks `frame_deltas_local` and `write_gif` make before they cross into C; and `write_gif`'s local colour tables with `gif_lzw`
replaced by a stand-in on tests/lzw_ref.py's encoder, read back by local_delta_ref's parser and compositor and by PIL.  No GPU."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import delta_ref, local_delta_ref, lzw_ref
from tests.test_gpu_remap import _palette

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _case(size, F, rows, kind):
    from oracle import binding as ob
    frames, pal = delta_ref.clip(size[0], size[1], F), _palette(rows, seed=2)
    maps = delta_ref.maps_of(ob, frames, pal, kind)
    for a in (frames, pal, maps):
        a.setflags(write=False)
    return frames, pal, maps


@pytest.mark.parametrize("tolerance", [0.0, 0.02, 0.05])
@pytest.mark.parametrize("rows", [2, 16, 255])
@pytest.mark.parametrize("size,F", [((40, 56), 5), ((37, 53), 4)])
def test_one_table_or_identical_tables_give_the_plain_deltas(ob, size, F, rows, tolerance):
    """Consequence (c), distinct rows: P == 1 with every frame on table 0, and F copies of the table with palette_of None."""
    frames, pal, maps = _case(size, F, rows, "nearest")
    d, s, r, c, gap, tested, kept = delta_ref.frame_deltas(ob, maps, pal, frames=frames, tolerance=tolerance)
    for palettes, of in ((pal[None], [0] * F), (np.stack([pal] * F), None), (np.stack([pal] * 2), [f % 2 for f in range(F)])):
        dl, sl, rl, cl, gapl, testedl, keptl = local_delta_ref.frame_deltas(ob, maps, palettes, of, frames=frames, tolerance=tolerance)
        assert np.array_equal(dl, d) and np.array_equal(rl, r) and np.array_equal(cl, c)
        assert np.array_equal(sl, pal[s])
        assert (gapl, testedl, keptl) == (gap, tested, kept)
        assert np.array_equal(local_delta_ref.replay_rgb(dl, palettes, of, rows), sl)           # consequence (a)
        if tolerance == 0:
            assert np.array_equal(sl, pal[maps])                                                # consequence (b)


def test_tables_that_differ(ob):
    """Two scenes, two tables: (a), (b) and (d); a row shared byte for byte between the tables keeps across them."""
    size, F = (40, 56), 6
    frames = delta_ref.clip(size[0], size[1], F)
    palettes = np.stack([_palette(16, seed=2), _palette(16, seed=3)])
    palettes[1, 5] = palettes[0, 9]
    of = [0, 0, 0, 1, 1, 1]
    maps = np.stack([delta_ref.maps_of(ob, frames[f:f + 1], palettes[of[f]], "nearest")[0] for f in range(F)])
    maps[2, :4, :4], maps[3, :4, :4] = 9, 5                              # the shared colour, under both tables
    for tolerance in (0.0, 0.05):
        d, s, r, c, gap, tested, kept = local_delta_ref.frame_deltas(ob, maps, palettes, of, frames=frames, tolerance=tolerance)
        assert np.array_equal(local_delta_ref.replay_rgb(d, palettes, of, 16), s)
        own = np.stack([palettes[of[f]][maps[f]] for f in range(F)])
        if tolerance == 0:
            assert np.all(d[3, :4, :4] == 16)                           # kept across the tables
            assert np.array_equal(s, own)
            assert c[3] > 0.9 * size[0] * size[1]                        # the other table: nearly everything is drawn again
        else:
            held = np.any(s != own, axis=-1)
            assert np.any(held) and 0 < kept < tested
            for f in range(F):                                          # (d): within the tolerance of that frame's source
                px = frames[f][held[f]].astype(np.float64) / 255.0
                sh = s[f][held[f]].astype(np.float64) / 255.0
                dd = ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(px)), px.shape[0]) - \
                    ob.unplanar(ob.convert("srgb_to_ictcp", ob.planar(sh)), sh.shape[0])
                assert np.all((dd * dd).sum(axis=1) <= 0.05 * 0.05 * (1 + 1e-12))
        for f in range(F):
            assert tuple(r[f]) == delta_ref.rect_of(d[f] != 16) or f == 0


def test_duplicate_rows_by_hand():
    """Consequence (c) with duplicate rows, every value stated: 2 frames of 2 x 3, one table of 3 rows whose rows 0 and 2 are equal."""
    pal = np.array([[10, 20, 30], [200, 100, 0], [10, 20, 30]], dtype=np.uint8)
    maps = np.array([[[0, 1, 2], [0, 1, 2]],
                     [[2, 1, 0], [1, 0, 2]]], dtype=np.uint8)
    T = 3
    d, s, r, c, *_ = local_delta_ref.frame_deltas(None, maps, pal[None], [0, 0])
    assert d[1].tolist() == [[T, T, T], [1, 0, T]]                       # 0 <-> 2 is the same colour: kept
    assert r.tolist() == [[0, 0, 3, 2], [0, 1, 2, 1]] and c.tolist() == [6, 2]
    assert np.array_equal(s[1], pal[maps[1]])
    dp, sp, rp, cp, *_ = delta_ref.frame_deltas(None, maps, 3)
    assert dp[1].tolist() == [[2, T, 0], [1, 0, T]]                      # the plain deltas compare indices: drawn
    assert rp.tolist() == [[0, 0, 3, 2], [0, 0, 3, 2]] and cp.tolist() == [6, 4]
    assert np.array_equal(pal[sp], s)                                   # both show the same colours


def _no_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "lib", no_library)


def test_frame_deltas_local_checks_its_arguments_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    f = patolette_amd.frame_deltas_local
    maps = np.zeros((2, 4, 5), dtype=np.uint8)
    frames = np.zeros((2, 4, 5, 3), dtype=np.uint8)
    pals = np.zeros((2, 16, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="maps must be"):
        f(maps[0], pals)
    with pytest.raises(ValueError, match="maps must be"):
        f(maps.astype(np.int64), pals)
    with pytest.raises(ValueError, match="maps must be uint8"):
        f(maps.astype(np.uint16), pals)
    for bad in (-0.01, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="tolerance"):
            f(maps, pals, frames=frames, tolerance=bad)
    for bad in (pals[0], pals.astype(np.float64), np.zeros((2, 16, 4), dtype=np.uint8), np.zeros((0, 16, 3), dtype=np.uint8),
                np.zeros((2, 0, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match=r"\(P, K, 3\)"):
            f(maps, bad)
    with pytest.raises(ValueError, match="at most 255 rows"):
        f(maps, np.zeros((2, 256, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="do not match 2 frames"):       # palette_of None with P != F
        f(maps, np.zeros((3, 16, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="palette_of must be"):          # wrong length, wrong dtype
        f(maps, pals, palette_of=[0, 1, 1])
    with pytest.raises(ValueError, match="palette_of must be"):
        f(maps, pals, palette_of=np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="palette_of value"):
        f(maps, pals, palette_of=[0, 2])
    with pytest.raises(ValueError, match="palette_of value"):
        f(maps, pals, palette_of=[-1, 0])
    for bad in (15, 256, -1):
        with pytest.raises(ValueError, match="transparent_index"):
            f(maps, pals, transparent_index=bad)
    with pytest.raises(ValueError, match="transparent_index"):
        f(maps, pals, transparent_index=16.0)
    with pytest.raises(ValueError, match="do not match"):
        f(maps, pals, frames=frames[:, :3], tolerance=0.05)
    with pytest.raises(ValueError, match="frames"):
        f(maps, pals, frames=frames[0], tolerance=0.05)
    with pytest.raises(ValueError, match="frames"):                      # the lossy mode without pixels
        f(maps, pals, tolerance=0.05)
    with pytest.raises(AssertionError, match="the library was called"):  # (and good arguments do reach it)
        f(maps, pals, palette_of=[1, 0], transparent_index=255, frames=frames, tolerance=0.05, want_shown=True)


def test_write_gif_checks_its_new_arguments_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    w = patolette_amd.write_gif
    maps = np.zeros((2, 4, 5), dtype=np.uint8)
    pals = np.zeros((2, 16, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="palette_u8 must be"):          # a wrong ndim
        w(None, maps, np.zeros((2, 2, 16, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="palette_u8 must be"):
        w(None, maps, np.zeros(48, dtype=np.uint8))
    with pytest.raises(ValueError, match=r"\(P, K, 3\)"):
        w(None, maps, pals.astype(np.float64))
    with pytest.raises(ValueError, match="at most 256 rows"):
        w(None, maps, np.zeros((2, 257, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="palette_of must be"):
        w(None, maps, pals, palette_of=[0])
    with pytest.raises(ValueError, match="palette_of must be"):
        w(None, maps, pals, palette_of=np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="palette_of value"):
        w(None, maps, pals, palette_of=[0, 2])
    with pytest.raises(ValueError, match="do not match 2 frames"):
        w(None, maps, np.zeros((3, 16, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="palette_of needs"):
        w(None, maps, pals[0], palette_of=[0, 0])
    for bad in (np.zeros((256, 16), dtype=np.uint8), np.zeros((3, 256, 16), dtype=np.uint8), np.zeros((2, 256, 15), dtype=np.uint8),
                np.zeros((2, 256, 16), dtype=np.int32)):
        with pytest.raises(ValueError, match=r"\(P, 256, 16\)"):
            w(None, maps, pals, near=bad)
    with pytest.raises(AssertionError, match="the library was called"):
        w(None, maps, pals, palette_of=[1, 0], near=np.zeros((2, 256, 16), dtype=np.uint8))


@pytest.fixture
def standin(monkeypatch):
    """`gif_lzw` by tests/lzw_ref.py's encoder."""
    calls = []

    def fake(maps, rects=None, min_code_size=8, segment=None):
        calls.append((np.asarray(maps).shape, min_code_size))
        data, offsets = lzw_ref.encode_frames(np.asarray(maps), rects, min_code_size, segment or lzw_ref.DEFAULT_SEGMENT)
        return (True, data, offsets, "")

    monkeypatch.setattr(patolette_amd, "gif_lzw", fake)
    return calls


def _two_scenes(ob, size=(40, 56), K=16, T=None):
    frames = np.concatenate([delta_ref.clip(size[0], size[1], 3, seed=5), 255 - delta_ref.clip(size[0], size[1], 3, seed=7)])
    palettes = np.stack([_palette(K, seed=2), _palette(K, seed=3)])
    of = [0, 0, 0, 1, 1, 1]
    maps = np.stack([delta_ref.maps_of(ob, frames[f:f + 1], palettes[of[f]], "nearest")[0] for f in range(6)]).astype(np.uint8)
    return frames, palettes, of, maps


@pytest.mark.parametrize("K,T,bits", [(16, 16, 5), (15, 15, 4), (3, 3, 2), (2, 255, 8)])
def test_write_gif_local_tables(ob, standin, tmp_path, K, T, bits):
    frames, palettes, of, maps = _two_scenes(ob, K=K)
    d, s, r, c, *_ = local_delta_ref.frame_deltas(ob, maps, palettes, of, T=T)
    d = d.astype(np.uint8)
    for order in (of, [1, 1, 1, 0, 0, 1]):                              # (the second: the global table is table 1, frame 5 returns to it)
        if order is not of:
            d, s, r, c, *_ = local_delta_ref.frame_deltas(ob, maps, palettes, order, T=T)
            d = d.astype(np.uint8)
        path = tmp_path / "local.gif"
        blob = patolette_amd.write_gif(path, d, palettes, r, transparent_index=T, palette_of=order)
        assert path.read_bytes() == blob and len(standin) >= 1 and standin[-1] == ((6, 40, 56), max(2, bits))
        head, parsed = local_delta_ref.parse_gif(blob)
        padded = np.zeros((2, 1 << bits, 3), dtype=np.uint8)
        padded[:, :K] = palettes
        assert blob[10] == 0x80 | 7 << 4 | (bits - 1) and np.array_equal(head["table"], padded[order[0]])
        for f, fr in enumerate(parsed):
            assert fr["m"] == max(2, bits) and fr["transparent"] == T and fr["disposal"] == 1 and fr["rect"] == tuple(int(v) for v in r[f])
            if order[f] == order[0]:
                assert fr["table"] is None and fr["packed"] == 0
            else:
                assert fr["packed"] == 0x80 | (bits - 1) and np.array_equal(fr["table"], padded[order[f]])
        assert np.array_equal(local_delta_ref.composite_rgb(head, parsed), s)
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(io.BytesIO(blob))
        assert im.n_frames == 6
        for f in range(6):
            im.seek(f)
            assert np.array_equal(np.asarray(im.convert("RGB")), s[f]), f


def test_write_gif_with_a_2d_palette_writes_what_it_wrote(ob, standin):
    frames, palettes, of, maps = _two_scenes(ob)
    d, _, r, _, *_ = delta_ref.frame_deltas(ob, maps[:3], palettes[0])
    d = d.astype(np.uint8)
    blob = patolette_amd.write_gif(None, d, palettes[0], r, transparent_index=16)
    data, offsets = lzw_ref.encode_frames(d, r, 5)
    table = np.zeros((32, 3), dtype=np.uint8)
    table[:16] = palettes[0]
    streams = [bytes(data[offsets[f]:offsets[f + 1]]) for f in range(3)]
    assert blob == lzw_ref.wrap_gif(streams, r, (40, 56), table, 5, transparent_index=16)
    head, parsed = lzw_ref.parse_gif(blob)                              # the reader that refuses local tables reads it
    assert len(parsed) == 3
    # one table for every frame, given as a stack: the same bytes
    assert patolette_amd.write_gif(None, d, palettes[:1], r, transparent_index=16, palette_of=[0, 0, 0]) == blob
    assert patolette_amd.write_gif(None, d, np.stack([palettes[0]] * 3), r, transparent_index=16) != blob    # (equal tables are still written)


def test_write_gif_near_runs_once_per_table_in_use(ob, monkeypatch):
    frames, palettes, of, maps = _two_scenes(ob)
    d, s, r, c, *_ = local_delta_ref.frame_deltas(ob, maps, palettes, of, T=16)
    d = d.astype(np.uint8)
    calls = []

    def fake(maps, near, rects=None, min_code_size=8, segment=None, want_coded=False):
        calls.append((np.asarray(maps).copy(), near.copy(), np.asarray(rects).copy()))
        data, offsets = lzw_ref.encode_frames(np.asarray(maps), rects, min_code_size, segment or lzw_ref.DEFAULT_SEGMENT)
        return (True, data, offsets, None, "")

    monkeypatch.setattr(patolette_amd, "gif_lzw_lossy", fake)
    near = np.zeros((3, 256, 16), dtype=np.uint8)
    near[0, 1, :2], near[2, 1, :2] = (1, 2), (1, 3)
    order = [2, 0, 2, 0, 0, 2]
    pal3 = np.stack([palettes[0], palettes[1], palettes[1]])
    blob = patolette_amd.write_gif(None, d, pal3, r, transparent_index=16, near=near, palette_of=order)
    assert len(calls) == 2                                              # tables 0 and 2; table 1 is not in use
    assert np.array_equal(calls[0][0], d[[1, 3, 4]]) and np.array_equal(calls[0][1], near[0]) and np.array_equal(calls[0][2], r[[1, 3, 4]])
    assert np.array_equal(calls[1][0], d[[0, 2, 5]]) and np.array_equal(calls[1][1], near[2]) and np.array_equal(calls[1][2], r[[0, 2, 5]])
    head, parsed = local_delta_ref.parse_gif(blob)
    for f, fr in enumerate(parsed):                                      # the streams are back in frame order
        x0, y0, w, h = fr["rect"]
        assert lzw_ref.decode(fr["stream"], fr["m"], w * h) == d[f, y0:y0 + h, x0:x0 + w].reshape(-1).tolist()


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(HERE, "..", "include", "patolette_amd.h")).read()
    for name in ("patolette_amd_frame_deltas_local", "patolette_amd_frame_deltas_local_device"):
        assert "void %s(" % name in header and name in _native.SYMBOLS
        restype, argtypes = _native.SYMBOLS[name]
        assert restype is None and len(argtypes) == 17 and argtypes[-1] == C.POINTER(C.c_int) and argtypes[7] == C.POINTER(C.c_int32)
    for name in ("patolette_amd_debug_delta_local_tables", "patolette_amd_debug_delta_local_route"):
        assert "int %s(" % name in header and name in _native.SYMBOLS
    assert "frame_deltas_local" in patolette_amd.__all__ and callable(patolette_amd.frame_deltas_local)
    import inspect
    assert "palette_of" in inspect.signature(patolette_amd.write_gif).parameters
    assert "k_frame_deltas_local" in open(os.path.join(HERE, "..", "patolette_amd", "csrc", "delta.hip")).read()
