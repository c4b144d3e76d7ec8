"""frame_deltas_rgba / patolette_amd_frame_deltas_rgba on the device against tests/rgba_delta_ref.py (numpy on the CPU oracle).

Every comparison with the reference is bit for bit over all elements of deltas, shown, rects, disposals and changed.  The device's pow
is within 0.52 ulp of glibc's, not equal to it, so, as in tests/test_gpu_delta.py, every lossy case first asserts that the REFERENCE's
smallest relative gap |D - tol^2| / tol^2 over every distance it evaluated is at least 1e-9, and that both outcomes (kept, not kept)
occur.  If another input trips that, change the seed, not the bar.  (A palette of 2 rows has one opaque row: no two opaque entries
ever differ, the lossy mode evaluates no distance there, and the case says so instead.  The same holds for the clip whose disc moves
in EVERY frame: some pixel vanishes in every frame, so every frame is cleared over all it drew and the next one meets an empty canvas
-- rgba_delta_ref.clip has the argument.  That clip is compared bit for bit in every mode; the lossy sweeps use the clip whose disc
rests every second frame, and the other contents.)

The input maps are made on the CPU: the reference's own ordered / nearest maps of the RGBA clip, or maps built by hand from them.
Sizes: (1, 1); (5, 3); (37, 53), whose 1961 positions are no multiple of 64; (64, 64) and (120, 64), multiples of 4 where a lane can own
four positions; (263, 301), several blocks with rows that wrap inside a wavefront; (36, 301), a multiple of 4 with an odd width, so that
a lane's four positions wrap a row."""
import ctypes as C
import functools

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import delta_ref, lzw_ref, rgba_delta_ref
from tests.test_gpu_remap import _image, _palette
from tests.util import ROOT

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-9
PREFIX = "patolette_amd_frame_deltas_rgba:"
SIZES = {"one": ((1, 1), 3), "tiny": ((5, 3), 4), "odd64": ((37, 53), 8), "square": ((64, 64), 3), "wide": ((120, 64), 6),
         "wrap": ((263, 301), 2), "quadwrap": ((36, 301), 3), "single": ((37, 53), 1)}
# the lossy sweep: the disc rests every second frame, and three frames make it both rest and move
LOSSY_SIZES = {"square": ((64, 64), 3), "wide": ((120, 64), 6), "wrap": ((263, 301), 3), "quadwrap": ((36, 301), 3)}
CONTENTS = ["disc", "rest", "transparent", "opaque", "holes", "corners", "far", "still"]


@pytest.fixture(autouse=True)
def _defaults_again(gpu):
    yield
    _native.profile(False)
    gpu.patolette_amd_debug_delta_quad(-1)


def _dtype(rows):
    return np.uint8 if rows <= 256 else np.uint16


@functools.lru_cache(maxsize=None)
def _clip(size, F, rest=1):
    frames = rgba_delta_ref.clip(size[0], size[1], F, rest=rest)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _case(size, F, rows, content="disc", kind="ordered"):
    """(frames (F, H, W, 4) uint8, palette (rows, 3) uint8 whose row 0 is the transparent entry, maps in the numpy flavour's element
    type), computed once.  "disc": the clip, whose disc moves in every frame; "rest": its disc moves in every second frame only (see
    rgba_delta_ref.clip: a sprite that moves in every frame is drawn whole every time, and the lossy mode then has nothing to compare).
    The other contents are built from the fully opaque maps of the clip's RGB:
      transparent  every element 0;
      opaque       no element 0;
      holes        a static pattern of holes: nothing ever vanishes, every disposal is 1;
      corners      the four corner pixels are opaque in every frame but the last, so they vanish there and the rectangle of the frame
                   before reaches every edge;
      far          frames 0 and 1 show the same pixels and maps but for one changed element near the top left; in frame 2 one pixel near
                   the bottom right vanishes: V alone extends frame 1's rectangle, and what lies in it is drawn again;
      still        frame 1 is frame 0 again, and frame 2 has a hole: frame 1 has changed == 0 and a rectangle."""
    from oracle import binding as ob
    h, w = size
    pal = _palette(rows, seed=2)
    frames = _clip(size, F, 2 if content == "rest" else 1)
    if content in ("disc", "rest"):
        maps = rgba_delta_ref.maps_of(ob, frames, pal, kind)
    else:
        frames = frames.copy()
        frames[..., 3] = 255
        if content in ("far", "still"):
            assert F >= 3
            frames[1] = frames[0]
        maps = 1 + delta_ref.maps_of(ob, frames[..., :3], pal[1:], kind)
        if content == "transparent":
            maps[:] = 0
        elif content == "holes":
            maps[:, np.random.default_rng(11).random((h, w)) < 0.3] = 0
        elif content == "corners":
            for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
                maps[-1, y, x] = 0
        elif content == "far":
            maps[1, 1, 2] = 1 + maps[0, 1, 2] % (rows - 1)
            maps[2:, h - 2, w - 3] = 0
        elif content == "still":
            maps[2:, h // 2:h // 2 + 3, w // 2:w // 2 + 2] = 0
        else:
            assert content == "opaque"
    maps = maps.astype(_dtype(rows))
    for a in (frames, pal, maps):
        a.setflags(write=False)
    return frames, pal, maps


@functools.lru_cache(maxsize=None)
def _reference(size, F, rows, content, kind, tolerance, loop):
    """The reference's (deltas, shown, rects, disposals, changed, tested, kept) of _case(...), computed once.  Lossy: the gap condition
    and "both outcomes occur" are asserted here, before anything runs on the device."""
    from oracle import binding as ob
    frames, pal, maps = _case(size, F, rows, content, kind)
    d, s, r, disp, c, gap, tested, kept = rgba_delta_ref.frame_deltas(ob, maps, pal, frames=frames, tolerance=tolerance, loop=loop)
    print("rgba delta reference: %s F %d rows %d %s %s tolerance %g loop %d: %d distances, %d kept, smallest relative gap %.3g; disposals %s"
          % (size, F, rows, content, kind, tolerance, loop, tested, kept, gap, disp.tolist()))
    if tolerance > 0 and tested > 0:
        assert gap >= MIN_GAP
    for a in (d, s, r, disp, c):
        a.setflags(write=False)
    return d, s, r, disp, c, tested, kept


def _same(got, ref):
    """got: (deltas, rects, disposals, changed, shown) of the device; ref: the reference's (deltas, shown, rects, disposals, changed, ..)."""
    d, r, disp, c, s = got
    pairs = ((d, ref[0]), (s, ref[1]), (r, ref[2]), (disp, ref[3]), (c, ref[4]))
    wrong = [int(np.sum(np.asarray(a).astype(np.int64) != b)) for a, b in pairs]
    print("deltas / shown / rects / disposals / changed: %s of %s differ from the reference" % (wrong, [b.size for _, b in pairs]))
    assert all(np.asarray(a).shape == b.shape for a, b in pairs)
    assert wrong == [0, 0, 0, 0, 0]
    assert r.dtype == np.int32 and disp.dtype == np.int32 and c.dtype == np.int64


def _quads(size):
    """The lane forms to force: the launcher's rule, one position per lane, and four where the frame allows it."""
    return (-1, 0, 1) if size[0] * size[1] % 4 == 0 else (-1, 0)


def _run_and_compare(gpu, maps, pal, frames, tolerance, loop, ref, size):
    for quad in _quads(size):
        gpu.patolette_amd_debug_delta_quad(quad)
        ok, d, r, disp, c, s, msg = patolette_amd.frame_deltas_rgba(maps, pal, frames=frames, tolerance=tolerance, loop=loop, want_shown=True,
                                                                    transparent_index=0)
        assert ok, msg
        assert d.dtype == maps.dtype and s.dtype == maps.dtype
        _same((d, r, disp, c, s), ref)
        passes = 2 if loop else 1
        assert np.array_equal(rgba_delta_ref.replay(d, r, disp, passes), np.concatenate([s] * passes))
    return d, r, disp, c, s


# ---- the exact mode on random maps: every size, both loops, every lane form; no colour is read -------------------------------

@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("name", list(SIZES))
def test_exact_on_random_maps(gpu, name, loop):
    size, F = SIZES[name]
    h, w = size
    rng = np.random.default_rng(h * 1000 + w + F)
    for kind in ("sprite", "holes", "opaque"):
        maps = rng.integers(1, 7, size=(F, h, w)).astype(np.uint8)
        if kind == "sprite":                                          # a block that moves by (2, 3) and wraps, transparent around it
            keep = np.zeros((F, h, w), dtype=bool)
            for f in range(F):
                ys, xs = (np.arange(max(1, h // 2)) + 2 * f) % h, (np.arange(max(1, w // 2)) + 3 * f) % w
                keep[f][np.ix_(ys, xs)] = True
            maps[~keep] = 0
        elif kind == "holes":
            maps[rng.random((F, h, w)) < 0.3] = 0
        ref = rgba_delta_ref.frame_deltas(None, maps, 7, loop=loop)
        ref = ref[:5] + ref[6:]
        d, r, disp, c, s = _run_and_compare(gpu, maps, 7, None, 0.0, loop, ref, size)
        assert np.array_equal(s, maps)
        if kind == "opaque":
            assert np.all(disp == 1)
        elif F > 1 and h * w > 1:
            assert np.any(disp == 2)
    if name == "one":                                                 # (1, 1): opaque, gone, opaque again
        maps = np.array([[[3]], [[0]], [[5]]], dtype=np.uint8)
        ok, d, r, disp, c, s, msg = patolette_amd.frame_deltas_rgba(maps, 7, loop=loop, want_shown=True)
        assert ok, msg
        assert d.ravel().tolist() == [3, 0, 5] and disp.tolist() == [2, 1, 1] and c.tolist() == [1, 0, 1]
        assert r.tolist() == [[0, 0, 1, 1], [0, 0, 0, 0], [0, 0, 1, 1]]


@pytest.mark.parametrize("size", [(1024, 2048), (2048, 2052)])
def test_where_a_block_walks_several_tiles(gpu, size):
    """A frame's launch has at most 8 blocks per CU (2048 on an MI355X), each walking its tiles: 2^21 positions are 8192 tiles with one
    position per lane, 2048 x 2052 are 4104 tiles with four -- and from 2^21 positions on the launcher's own rule takes four.  The exact
    mode on random maps with a hole that moves and a block of changes, every lane form."""
    h, w = size
    rng = np.random.default_rng(3)
    first = rng.integers(1, 16, size=size, dtype=np.uint8)
    maps = np.stack([first, np.where(rng.random(size) < 0.1, rng.integers(1, 16, size=size, dtype=np.uint8), first)])
    maps[0, 100:300, 200:900] = 0
    maps[1, 150:350, 300:1000] = 0
    maps[0, h - 1, w - 1] = 0
    ref = rgba_delta_ref.frame_deltas(None, maps, 16)
    assert ref[3].tolist() == [2, 2]
    for quad in (-1, 0, 1):
        gpu.patolette_amd_debug_delta_quad(quad)
        ok, d, r, disp, c, s, msg = patolette_amd.frame_deltas_rgba(maps, 16, want_shown=True)
        assert ok, msg
        _same((d, r, disp, c, s), ref)


# ---- contents, sizes, palettes and tolerances against the CPU oracle ---------------------------------------------------------

@pytest.mark.parametrize("tolerance", [0.0, 0.02, 0.05])
@pytest.mark.parametrize("content", CONTENTS)
def test_contents(gpu, content, tolerance):
    size, F = SIZES["odd64"]
    rows, loop = 16, content != "far"
    frames, pal, maps = _case(size, F, rows, content)
    ref = _reference(size, F, rows, content, "ordered", tolerance, loop)
    if tolerance > 0 and content not in ("transparent", "disc"):      # ("disc": every frame meets an empty canvas -- rgba_delta_ref.clip)
        assert 0 < ref[6] < ref[5]                                    # both outcomes occur
    d, r, disp, c, s = _run_and_compare(gpu, maps, pal, frames, tolerance, loop, ref, size)
    h, w = size
    assert np.array_equal(s != 0, maps != 0)
    if tolerance == 0:
        assert np.array_equal(s, maps)
    if content in ("disc", "rest"):
        assert np.any(disp == 2)
    if content == "transparent":
        assert not d.any() and not r.any() and not c.any() and np.all(disp == 1)
    if content in ("opaque", "holes"):
        assert np.all(disp == 1)
    if content == "corners":                                          # (frame 0 is opaque where the last frame is: the loop clears nothing)
        assert disp.tolist() == [1] * (F - 2) + [2, 1] and r[F - 2].tolist() == [0, 0, w, h]
    if content == "far":
        assert disp[1] == 2 and c[1] <= 1 and r[1, 0] + r[1, 2] == w - 2 and r[1, 1] + r[1, 3] == h - 1
    if content == "far" and tolerance == 0:
        # frame 1: one changed element at (2, 1); the vanish at (w - 3, h - 2) extends the rectangle; frame 2 draws it again
        assert c[1] == 1 and r[1].tolist() == [2, 1, w - 4, h - 2]
        assert c[2] >= (w - 4) * (h - 2) - 1 and np.all(d[2, 1:h - 1, 2:w - 2][maps[2, 1:h - 1, 2:w - 2] != 0] != 0)
    if content == "still":
        assert c[1] == 0 and not d[1].any() and disp[1] == 2 and r[1].tolist() == [w // 2, h // 2, 2, 3]


@pytest.mark.parametrize("tolerance", [0.02, 0.05])
@pytest.mark.parametrize("rows", [16, 300])
@pytest.mark.parametrize("name", ["square", "wide", "wrap", "quadwrap"])
def test_sizes_and_rows_lossy(gpu, name, rows, tolerance):
    size, F = LOSSY_SIZES[name]
    kind = "nearest" if name == "wide" and rows == 300 else "ordered"
    frames, pal, maps = _case(size, F, rows, "rest", kind)
    for loop in (True, False):
        ref = _reference(size, F, rows, "rest", kind, tolerance, loop)
        assert 0 < ref[6] < ref[5]                                    # both outcomes occur
        for m in (maps,) if rows <= 256 else (maps, maps.astype(np.uint32)):
            _run_and_compare(gpu, m, pal, frames, tolerance, loop, ref, size)


def test_two_rows(gpu):
    """One opaque row: no two opaque entries differ, so the lossy mode evaluates no distance and equals the exact one."""
    size, F = SIZES["odd64"]
    frames, pal, maps = _case(size, F, 2)
    exact = _reference(size, F, 2, "disc", "ordered", 0.0, True)
    lossy = _reference(size, F, 2, "disc", "ordered", 0.05, True)
    assert lossy[5] == 0 and all(np.array_equal(a, b) for a, b in zip(exact[:5], lossy[:5]))
    for tolerance in (0.0, 0.05):
        _run_and_compare(gpu, maps, pal, frames, tolerance, True, exact, size)
    assert np.any(exact[3] == 2)


@functools.lru_cache(maxsize=None)
def _all_indices(size, F, rows, seed):
    """Maps that use every index below `rows`, with moving transparency, and pixels that make both outcomes of the lossy test occur:
    every opaque pixel shows, give or take one code value, the colour of its own entry or of the entry its predecessor had."""
    h, w = size
    rng = np.random.default_rng(seed)
    pal = _palette(rows, seed=2)
    maps = rng.integers(1, rows, size=(F, h, w))
    for f in range(F):                                                # a hole of (h // 3, w // 3) that moves by (2, 3) every second frame
        y, x = (5 + 2 * (f // 2)) % h, (3 * (f // 2)) % w
        maps[f, y:y + h // 3, x:x + w // 3] = 0
    if h * w >= 2 * rows:
        maps.reshape(F, -1)[:, -rows:] = np.arange(rows)              # every index, in every frame
    own = rng.random((F, h, w)) < 0.5
    shows = np.where(own, maps, np.concatenate([maps[:1], maps[:-1]]))
    px = np.clip(pal[shows].astype(np.int64) + rng.integers(-1, 2, size=(F, h, w, 3)), 0, 255).astype(np.uint8)
    frames = np.concatenate([px, np.where(maps[..., None] != 0, 255, 0).astype(np.uint8)], axis=-1)
    maps = maps.astype(_dtype(rows))
    for a in (frames, pal, maps):
        a.setflags(write=False)
    return frames, pal, maps


@pytest.mark.parametrize("tolerance", [0.0, 0.02, 0.05])
def test_256_rows_in_a_byte(gpu, tolerance):
    """A one-byte map that uses all 256 indices: 0 is both the transparent entry and the deltas' "leave the canvas"."""
    from oracle import binding as ob
    size, F = SIZES["square"]
    frames, pal, maps = _all_indices(size, F, 256, 3)
    assert maps.dtype == np.uint8 and np.unique(maps).size == 256
    ref = rgba_delta_ref.frame_deltas(ob, maps, pal, frames=frames, tolerance=tolerance)
    if tolerance > 0:
        print("256 rows, tolerance %g: %d distances, %d kept, smallest relative gap %.3g" % (tolerance, ref[6], ref[7], ref[5]))
        assert ref[5] >= MIN_GAP and 0 < ref[7] < ref[6]
    d, r, disp, c, s = _run_and_compare(gpu, maps, pal, frames, tolerance, True, ref[:5] + ref[6:], size)
    assert np.any(d == 255) and np.any(disp == 2)


@pytest.mark.parametrize("tolerance", [0.0, 0.05])
def test_a_palette_beyond_the_rows_held_in_lds(gpu, tolerance):
    """1100 rows: the palette is indexed in global memory.  (5, 3), and (37, 53) for more than a handful of distances."""
    from oracle import binding as ob
    for name in ("tiny", "odd64"):
        size, F = SIZES[name]
        frames, pal, maps = _all_indices(size, F, 1100, 4)
        assert maps.dtype == np.uint16 and (name == "tiny" or maps.max() >= 1024)
        ref = rgba_delta_ref.frame_deltas(ob, maps, pal, frames=frames, tolerance=tolerance)
        if tolerance > 0:
            print("1100 rows %s: %d distances, %d kept, smallest relative gap %.3g" % (size, ref[6], ref[7], ref[5]))
            assert ref[5] >= MIN_GAP and 0 < ref[7] < ref[6]
        _run_and_compare(gpu, maps, pal, frames, tolerance, True, ref[:5] + ref[6:], size)


def test_palette_forms(gpu):
    size, F = SIZES["odd64"]
    frames, pal, maps = _case(size, F, 16, "rest")
    ref = _reference(size, F, 16, "rest", "ordered", 0.05, True)
    palf = pal.astype(np.float64) / 255.0
    rgba = np.concatenate([pal, np.full((16, 1), 255, dtype=np.uint8)], axis=1)
    rgba[0] = 0
    padded = np.concatenate([rgba, np.zeros((4, 4), dtype=np.uint8)])                     # trailing unused rows, as quantize_rgba fills them
    filled = np.full((20, 3), -1.0)                                                       # ... and as the f64 palettes do
    filled[:16] = palf
    other0 = palf.copy()
    other0[0] = (np.nan, -np.inf, 7.0)                                                    # row 0's colour is never read
    for form, tidx in ((pal, 0), (np.ascontiguousarray(palf), 0), (np.asfortranarray(palf), 0), (rgba, None), (rgba, 0), (padded, None),
                       (filled, 0), (np.asfortranarray(filled), 0), (other0, 0)):
        ok, d, r, disp, c, s, msg = patolette_amd.frame_deltas_rgba(maps, form, frames=frames, tolerance=0.05, want_shown=True,
                                                                    transparent_index=tidx)
        assert ok, msg
        _same((d, r, disp, c, s), ref)
    ok, d, r, disp, c, s, msg = patolette_amd.frame_deltas_rgba(maps, pal, frames=frames[..., :3], tolerance=0.05, want_shown=True,
                                                                transparent_index=0)                # three channels
    assert ok, msg
    _same((d, r, disp, c, s), ref)
    exact = _reference(size, F, 16, "rest", "ordered", 0.0, True)
    ok, d, r, disp, c, s, msg = patolette_amd.frame_deltas_rgba(maps, 16)                           # a row count, no shown
    assert ok and s is None, msg
    assert np.array_equal(d, exact[0]) and np.array_equal(r, exact[2]) and np.array_equal(disp, exact[3])


# ---- the C entry ---------------------------------------------------------------------------------------------------------

def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c_call(gpu, maps, elem, rows, frames=None, channels=4, palette=None, palette_u8=None, tolerance=0.0, loop=1, delta=None, shown=None,
            rects=None, disposals=None, changed=None, dims=None):
    F, h, w = dims if dims is not None else maps.shape
    code = C.c_int(7)
    i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    gpu.patolette_amd_frame_deltas_rgba(F, w, h, _vp(maps), elem, rows, _vp(frames), channels,
                                        None if palette is None else palette.ctypes.data_as(_native.dp), _vp(palette_u8), tolerance, loop,
                                        _vp(delta), _vp(shown), i32(rects), i32(disposals),
                                        None if changed is None else changed.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(code))
    return code.value


def test_elements_aliasing_and_outputs_through_the_c_entry(gpu):
    size, F = SIZES["odd64"]
    frames, pal, maps = _case(size, F, 16, "rest")
    for tolerance in (0.0, 0.05):
        kw = dict(frames=frames, palette_u8=pal, tolerance=tolerance) if tolerance else {}
        ref = _reference(size, F, 16, "rest", "ordered", tolerance, True)
        for eb, dt in ((1, np.uint8), (2, np.uint16), (4, np.uint32), (8, np.uint64)):
            m = maps.astype(dt)
            d, s = np.full_like(m, 9), np.full_like(m, 9)
            r, disp, c = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.uint64)
            assert _c_call(gpu, m, eb, 16, delta=d, shown=s, rects=r, disposals=disp, changed=c, **kw) == 0
            _same((d, r, disp, c.astype(np.int64), s), ref)
            inout = m.copy()                                          # delta_maps aliasing palette_maps
            assert _c_call(gpu, inout, eb, 16, delta=inout, **kw) == 0
            assert np.array_equal(inout, ref[0].astype(dt))
        # every output NULL but one; loop 0
        d, s = np.zeros_like(maps), np.zeros_like(maps)
        r, disp, c = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.uint64)
        assert _c_call(gpu, maps, 1, 16, delta=d, **kw) == 0 and np.array_equal(d, ref[0])
        assert _c_call(gpu, maps, 1, 16, shown=s, **kw) == 0 and np.array_equal(s, ref[1])
        assert _c_call(gpu, maps, 1, 16, rects=r, **kw) == 0 and np.array_equal(r, ref[2])
        assert _c_call(gpu, maps, 1, 16, disposals=disp, **kw) == 0 and np.array_equal(disp, ref[3])
        assert _c_call(gpu, maps, 1, 16, changed=c, **kw) == 0 and np.array_equal(c.astype(np.int64), ref[4])
        assert _c_call(gpu, maps, 1, 16, **kw) == 0
        once = _reference(size, F, 16, "rest", "ordered", tolerance, False)
        assert _c_call(gpu, maps, 1, 16, loop=0, delta=d, rects=r, disposals=disp, **kw) == 0
        assert np.array_equal(d, once[0]) and np.array_equal(r, once[2]) and np.array_equal(disp, once[3])


def test_errors_and_recovery(gpu):
    size, F = SIZES["odd64"]
    h, w = size
    frames, pal, maps = _case(size, F, 16, "rest")
    palf = np.asfortranarray(pal.astype(np.float64) / 255.0)
    ref = _reference(size, F, 16, "rest", "ordered", 0.05, True)
    d = np.zeros_like(maps)
    r = np.zeros((F, 4), dtype=np.int32)

    def lossy(m=maps, **kw):
        args = dict(frames=frames, palette_u8=pal, tolerance=0.05, delta=d, rects=r)
        args.update(kw)
        return _c_call(gpu, m, args.pop("elem", 1), args.pop("rows", 16), **args)

    def good():
        d[:] = 99
        r[:] = -1
        assert lossy() == 0
        assert np.array_equal(d, ref[0]) and np.array_equal(r, ref[2])

    def failed(code, *words):
        assert code == -1
        text = _native.last_error()
        assert text.startswith(PREFIX) and all(word in text for word in words), text
        good()

    good()
    # an element that is no row: the kernel's flag, in both modes -- in frame 0, in a middle frame, at the last position
    for at in ((0, 0, 0), (3, 17, 5), (F - 1, h - 1, w - 1)):
        bad = maps.copy()
        bad[at] = 16
        failed(lossy(m=bad), "palette_rows")
        failed(_c_call(gpu, bad, 1, 16, delta=d), "palette_rows")
    bad = maps.copy()
    bad[0, 0, 0] = 200
    failed(lossy(m=bad), "palette_rows")
    filled = np.full((20, 3), -1.0, order="F")                        # ... and one that names a dropped row
    filled[:16] = palf
    bad = maps.copy()
    bad[2, h - 1, w - 1] = 17
    failed(lossy(m=bad, palette_u8=None, palette=filled, rows=20), "dropped")
    assert lossy(palette_u8=None, palette=filled, rows=20) == 0 and np.array_equal(d, ref[0])
    with pytest.raises(ValueError, match="palette_rows"):
        patolette_amd.frame_deltas_rgba(bad, pal, frames=frames, tolerance=0.05, transparent_index=0)
    good()
    # -1: the arguments
    failed(lossy(elem=3), "map_elem_bytes")
    failed(lossy(elem=0), "map_elem_bytes")
    failed(lossy(channels=2), "channels")
    failed(lossy(channels=5), "channels")
    for tolerance in (-0.01, float("nan"), float("inf"), -float("inf")):
        failed(lossy(tolerance=tolerance), "tolerance")
    failed(lossy(loop=2), "loop")
    failed(lossy(loop=-1), "loop")
    failed(lossy(palette=palf), "exactly one")
    failed(lossy(palette_u8=None), "exactly one")
    failed(lossy(frames=None), "pixels")
    failed(lossy(rows=0), "palette_rows")
    nan = palf.copy(order="F")
    nan[3, 1] = np.nan
    failed(lossy(palette_u8=None, palette=nan), "finite")
    code = C.c_int(7)
    gpu.patolette_amd_frame_deltas_rgba(F, w, h, None, 1, 16, None, 4, None, None, 0.0, 1, _vp(d), None, None, None, None, C.byref(code))
    failed(code.value, "no maps")
    assert lossy(tolerance=-0.0) == 0                                 # -0.0 is not negative: the exact mode
    # -2 and -4
    assert lossy(dims=(0, h, w)) == -2
    assert lossy(dims=(F, 0, w)) == -2
    assert lossy(dims=(F, h, 0)) == -2
    good()
    assert lossy(dims=(1 << 31, h, w)) == -4 and _native.last_error().startswith(PREFIX) and "too big" in _native.last_error()
    assert lossy(dims=(1, 50000, 50000)) == -4
    good()
    ok, *rest, msg = patolette_amd.frame_deltas_rgba(np.zeros((2, 0, 5), dtype=np.uint8), 16)
    assert not ok and rest == [None] * 5 and msg == "Image dimensions should be greater than 0."


def test_last_stats_and_launches(gpu):
    size, F = SIZES["wide"]
    frames, pal, maps = _case(size, F, 16, "rest", "nearest")
    for tolerance in (0.0, 0.05):
        for want_shown in (False, True):
            _native.profile(True)
            ok, *_ = patolette_amd.frame_deltas_rgba(maps, pal, frames=frames, tolerance=tolerance, want_shown=want_shown, transparent_index=0)
            prof = _native.profile_results()
            _native.profile(False)
            assert ok
            assert prof["k_rgba_vanish"]["launches"] == 1 and prof["k_frame_delta_rgba"]["launches"] == F
            assert not set(prof) & {"k_frame_deltas", "k_delta_boxes", "k_convert_u8", "k_convert", "k_nn_map", "k_nn_map_u8", "k_ordered_map"}
            st = patolette_amd.last_stats()
            assert st["ms_total"] > 0 and st["ms_map"] > 0 and st["ms_upload"] > 0 and st["ms_download"] > 0
            assert st["ms_total"] >= st["ms_map"]
            assert all(st[key] == 0 for key in st if not key.startswith("ms_"))
            assert st["ms_convert"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0 and st["ms_kmeans"] == 0 and st["ms_saliency"] == 0


def test_workspace_history(gpu):
    """Fresh workspace, poisoned workspace, a workspace other entries have used and grown: the same bits, and nothing grows late."""
    size, F = SIZES["wrap"]
    frames, pal, maps = _case(size, F, 300, "rest")
    other = _image("noise", (96, 80), 1, 3)
    small = _case(*SIZES["odd64"], 16, "rest")

    def run(want_shown=True):
        ok, d, r, disp, c, s, msg = patolette_amd.frame_deltas_rgba(maps, pal, frames=frames, tolerance=0.02, want_shown=want_shown,
                                                                    transparent_index=0)
        assert ok, msg
        return d, r, disp, c, s

    gpu.patolette_amd_release_workspace()
    fresh = run()
    _same(fresh, _reference(size, F, 300, "rest", "ordered", 0.02, True))
    gpu.patolette_amd_release_workspace()
    prev = gpu.patolette_amd_debug_workspace(1 | 2)
    try:
        before = gpu.patolette_amd_debug_late_growths()
        ok, *_ = patolette_amd.quantize_u8(other, 16, dither=True, tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
        assert ok
        ok, *_ = patolette_amd.frame_deltas_rgba(small[2], small[1], frames=small[0], tolerance=0.05, transparent_index=0)
        assert ok
        first = run()
        ok, *_ = patolette_amd.frame_deltas(small[2], 16, want_shown=True)
        assert ok
        unshown = run(False)
        second = run()
        assert gpu.patolette_amd_debug_late_growths() == before
    finally:
        gpu.patolette_amd_debug_workspace(prev)
        gpu.patolette_amd_release_workspace()
    for got in (first, second):
        assert all(np.array_equal(a, b) for a, b in zip(got, fresh))
    assert unshown[4] is None and all(np.array_equal(a, b) for a, b in zip(unshown[:4], fresh[:4]))


def test_torch_flavour(gpu):
    """Torch CUDA tensors go through patolette_amd_frame_deltas_rgba_device: the numpy flavour's results, deltas and shown on the maps'
    device.  Own process: torch loads its HIP runtime before libpatolette_amd.so does."""
    import subprocess
    import sys
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
if not torch.cuda.is_available():
    print("TORCH-NO-DEVICE")
    sys.exit(0)
import patolette_amd as p
from oracle import binding as ob
from tests import rgba_delta_ref
from tests.test_gpu_remap import _palette
for size, F, rows in (((37, 53), 8, 300), ((120, 64), 6, 16), ((36, 301), 3, 300)):
    frames, pal = rgba_delta_ref.clip(size[0], size[1], F, rest=2), _palette(rows, seed=2)
    maps = rgba_delta_ref.maps_of(ob, frames, pal, "nearest")
    m_np = maps.astype(np.uint8 if rows <= 256 else np.uint16)
    m_t = torch.from_numpy(maps.astype(np.uint8 if rows <= 256 else np.int32)).cuda()
    f_t = torch.from_numpy(frames).cuda()
    for tol in (0.0, 0.05):
        for loop in (True, False):
            p._native.lib().patolette_amd_debug_delta_quad(-1)
            ok, d, r, disp, c, s, msg = p.frame_deltas_rgba(m_np, pal, frames=frames, tolerance=tol, loop=loop, want_shown=True, transparent_index=0)
            assert ok, msg
            p._native.lib().patolette_amd_debug_delta_quad(1)       # four positions per lane where the tensors allow it
            ok, dt, rt, dispt, ct, st, msg = p.frame_deltas_rgba(m_t, pal, frames=f_t, tolerance=tol, loop=loop, want_shown=True, transparent_index=0)
            assert ok, msg
            assert dt.device == m_t.device and st.device == m_t.device and dt.dtype == m_t.dtype and tuple(dt.shape) == d.shape
            assert isinstance(rt, np.ndarray) and isinstance(ct, np.ndarray) and isinstance(dispt, np.ndarray)
            assert np.array_equal(dt.cpu().numpy().astype(np.int64), d.astype(np.int64))
            assert np.array_equal(st.cpu().numpy().astype(np.int64), s.astype(np.int64))
            assert np.array_equal(rt, r) and np.array_equal(ct, c) and np.array_equal(dispt, disp)
            ok, dt2, rt2, dispt2, ct2, none, msg = p.frame_deltas_rgba(m_t, pal, frames=f_t, tolerance=tol, loop=loop, transparent_index=0)
            assert ok and none is None, msg
            assert torch.equal(dt2, dt) and np.array_equal(rt2, r) and np.array_equal(dispt2, disp) and np.array_equal(ct2, c)
    try:
        p.frame_deltas_rgba(m_t, pal, frames=frames, tolerance=0.05, transparent_index=0)
        raise SystemExit("host frames with device maps were accepted")
    except ValueError:
        pass
print("TORCH-RGBA-DELTA-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-RGBA-DELTA-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- end to end: quantise, deltas, file --------------------------------------------------------------------------------------

@pytest.mark.parametrize("tolerance", [0.0, 0.05])
@pytest.mark.parametrize("name", ["odd64", "wide"])
def test_from_frames_to_a_file(gpu, name, tolerance):
    from oracle import binding as ob
    size, F = SIZES[name]
    frames = _clip(size, F, 2)                                        # (the disc rests every second frame: see rgba_delta_ref.clip)
    ok, prgba, maps, _, palf, tidx, msg = patolette_amd.quantize_rgba_frames(frames, 256, dither="ordered", tile_size=0, kmeans_niter=2,
                                                                            kmeans_max_samples=4096, want_quantized=False)
    assert ok and tidx == 0 and maps.dtype == np.uint8, msg
    ok, d, r, disp, c, s, msg = patolette_amd.frame_deltas_rgba(maps, prgba, frames=frames, tolerance=tolerance, want_shown=True)
    assert ok, msg
    assert np.any(disp == 2) and np.array_equal(s != 0, maps != 0)
    if tolerance == 0:
        assert np.array_equal(s, maps)
    else:
        assert np.any(s != maps) and np.sum(c) < np.sum(maps != 0)    # the lossy mode held something
        ref = rgba_delta_ref.frame_deltas(ob, maps, prgba, frames=frames, tolerance=tolerance)
        print("end to end %s: %d distances, %d kept, smallest relative gap %.3g" % (name, ref[6], ref[7], ref[5]))
        if ref[5] >= MIN_GAP:
            _same((d, r, disp, c, s), ref[:5])
    blob = patolette_amd.write_gif(None, d, prgba[:, :3], r, transparent_index=0, disposal=disp)
    head, parsed = lzw_ref.parse_gif(blob)
    assert (head["height"], head["width"]) == size and len(parsed) == F
    assert [fr["disposal"] for fr in parsed] == disp.tolist() and all(fr["transparent"] == 0 for fr in parsed)
    shows = rgba_delta_ref.replay_parsed(head, parsed, 2)
    assert np.array_equal(shows[:F], s) and np.array_equal(shows[F:], s)
    assert rgba_delta_ref.same_picture(rgba_delta_ref.pil_frames(blob), rgba_delta_ref.rgba_of(prgba[:, :3], s))
    # what the rectangles and the deltas buy: against the full frames written with disposal 2
    full = patolette_amd.write_gif(None, maps, prgba[:, :3], None, transparent_index=0, disposal=2)
    print("end to end %s tolerance %g: %d bytes as deltas, %d as full frames; rectangle area %d of %d"
          % (name, tolerance, len(blob), len(full), int(np.sum(r[:, 2].astype(np.int64) * r[:, 3])), F * size[0] * size[1]))
