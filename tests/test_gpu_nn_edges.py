"""The nearest map's three kernel routes at their edges, ties and margins: every comparison is bit for bit against the CPU oracle's
brute force (ob.nn_map), through patolette_amd_debug_nn_map_elem, except where a remap is named (tests/remap_ref.py).

patolette_amd_debug_nn_route(1 | 2 | 3) sends a map of any size down the route of a size class (brute force below 16 384 pixels; the
32^3 candidate table; from 2^22 pixels the 64^3 table behind a four-candidate table in LDS, k_nn_map_mid), so that the tails, queues,
packed stores and margins of the large-image kernels are met with a few hundred pixels.  Which route ran is read off the profile:
k_nn_lut_build is absent on route 1 and its bytes per launch are 32 x 32^3 on route 2, 32 x 64^3 on route 3 (64 x for more than 256
palette rows) -- the three map kernels themselves are all timed as k_nn_map.  The inputs come from tests/nn_ref.py, whose promises
tests/test_nn_reference.py checks without a GPU."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import nn_ref, remap_ref
from tests.util import ROOT

pytestmark = pytest.mark.gpu

ROUTES = (0, 1, 2, 3)
ELEMS = ((1, 0), (1, 1), (4, 0))                                   # (map element bytes, misalign)
DTYPES = {1: np.uint8, 4: np.uint32, 8: np.uint64}


def _planar(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).reshape(-1)


def _dp(a):
    return a.ctypes.data_as(_native.dp)


def _default_map(L, px, pal):
    got = np.zeros(px.shape[0], dtype=np.uintp)
    assert L.patolette_amd_nn_map(_dp(_planar(px)), px.shape[0], _dp(_planar(pal)), pal.shape[0], got.ctypes.data_as(_native.zp)) == 0
    return got


def _hygiene_input():
    rng = np.random.default_rng(2024)
    return rng.random((100000, 3)), rng.random((64, 3))


@pytest.fixture(scope="module", autouse=True)
def untouched(gpu):
    """the default route's map of 100 000 pixels before this file touches a knob (test_knobs_are_back_where_they_were, last)"""
    assert gpu.patolette_amd_debug_nn_route(0) == 0
    return _default_map(gpu, *_hygiene_input())


@pytest.fixture(autouse=True)
def _knobs_restored(gpu, untouched):
    try:
        yield
    finally:
        gpu.patolette_amd_debug_nn_route(0)
        gpu.patolette_amd_debug_remap_two_pass(0)
        _native.profile(False)


_want_cache = {}


def _want(ob, key, px, pal):
    """the oracle's map, computed once per named input"""
    if key not in _want_cache:
        _want_cache[key] = ob.nn_map(_planar(px), px.shape[0], np.ascontiguousarray(pal)).astype(np.int64)
    return _want_cache[key]


def _build_bytes(route, n, k):
    """k_nn_lut_build's bytes per launch on the route a map of n pixels and k rows takes, None where no table is built"""
    cls = route - 1 if route else (2 if n >= 1 << 22 else 1 if n >= 16384 else 0)
    if cls == 0 or not 8 <= k <= 4096:
        return None
    return (32 if k <= 256 else 64) * (64 if cls == 2 else 32) ** 3


def _map(L, px, pal, elem, misalign=0, flat=None, pflat=None):
    n, k = px.shape[0], pal.shape[0]
    flat = _planar(px) if flat is None else flat
    pflat = _planar(pal) if pflat is None else pflat
    got = np.full(n, 0xA5, dtype=DTYPES[elem]) if elem == 1 else np.zeros(n, dtype=DTYPES[elem])
    assert L.patolette_amd_debug_nn_map_elem(_dp(flat), n, _dp(pflat), k, elem, misalign, got.ctypes.data_as(C.c_void_p)) == 0, _native.last_error()
    return got.astype(np.int64)


def _check(L, name, px, pal, want, route, elems=ELEMS, build="route"):
    """the map under `route` for every element layout == want; the route's kernels ran"""
    n, k = px.shape[0], pal.shape[0]
    flat, pflat = _planar(px), _planar(pal)
    L.patolette_amd_debug_nn_route(route)
    try:
        for elem, misalign in elems:
            if elem == 1 and k > 256:
                continue
            _native.profile(True)
            got = _map(L, px, pal, elem, misalign, flat, pflat)
            res = _native.profile_results()
            _native.profile(False)
            mism = int(np.sum(got != want))
            print("nn %s: route %d n %d k %d elem %d misalign %d: %d differ from the oracle; kernels %s" %
                  (name, route, n, k, elem, misalign, mism, sorted(res)))
            assert mism == 0, np.nonzero(got != want)[0][:10]
            assert res["k_nn_map"]["launches"] == 1
            expect = _build_bytes(route, n, k) if build == "route" else build
            if expect is None:
                assert "k_nn_lut_build" not in res
            else:
                assert res["k_nn_lut_build"]["launches"] == 1 and res["k_nn_lut_build"]["bytes"] == expect
    finally:
        L.patolette_amd_debug_nn_route(0)


# ---- constructed ties, near-ties, margins, queues -------------------------------------------------------------------------------------
def _constructed(name):
    if name == "lattice":
        return nn_ref.lattice()
    if name.startswith("shifted-"):
        return nn_ref.lattice_shifted(int(name[8:]))
    if name.startswith("sweep-"):
        return nn_ref.margin_sweep(64, name[6:])[:2]
    if name == "bisectors":
        return nn_ref.edge_bisectors(*nn_ref.random_box())[:2]
    if name == "lattice-300":                                      # unsigned-short candidates: the lattice's rows and 175 more dyadic ones
        px, pal = nn_ref.lattice()
        return px, np.concatenate([pal, np.random.default_rng(8).integers(0, 65, size=(175, 3)) / 64.0])
    assert name.startswith("crowded-")
    return nn_ref.crowded(name[8:])[:2]


CONSTRUCTED = (["lattice"] + ["shifted-%d" % s for s in (30, 40, 50, 52)] + ["sweep-" + b for b in nn_ref.BOXES] + ["bisectors"] +
               ["crowded-" + d for d in nn_ref.CROWDED])


@pytest.mark.parametrize("name", CONSTRUCTED)
@pytest.mark.parametrize("route", ROUTES)
def test_ties_margins_and_queues(gpu, ob, route, name):
    px, pal = _constructed(name)
    _check(gpu, name, px, pal, _want(ob, name, px, pal), route)


@pytest.mark.parametrize("route", ROUTES)
def test_eight_byte_elements(gpu, ob, route):
    px, pal = _constructed("lattice")
    _check(gpu, "lattice", px, pal, _want(ob, "lattice", px, pal), route, elems=((8, 0),))


@pytest.mark.parametrize("route", (2, 3))
def test_lattice_with_300_rows(gpu, ob, route):
    px, pal = _constructed("lattice-300")
    _check(gpu, "lattice-300", px, pal, _want(ob, "lattice-300", px, pal), route, elems=((4, 0), (8, 0)))


@pytest.mark.parametrize("k", (8, 256, 300))
@pytest.mark.parametrize("G", (32, 64))
@pytest.mark.parametrize("route", ROUTES)
def test_cell_edges(gpu, ob, route, G, k):
    lo, hi = nn_ref.random_box()
    px, pal = nn_ref.cell_edges(G, lo, hi), nn_ref.box_palette(k, lo, hi)
    name = "edges-%d-%d" % (G, k)
    _check(gpu, name, px, pal, _want(ob, name, px, pal), route)


# ---- shapes: tails, one wavefront, several trips --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cus():
    """the device's compute units, from torch in a child process (it loads its own HIP runtime); 256, an MI355X's, where torch is not to
    be had"""
    code = "import torch; print('CUS', torch.cuda.get_device_properties(0).multi_processor_count)"
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
        for line in r.stdout.splitlines():
            if line.startswith("CUS "):
                return int(line.split()[1])
    except (OSError, subprocess.SubprocessError):
        pass
    print("compute units: torch did not tell; taking an MI355X's 256")
    return 256


def _trip_n(cus):
    return 2 * cus * 16 * 256 + 77                                 # every wavefront of k_nn_map_mid a second tile, the last one partial


@pytest.fixture(scope="module")
def randoms(ob, cus):
    """random pixels on a random palette of 16 rows and the oracle's map, once, for every shape (a pixel's row does not depend on the
    others: a prefix of the pixels has the prefix of the map)"""
    rng = np.random.default_rng(11)
    n = _trip_n(cus)
    px, pal = rng.random((n, 3)), rng.random((16, 3))
    return px, pal, ob.nn_map(_planar(px), n, pal).astype(np.int64)


def _shape_list(unit):
    return [1, 2, 63, 64, 65, unit - 1, unit, unit + 1, 16 * unit - 1, 16 * unit, 16 * unit + 1, 2 * 16 * unit + 3]


@pytest.mark.parametrize("route", (1, 2, 3))
def test_small_shapes(gpu, randoms, route):
    """around one tile of k_nn_map_mid (64 lanes x 4 pixels with 1-byte elements, x 2 otherwise), one block of 16 wavefronts, two blocks;
    the same counts around the block of 256 of the other two kernels.  Odd and even n, each with an even and an odd output address."""
    px, pal, want = randoms
    for elem, misalign in ELEMS:
        unit = nn_ref.tile(elem) if route == 3 else 256
        for n in _shape_list(unit):
            _check(gpu, "shape", px[:n], pal, want[:n], route, elems=((elem, misalign),))


@pytest.mark.parametrize("route", (1, 2, 3))
def test_several_trips(gpu, randoms, cus, route):
    """2 x CUs x 16 x 256 + 77 pixels: every wavefront of k_nn_map_mid prefetches across `base += step`, the last tile is partial and
    takes the slow fetch; k_nn_map_lut takes its second pair of pixels; the brute kernel its second trip."""
    px, pal, want = randoms
    assert px.shape[0] == _trip_n(cus)
    _check(gpu, "trips", px, pal, want, route)


@pytest.mark.parametrize("elem", (1, 4))
def test_crowded_tail(gpu, ob, cus, elem):
    """overflow pixels in the last, partial tile: inside `left` (they are parked and flushed at the end), and as the very last pixel,
    which the lanes beyond `left` read too (they must park nothing).  One tile, 17 tiles, and the second trip's tail."""
    t = nn_ref.tile(elem)
    t8 = nn_ref.tie8_points()
    for n in (t + 1, t + 77, 16 * t + 40, 2 * cus * 16 * t + 77):
        px, pal, over = nn_ref.crowded("sparse", n)
        left = n % t
        for back in sorted({1, (left + 1) // 2, left}):
            px[n - back] = t8[back % 64]
        name = "tail-%d" % n
        _check(gpu, name, px, pal, _want(ob, name, px, pal), 3, elems=((elem, 0),) if elem == 4 else ((1, 0), (1, 1)))


@pytest.mark.parametrize("route", (2, 3))
def test_crowded_over_several_trips(gpu, ob, cus, route):
    """a queue that carries parked pixels from one tile of its wavefront to the next: one overflow pixel in a thousand over two trips"""
    n = _trip_n(cus)
    px, pal, over = nn_ref.crowded("sparse", n)
    name = "crowded-trips-%d" % n
    _check(gpu, name, px, pal, _want(ob, name, px, pal), route, elems=((1, 0),))


# ---- the natural thresholds ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold_pixels():
    return np.random.default_rng(21).random((16384, 3))


@pytest.mark.parametrize("k", (7, 8, 256, 257, 4096, 4097))
@pytest.mark.parametrize("n", (16383, 16384))
def test_natural_thresholds(gpu, ob, threshold_pixels, n, k):
    """default route on either side of 16 384 pixels and of 8, 256 / 257 and 4096 rows; a palette with one duplicated row"""
    pal = np.random.default_rng(k).random((k, 3))
    pal[k - 2] = pal[1]
    px = threshold_pixels[:n]
    want = _want(ob, "threshold-%d" % k, threshold_pixels, pal)[:n]
    assert not np.any(want == k - 2)
    table = n >= 16384 and 8 <= k <= 4096
    _check(gpu, "threshold", px, pal, want, 0, build=((32 if k <= 256 else 64) * 32 ** 3) if table else None)


# ---- the byte source (remap) ----------------------------------------------------------------------------------------------------------
def _byte_palette(rows, seed):
    codes = np.random.default_rng(seed).choice(1 << 24, size=rows, replace=False)
    return np.stack([codes >> 16, (codes >> 8) & 255, codes & 255], axis=1).astype(np.uint8)


def _remap_palette(kind):
    if kind in ("8", "16", "256"):
        return _byte_palette(int(kind), 40 + int(kind))
    if kind == "300-given-256-used":
        pal = np.full((300, 3), -1.0)
        pal[:256] = _byte_palette(256, 44).astype(np.float64) / 255.0
        return pal
    if kind == "duplicate-row":
        pal = _byte_palette(32, 45)
        pal[20] = pal[3]
        return pal
    assert kind == "own-colours"
    return _byte_palette(64, 46)


def _remap_image(shape, channels, pal8, own):
    rng = np.random.default_rng(sum(shape) + channels)
    if own:                                                        # every pixel IS a palette row: distance 0
        img = pal8[rng.integers(0, pal8.shape[0], size=shape)]
    else:
        img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
        img.reshape(-1, 3)[::7] = pal8[rng.integers(0, pal8.shape[0], size=len(img.reshape(-1, 3)[::7]))]
    if channels == 4:
        img = np.concatenate([img, rng.integers(0, 256, size=shape + (1,), dtype=np.uint8)], axis=-1)
    return np.ascontiguousarray(img)


REMAP_SHAPES = ((1, 1), (5, 3), (37, 53), (64, 64), (3, 37, 53))


@pytest.mark.parametrize("kind", ("8", "16", "256", "300-given-256-used", "duplicate-row", "own-colours"))
def test_byte_source_under_route_3(gpu, ob, kind):
    """remap(dither=False) of small images through k_nn_map_u8 (by default from 2^22 pixels on): against tests/remap_ref.py; the fused
    kernel ran; with the two-pass route forced it did not, and the maps are equal."""
    pal = _remap_palette(kind)
    pal8 = remap_ref.pal8(pal)[:256] if pal.dtype != np.uint8 else pal
    for shape in REMAP_SHAPES:
        for channels in (3, 4):
            image = _remap_image(shape, channels, pal8, kind == "own-colours")
            m_ref, q_ref = remap_ref.remap(ob, image, pal, dither=False)
            gpu.patolette_amd_debug_nn_route(3)
            _native.profile(True)
            ok, m, q, msg = patolette_amd.remap(image, pal, dither=False)
            names = set(_native.profile_results())
            gpu.patolette_amd_debug_remap_two_pass(1)
            _native.profile(True)
            ok2, m2, q2, msg2 = patolette_amd.remap(image, pal, dither=False)
            names2 = set(_native.profile_results())
            _native.profile(False)
            gpu.patolette_amd_debug_remap_two_pass(0)
            gpu.patolette_amd_debug_nn_route(0)
            assert ok and ok2, (msg, msg2)
            mism = int(np.sum(m.astype(np.int64) != m_ref))
            print("remap %s: shape %s channels %d: %d of %d differ from the reference; kernels %s / two-pass %s" %
                  (kind, shape, channels, mism, m.size, sorted(names), sorted(names2)))
            assert mism == 0 and np.array_equal(q, q_ref)
            assert m.dtype == (np.uint8 if pal.shape[0] <= 256 else np.uint16)
            assert "k_nn_map_u8" in names and "k_convert_u8" not in names and "k_nn_map" not in names
            assert "k_nn_map_u8" not in names2 and "k_convert_u8" in names2 and "k_nn_map" in names2
            assert np.array_equal(m2, m) and np.array_equal(q2, q)
            if kind == "own-colours":
                assert np.array_equal(q, image[..., :3])


@pytest.mark.parametrize("route", (0, 1, 2))
def test_byte_source_only_under_route_3(gpu, ob, route):
    pal = _remap_palette("16")
    image = _remap_image((37, 53), 3, pal, False)
    m_ref, _ = remap_ref.remap(ob, image, pal, dither=False)
    gpu.patolette_amd_debug_nn_route(route)
    _native.profile(True)
    ok, m, _, msg = patolette_amd.remap(image, pal, dither=False)
    res = _native.profile_results()
    _native.profile(False)
    assert ok, msg
    assert "k_nn_map_u8" not in res and "k_nn_map" in res
    assert ("k_nn_lut_build" in res) == (route == 2)
    assert np.array_equal(m.astype(np.int64), m_ref)


def test_byte_source_to_an_odd_device_address(gpu, ob):
    """patolette_amd_remap_u8_device with the map one byte into its allocation: whole tiles take byte stores instead of packed ones"""
    pal = _remap_palette("16")
    for shape in ((37, 53), (64, 64)):
        image = _remap_image(shape, 3, pal, False)
        m_ref, _ = remap_ref.remap(ob, image, pal, dither=False)
        h, w = shape
        n = h * w
        d_px, d_map = gpu.patolette_amd_malloc(3 * n), gpu.patolette_amd_malloc(n + 2)
        assert d_px and d_map
        try:
            guard = np.full(n + 2, 0xEE, dtype=np.uint8)
            assert gpu.patolette_amd_memcpy_h2d(d_px, image.ctypes.data_as(C.c_void_p), 3 * n) == 0
            assert gpu.patolette_amd_memcpy_h2d(d_map, guard.ctypes.data_as(C.c_void_p), n + 2) == 0
            code = C.c_int(7)
            gpu.patolette_amd_debug_nn_route(3)
            _native.profile(True)
            gpu.patolette_amd_remap_u8_device(1, w, h, d_px, 3, None, pal.ctypes.data_as(C.c_void_p), 16, 0, d_map + 1, 1, None, C.byref(code))
            names = set(_native.profile_results())
            _native.profile(False)
            gpu.patolette_amd_debug_nn_route(0)
            assert code.value == 0, _native.last_error()
            assert "k_nn_map_u8" in names
            got = np.zeros(n + 2, dtype=np.uint8)
            assert gpu.patolette_amd_memcpy_d2h(got.ctypes.data_as(C.c_void_p), d_map, n + 2) == 0
            assert got[0] == 0xEE and got[n + 1] == 0xEE            # nothing written before or behind the map
            assert np.array_equal(got[1:n + 1].astype(np.int64).reshape(h, w), m_ref)
        finally:
            gpu.patolette_amd_free(d_px)
            gpu.patolette_amd_free(d_map)


# ---- non-finite and huge values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("inf-plane0", "nan", "minus-inf-plane2", "1e39"))
@pytest.mark.parametrize("n,route", ((20000, 0), (20000, 3), (300, 3), (300, 2)))
def test_non_finite_and_huge_pixels(gpu, ob, n, route, variant):
    """One odd pixel must not move any other: the reference gives a pixel whose distances are all NaN or +Inf index 0 and every other
    pixel what it gets without the odd one.  (An infinite bound admits no grid: such an image takes the brute-force kernel.  A range
    that f32 cannot hold keeps off the LDS-table kernel, whose cell index is f32 and unclamped: 1e39 takes the 32^3 table.)"""
    rng = np.random.default_rng(n)
    px, pal = rng.random((n, 3)), rng.random((16, 3))
    clean = _want(ob, "finite-%d" % n, px, pal)
    odd = n // 3
    plane, value = {"inf-plane0": (0, np.inf), "nan": (1, np.nan), "minus-inf-plane2": (2, -np.inf), "1e39": (0, 1e39)}[variant]
    px = px.copy()
    px[odd, plane] = value
    want = ob.nn_map(_planar(px), n, pal).astype(np.int64)
    assert np.array_equal(np.delete(want, odd), np.delete(clean, odd))
    if not np.isfinite(value):
        assert want[odd] == 0
    build = _build_bytes(route, n, 16)
    if np.isinf(value):
        build = None
    elif variant == "1e39":
        build = 32 * 32 ** 3
    _check(gpu, variant, px, pal, want, route, build=build)


# ---- last: the knobs are back -------------------------------------------------------------------------------------------------------
def test_knobs_are_back_where_they_were(gpu, untouched):
    assert gpu.patolette_amd_debug_nn_route(0) == 0
    assert gpu.patolette_amd_debug_remap_two_pass(0) == 0
    px, pal = _hygiene_input()
    _native.profile(True)
    again = _default_map(gpu, px, pal)
    res = _native.profile_results()
    _native.profile(False)
    assert np.array_equal(again, untouched)
    assert res["k_nn_lut_build"]["bytes"] == 32 * 32 ** 3         # 100 000 pixels: the 32^3 table, as the size says
    assert gpu.patolette_amd_debug_nn_route(2) == 0 and gpu.patolette_amd_debug_nn_route(9) == 2 and gpu.patolette_amd_debug_nn_route(0) == 0
