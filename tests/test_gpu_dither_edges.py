"""The dither's own nearest-colour searches at ties, margins and grid edges, under both layouts: k_dither's register search with its
hand-scheduled DPP blocks (and the copy in k_dither_lane_repair), k_dither_lanes' three nested grids with the f32 first pass, and the
whole-wavefront scan dither_nearest_all.  Every case goes through patolette_amd_dither and must be the oracle's chain bit for bit.

The images come from tests/dither_ref.py: probes between resets, so that every seventeenth step of the real chain is a query chosen
by the test (tests/test_dither_reference.py checks, without a GPU, that the resets hold and which classes of query the images meet).
patolette_amd_debug_dither_lane_tables reads back what the lane layout's search read: the host's grid arithmetic is held to its
restatement bit for bit, the records to their own claim (every row that attains the minimum is listed), and the routes the kernel
took are counted from the device's own records."""
import ctypes as C

import numpy as np
import pytest

from patolette_amd import _native
from tests import dither_ref as dr
from tests import util

pytestmark = pytest.mark.gpu

FLOOR = 64


def _dp(a):
    return a.ctypes.data_as(_native.dp)


def _dither(L, image, w, h, pal):
    k = pal.shape[0]
    got = np.zeros(w * h, dtype=np.uintp)
    p = np.ascontiguousarray(pal.T).reshape(-1)
    assert L.patolette_amd_dither(_dp(image), w, h, _dp(p), k, got.ctypes.data_as(_native.zp)) == 0, _native.last_error()
    return got.astype(np.int64), _native.last_stats()


def _hygiene_input(ob):
    w = h = 256
    flat = ob.convert("srgb_to_rec2020", ob.image(w * h, 41))
    pal = ob.convert("srgb_to_rec2020", ob.image(64, 43)).reshape(3, 64).T.copy()
    return flat, w, h, pal


@pytest.fixture(scope="module", autouse=True)
def untouched(gpu, ob):
    """the default dither of a noise image before this file touches a knob (test_knobs_are_back_where_they_were, last)"""
    flat, w, h, pal = _hygiene_input(ob)
    got, st = _dither(gpu, flat, w, h, pal)
    return got, st["dither_segments"]


@pytest.fixture(autouse=True)
def _knobs_restored(gpu, untouched):
    try:
        yield
    finally:
        gpu.patolette_amd_dither_config(0, -1)
        gpu.patolette_amd_dither_layout(-1)
        gpu.patolette_amd_debug_dither_stall_passes(-1)
        gpu.patolette_amd_debug_dither_solo_cap(-1)


def _report(name, what, ev, got, st):
    bad = np.nonzero(got != ev.want)[0]
    print("dither %s, %s: %d of %d differ from the oracle; runs %d repairs %d passes %d solo %d" %
          (name, what, bad.size, got.size, st["dither_segments"], st["dither_repairs"], st["dither_rounds"], st["dither_solo"]))
    if bad.size:
        rank = np.empty(got.size, dtype=np.int64)
        rank[ev.order] = np.arange(got.size)
        first = int(np.min(rank[bad]))
        print("   first at curve rank %d (a probe: %s): got %d, oracle %d" % (first, bool(ev.probe[first]), got[ev.order[first]], ev.chain[first]))
    return bad.size


# ---- one wavefront per run: k_dither's search -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", (1, 7, 0))
@pytest.mark.parametrize("name", dr.wave_cases())
def test_wavefront_layout(gpu, ob, name, segments):
    """PER = 1, 2, 4 rows per lane in registers, the generic loop from 257 rows, the tables in global memory from 3201; exact ties (the
    lowest index of up to 400 tied rows), near-ties down to one low-word step; one chain, seven runs, the default cut"""
    ev = dr.evaluated(ob, name)
    lay = ev.lay
    gpu.patolette_amd_dither_layout(0)
    gpu.patolette_amd_dither_config(segments, -1)
    got, st = _dither(gpu, lay.image, lay.width, lay.height, lay.pal)
    assert _report(name, "wavefronts, %d runs asked" % segments, ev, got, st) == 0
    if segments:
        assert st["dither_segments"] == segments


# ---- one lane per run: k_dither_lanes' search ---------------------------------------------------------------------------------------------
def _tables(L, npix):
    geom = np.zeros(30)
    amb = np.zeros(3, dtype=np.float32)
    assert L.patolette_amd_debug_dither_lane_tables(_dp(geom), amb.ctypes.data_as(C.POINTER(C.c_float)), None, 0) == 0, _native.last_error()
    g = geom.reshape(3, 10)
    G = g[:, 9].astype(np.int64)
    raw = np.zeros(32 * int(np.sum(G ** 3)), dtype=np.uint8)
    assert L.patolette_amd_debug_dither_lane_tables(_dp(geom), amb.ctypes.data_as(C.POINTER(C.c_float)), raw.ctypes.data_as(C.c_void_p), raw.size) == 0
    return dr.Geometry(g[:, 0:3].copy(), g[:, 3:6].copy(), g[:, 6:9].copy(), G, amb[0], amb[1], amb[2]), dr.Tables(raw, G)


def _check_tables(L, ev, routes=None):
    """the device's geometry == its restatement, bit for bit; every record the replayed chain reads lists every row that attains the
    reference's minimum (unless it says "more than thirty"); routes: a dict that takes the counts of what the kernel met"""
    lay = ev.lay
    npix = lay.width * lay.height
    dev, tab = _tables(L, npix)
    geo = dr.lane_geometry(lay.pal, npix)
    for a, b, what in ((dev.lo, geo.lo, "lo"), (dev.hi, geo.hi, "hi"), (dev.inv, geo.inv, "inv")):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (ev.name, what, a, b)
    assert np.array_equal(dev.G, geo.G)
    for a, b, what in ((dev.amb, geo.amb, "amb"), (dev.amb_p, geo.amb_p, "amb_p"), (dev.amb_x, geo.amb_x, "amb_x")):
        assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32), (ev.name, what, a, b)
    big = ev.name.startswith("big-")
    sel = np.arange(npix) if not big else np.concatenate([np.arange(70000 + dr.STRIDE), lay.ranks[lay.ranks > 70000]])
    q, idx, gap = ev.q[sel], ev.idx[sel], ev.gap[sel]
    palw = lay.pal * dr.FW
    lv, cnt, ent = tab.records(q, dev)
    listed = cnt != 255
    assert np.all(cnt[listed] <= 30) and np.all(cnt[listed] >= 1), ev.name
    assert np.all(cnt[lv == 3] == 255)
    valid = np.arange(30)[None, :] < cnt[:, None]
    assert np.all(ent[valid & listed[:, None]] < lay.pal.shape[0]), ev.name
    missing = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, q.shape[0], 8192):
            c = q[s:s + 8192]
            d0, d1, d2 = (c[:, None, a] - palw[None, :, a] for a in range(3))
            d = (d0 * d0 + d1 * d1) + d2 * d2
            tied = d == np.min(np.where(np.isnan(d), np.inf, d), axis=1)[:, None]
            e, v, li = ent[s:s + 8192], valid[s:s + 8192], listed[s:s + 8192]
            have = np.zeros_like(tied)
            rows = np.repeat(np.arange(c.shape[0]), 30).reshape(-1, 30)
            have[rows[v], e[v]] = True
            missing += int(np.sum(tied & ~have & li[:, None]))
    where = np.argmax((ent == idx[:, None]) & valid, axis=1)                # the winner's place in its cell's list
    if routes is not None:
        M = dr.query_margin(q, dev)
        within, clear = gap <= 0.5 * M, gap > 2.0 * M
        for key, sel_ in (("short list", listed & (cnt <= 15)), ("second record wins", listed & (cnt > 15) & (where >= 15)),
                          ("more than thirty", ~listed & (lv < 3)), ("outside all grids", lv == 3)):
            for side, s2 in (("within the margin", within), ("clear", clear)):
                routes["%s, %s" % (key, side)] = routes.get("%s, %s" % (key, side), 0) + int(np.sum(sel_ & s2))
        routes["code"] = np.where(lv == 3, 3, np.where(~listed, 2, np.where(cnt > 15, 1, 0)))
    print("tables %s: %d steps, records with count <= 15: %d, 16..30: %d, 255 inside a grid: %d, outside: %d; tied rows not listed: %d" %
          (ev.name, q.shape[0], int(np.sum(listed & (cnt <= 15))), int(np.sum(listed & (cnt > 15))), int(np.sum(~listed & (lv < 3))),
           int(np.sum(lv == 3)), missing))
    assert missing == 0, ev.name


@pytest.mark.parametrize("name", dr.lane_cases())
def test_lane_layout(gpu, ob, name):
    """G = 32.  The speculation must hold on a probe image (a zero queue is the true one after at most one reset): nothing is repaired,
    so k_dither_lanes itself decided every probe -- and its tables say what they claim."""
    ev = dr.evaluated(ob, name)
    lay = ev.lay
    gpu.patolette_amd_dither_layout(1)
    assert gpu.patolette_amd_dither_layout_in_use(lay.width, lay.height, lay.pal.shape[0]) == 1
    got, st = _dither(gpu, lay.image, lay.width, lay.height, lay.pal)
    assert _report(name, "lanes", ev, got, st) == 0
    assert st["dither_segments"] > 1 and st["dither_repairs"] == 0 and st["dither_rounds"] == 1, st
    _check_tables(gpu, ev)


@pytest.mark.parametrize("name", dr.lane_cases())
def test_single_chain(gpu, ob, name):
    """patolette_amd_dither_config(1): the whole image in one chain of one wavefront, whatever the layout asked for"""
    ev = dr.evaluated(ob, name)
    lay = ev.lay
    gpu.patolette_amd_dither_layout(1)
    gpu.patolette_amd_dither_config(1, -1)
    got, st = _dither(gpu, lay.image, lay.width, lay.height, lay.pal)
    assert _report(name, "one chain", ev, got, st) == 0
    assert st["dither_segments"] == 1
    geom, amb = np.zeros(30), np.zeros(3, dtype=np.float32)
    assert gpu.patolette_amd_debug_dither_lane_tables(_dp(geom), amb.ctypes.data_as(C.POINTER(C.c_float)), None, 0) == -1   # not the lane layout


@pytest.mark.parametrize("name", dr.big_cases())
def test_lane_layout_with_64_cubed_grids(gpu, ob, name):
    """1024 x 1024: the first two grids have 64^3 cells; probes in the first 70 000 curve positions and at 3000 scattered ones"""
    ev = dr.evaluated(ob, name)
    lay = ev.lay
    gpu.patolette_amd_dither_layout(1)
    got, st = _dither(gpu, lay.image, lay.width, lay.height, lay.pal)
    assert _report(name, "lanes", ev, got, st) == 0
    assert st["dither_repairs"] == 0 and st["dither_rounds"] == 1, st
    _check_tables(gpu, ev)


REPAIR = ("ties-64-shuffled", "margin-64", "ties-128-grouped", "ties-255-shuffled", "ties-256-grouped", "margin-256", "crowded-256", "tiny-255")


@pytest.mark.parametrize("name", REPAIR)
def test_repair_kernel_decides_every_probe(gpu, ob, name):
    """no warm-up: every boundary fails its check; no stall passes: one wavefront alone walks through all runs with
    k_dither_lane_repair's step -- its PER = 1, 2 and 4 searches decide every probe"""
    ev = dr.evaluated(ob, name)
    lay = ev.lay
    gpu.patolette_amd_dither_layout(1)
    gpu.patolette_amd_dither_config(0, 0)
    gpu.patolette_amd_debug_dither_stall_passes(0)
    got, st = _dither(gpu, lay.image, lay.width, lay.height, lay.pal)
    assert _report(name, "lanes, every run repaired by a lone wavefront", ev, got, st) == 0
    assert st["dither_solo"] >= 1 and st["dither_segments"] > 1, st


def test_routes_of_the_lane_search_from_the_devices_own_tables(gpu, ob):
    """one image whose probes of four kinds are shuffled along the curve, so that the lanes of a step differ in class: what the
    kernel met, counted from the records it read"""
    ev = dr.evaluated(ob, "mixed-256")
    lay = ev.lay
    gpu.patolette_amd_dither_layout(1)
    got, st = _dither(gpu, lay.image, lay.width, lay.height, lay.pal)
    assert _report("mixed-256", "lanes", ev, got, st) == 0
    routes = {}
    _check_tables(gpu, ev, routes)
    code = routes.pop("code")
    for key in sorted(routes):
        print("%-44s %8d" % (key, routes[key]))
    assert len(routes) == 8
    for key, n in routes.items():
        assert n >= FLOOR, (key, n)
    # ... and mixed within wavefronts: the 64 lanes of a wavefront of k_dither_lanes walk 64 consecutive runs in lock step
    S, N = st["dither_segments"], code.shape[0]
    t = np.arange(S + 1, dtype=np.int64) * N // S
    mixed = 0
    for w0 in range(0, S, 64):
        b = np.arange(w0, min(S, w0 + 64))
        steps = int(np.min(t[b + 1] - t[b]))
        c = code[t[b][:, None] + np.arange(steps)[None, :]]
        mixed += int(np.sum(np.any(c != c[0:1], axis=0)))
    print("steps of a wavefront whose lanes differ in class: %d" % mixed)
    assert S >= 128 and mixed >= FLOOR


# ---- pixels that are not finite -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [v[0] for v in dr.NONFINITE])
@pytest.mark.parametrize("name,layout", (("margin-64", 0), ("margin-128", 0), ("margin-256", 0), ("margin-700", 0), ("margin-64", 1), ("margin-256", 1),
                                         ("margin-64", 2), ("margin-128", 2), ("margin-256", 2),
                                         ("margin-64", 3), ("margin-128", 3), ("margin-256", 3), ("margin-700", 3)))
def test_non_finite_pixels(gpu, ob, name, layout, variant):
    """one plane of six pixels NaN, +-Inf, 1e200 (every distance overflows), 1e39, or 1e308 twice in a row (finite pixels whose errors
    sum to +Inf): at a probe, mid-reset, and -- sixteen runs, their starts under either layout worked out (dither_ref.nonfinite_places)
    -- within the last sixteen pixels of a run and in the next run's warm-up.  The oracle keeps index 0 where every distance is NaN
    or +Inf, the chain recovers once the queue has turned over.  layout 2: the lane layout without warm-up and stall passes, so that
    a lone wavefront walks every run again with k_dither_lane_repair's step.  layout 3: the wavefront layout without warm-up, so that
    every boundary fails its check and k_dither's repair mode rebuilds its queue from the sixteen pixels before the run -- the pixel
    that is not finite among them -- and walks the run again."""
    ev = dr.evaluated(ob, name)
    lay, order = ev.lay, ev.order
    image = dr.with_nonfinite(lay, order, variant, dr.nonfinite_places(lay, util.dither_locate(_native, lay.width, lay.height)))
    want = ob.dither(image, lay.width, lay.height, lay.pal).astype(np.int64)
    lanes = 1 if layout in (1, 2) else 0
    gpu.patolette_amd_dither_layout(lanes)
    gpu.patolette_amd_dither_config(16, 0 if layout >= 2 else -1)
    if layout == 2:
        gpu.patolette_amd_debug_dither_stall_passes(0)
    assert gpu.patolette_amd_dither_layout_in_use(lay.width, lay.height, lay.pal.shape[0]) == lanes
    got, st = _dither(gpu, image, lay.width, lay.height, lay.pal)
    assert st["dither_segments"] == 16
    assert layout != 2 or st["dither_solo"] >= 1
    assert layout != 3 or (st["dither_repairs"] >= 15 and st["dither_rounds"] >= 2)      # every boundary was rebuilt from the map
    bad = np.nonzero(got != want)[0]
    print("dither %s with %s, layout %d: %d of %d differ from the oracle; %s" % (name, variant, layout, bad.size, got.size,
          {k_: st[k_] for k_ in ("dither_segments", "dither_repairs", "dither_rounds")}))
    if bad.size:
        rank = np.empty(got.size, dtype=np.int64)
        rank[order] = np.arange(got.size)
        r = np.sort(rank[bad])
        print("   curve ranks %s ..., got %s, oracle %s" % (r[:6], got[order[r[:6]]], want[order[r[:6]]]))
    assert bad.size == 0


# ---- last: the knobs are back ---------------------------------------------------------------------------------------------------------
def test_knobs_are_back_where_they_were(gpu, ob, untouched):
    flat, w, h, pal = _hygiene_input(ob)
    assert gpu.patolette_amd_dither_layout_in_use(w, h, 64) == 0           # 65 536 pixels: wavefronts by default
    assert gpu.patolette_amd_dither_layout_in_use(4096, 4096, 64) == 1
    assert gpu.patolette_amd_debug_dither_stall_passes(-1) == 2 and gpu.patolette_amd_debug_dither_solo_cap(-1) == 4096
    got, st = _dither(gpu, flat, w, h, pal)
    assert np.array_equal(got, untouched[0]) and st["dither_segments"] == untouched[1]
    assert np.array_equal(got, ob.dither(flat, w, h, pal).astype(np.int64))
