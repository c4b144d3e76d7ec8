"""remap_rgba / patolette_amd_remap_rgba_u8 and quantize_rgba_frames on the device against tests/rgba_remap_ref.py (numpy on the CPU
oracle).  Every comparison is bit for bit over every element of map and quantized, none excluded.

The nearest and the ordered mode compare distances the device computes with its own pow (0.52 ulp from glibc's), so -- as in
tests/test_gpu_ordered.py and for the same reason -- each of their cases first asserts that the REFERENCE's smallest relative gap
between the best and the second-best row, over all pixels, is at least 1e-9.  If another seed trips that, change the seed, not the bar.

Sizes: (40, 56); three frames of (37, 53) = 1961 pixels, so no frame but the first starts on a vector boundary of the stamp and the
stack's 5883 pixels leave a tail of three; (1, 1); (301, 1) x 2; (263, 301) x 2 for the per-pixel modes (the Python walk is too slow
there).  Rows (transparent row included): 2, 3, 17, 256, 257 (the elements' widths change) and 1030 (the stamp's palette leaves LDS)."""
import ctypes as C
import functools

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import rgba_remap_ref
from tests.test_gpu_remap import _content, _palette
from tests.util import ROOT

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-9
NEAREST, RIEMERSMA, ORDERED = rgba_remap_ref.NEAREST, rgba_remap_ref.RIEMERSMA, rgba_remap_ref.ORDERED
DITHER = {NEAREST: False, RIEMERSMA: True, ORDERED: "ordered"}
GEOMETRY = [((40, 56), 1), ((37, 53), 3), ((1, 1), 1), ((301, 1), 2), ((263, 301), 2)]
ALPHAS = ["none", "all", "disc", "half", "frame", "edge"]


@pytest.fixture(autouse=True)
def _defaults(gpu):
    yield
    gpu.patolette_amd_debug_rgba_stamp_quad(-1)
    gpu.patolette_amd_debug_remap_two_pass(0)
    _native.profile(False)


def _alpha(kind, frames, h, w, seed, thr=128):
    rng = np.random.default_rng(seed)
    a = np.full((frames, h, w), 255, dtype=np.uint8)
    if kind == "all":
        a[:] = 0
    elif kind == "disc":                                             # opaque inside a disc, soft values around its edge
        yy, xx = np.mgrid[0:h, 0:w]
        r = np.hypot((yy - (h - 1) / 2) / max(h, 2), (xx - (w - 1) / 2) / max(w, 2))
        a[:] = np.clip((0.42 - r) * 1200 + 128, 0, 255).astype(np.uint8)[None]
    elif kind == "half":
        a[:] = np.where(rng.random((frames, h, w)) < 0.5, 0, 255)
    elif kind == "frame":                                            # one fully transparent frame among others
        a[:] = np.where(rng.random((frames, h, w)) < 0.3, 0, 255)
        a[frames // 2] = 0
    elif kind == "edge":                                             # exactly threshold - 1 and threshold
        a[:] = np.where(rng.random((frames, h, w)) < 0.5, max(thr - 1, 0), min(thr, 255))
    else:
        assert kind == "none"
    return a


@functools.lru_cache(maxsize=None)
def _case(size, frames, alpha, rows, form="rgba", seed=5, thr=128, kind="scene"):
    """(image (F,H,W,4) or (H,W,4), palette in `form`, transparent_index to pass); rows counts the transparent row when there is one."""
    h, w = size
    rgb = np.stack([_content(kind, h, w, seed + 7 * i) for i in range(frames)])
    image = np.concatenate([rgb, _alpha(alpha, frames, h, w, seed, thr)[..., None]], axis=-1)
    image = image if frames > 1 else image[0]
    colours = _palette(rows - 1, seed=seed)
    if form == "rgba":
        pal, tidx = np.zeros((rows + 2, 4), dtype=np.uint8), None    # two trailing unused rows
        pal[1:rows, :3], pal[1:rows, 3] = colours, 255
    elif form == "u8":
        pal, tidx = np.concatenate([np.array([[9, 9, 9]], dtype=np.uint8), colours]), 0   # (row 0's colour is never a candidate)
    else:
        assert form == "float"
        pal, tidx = np.full((rows + 3, 3), -1.0), 0                  # three trailing unused rows
        pal[0], pal[1:rows] = 0.0, colours / 255.0
        pal = np.asfortranarray(pal)
    image.setflags(write=False)
    pal.setflags(write=False)
    return image, pal, tidx


@functools.lru_cache(maxsize=None)
def _reference(size, frames, alpha, rows, mode, form="rgba", seed=5, thr=128, spread=None, kind="scene"):
    """(map, quantized) of the reference for _case(...), computed once and left unchanged; the gap condition is asserted here."""
    from oracle import binding as ob
    image, pal, tidx = _case(size, frames, alpha, rows, form, seed, thr, kind)
    m, q, gap = rgba_remap_ref.remap_rgba(ob, image, pal, tidx, thr, mode, spread, want_gap=True)
    if mode != RIEMERSMA:
        print("reference %s x%d %s rows %d mode %d: smallest relative gap %.3g" % (size, frames, alpha, rows, mode, gap))
        assert gap >= MIN_GAP
    m.setflags(write=False)
    q.setflags(write=False)
    return m, q


def _same(m, q, m_ref, q_ref):
    m = np.asarray(m)
    mism = int(np.sum(m.astype(np.int64) != m_ref)) if m.shape == m_ref.shape else -1
    print("remap_rgba: %d of %d elements differ from the reference" % (mism, m_ref.size))
    assert m.shape == m_ref.shape and mism == 0
    if q is not None:
        assert q.shape == q_ref.shape and np.array_equal(q, q_ref)


def _run(image, pal, tidx, mode, thr=128, spread=None, **kw):
    ok, m, q, msg = patolette_amd.remap_rgba(image, pal, tidx, thr, DITHER[mode], spread=spread, **kw)
    assert ok, msg
    return m, q


def _both_stamp_paths(gpu, image, pal, tidx, mode, m_ref, q_ref, thr=128, spread=None):
    for quad in (0, 1):
        gpu.patolette_amd_debug_rgba_stamp_quad(quad)
        _same(*_run(image, pal, tidx, mode, thr, spread), m_ref, q_ref)
    gpu.patolette_amd_debug_rgba_stamp_quad(-1)


@pytest.mark.parametrize("mode", [NEAREST, RIEMERSMA, ORDERED])
@pytest.mark.parametrize("size,frames", GEOMETRY, ids=lambda v: str(v).replace(" ", ""))
def test_geometry(gpu, size, frames, mode):
    if mode == RIEMERSMA and size == (263, 301):
        size, frames = (40, 56), 2                                   # (the Python walk is too slow at that size: two small frames instead)
    m_ref, q_ref = _reference(size, frames, "half", 17, mode)
    image, pal, tidx = _case(size, frames, "half", 17)
    m, q = _run(image, pal, tidx, mode)
    assert m.dtype == np.uint8 and q.dtype == np.uint8 and q.shape == image.shape
    _same(m, q, m_ref, q_ref)
    if mode != RIEMERSMA:
        _both_stamp_paths(gpu, image, pal, tidx, mode, m_ref, q_ref)
    if frames > 1:                                                   # no state passes between frames
        for i in range(frames):
            mi, qi = _run(image[i], pal, tidx, mode)
            assert np.array_equal(mi, m[i]) and np.array_equal(qi, q[i])


@pytest.mark.parametrize("mode", [NEAREST, RIEMERSMA, ORDERED])
@pytest.mark.parametrize("rows", [2, 3, 17, 256, 257, 1030])
def test_rows(gpu, rows, mode):
    size, frames = ((37, 53), 3) if mode != RIEMERSMA else ((40, 56), 1)
    kind = "noise" if rows > 17 else "scene"                         # (noise reaches every part of a large palette)
    m_ref, q_ref = _reference(size, frames, "disc", rows, mode, kind=kind)
    image, pal, tidx = _case(size, frames, "disc", rows, kind=kind)
    m, q = _run(image, pal, tidx, mode)
    assert m.dtype == (np.uint8 if rows + 2 <= 256 else np.uint16)   # sized by the rows as given (two trailing unused ones)
    _same(m, q, m_ref, q_ref)
    assert m_ref.max() <= rows - 1 and (rows == 2 or len(np.unique(m_ref)) > 2)
    if mode != RIEMERSMA:
        _both_stamp_paths(gpu, image, pal, tidx, mode, m_ref, q_ref)


@pytest.mark.parametrize("mode", [NEAREST, RIEMERSMA, ORDERED])
def test_palette_forms(gpu, mode):
    size, frames, rows = (40, 56), 1, 17
    m_ref, q_ref = _reference(size, frames, "disc", rows, mode)
    for form in ("rgba", "u8", "float"):
        image, pal, tidx = _case(size, frames, "disc", rows, form)
        from oracle import binding as ob
        m_own, q_own, _ = rgba_remap_ref.remap_rgba(ob, image, pal, tidx, 128, mode)
        assert np.array_equal(m_own, m_ref)                          # the three forms name one palette
        m, q = _run(image, pal, tidx, mode)
        _same(m, q, m_ref, q_own)
        assert m.dtype == np.uint8
    image, pal, tidx = _case(size, frames, "disc", rows, "float")
    m, q = _run(image, np.ascontiguousarray(pal), tidx, mode)        # any layout of the float palette
    _same(m, None, m_ref, None)


@pytest.mark.parametrize("mode", [NEAREST, RIEMERSMA, ORDERED])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_alpha_patterns(gpu, alpha, mode):
    size, frames = (37, 53), 3
    m_ref, q_ref = _reference(size, frames, alpha, 17, mode)
    image, pal, tidx = _case(size, frames, alpha, 17)
    opaque = image[..., 3] >= 128
    assert {"none": opaque.all(), "all": not opaque.any()}.get(alpha, opaque.any() and not opaque.all())
    if alpha == "frame":
        assert not opaque[1].any() and opaque[0].any() and opaque[2].any()
    if alpha == "edge":
        assert set(np.unique(image[..., 3])) == {127, 128}
    m, q = _run(image, pal, tidx, mode)
    _same(m, q, m_ref, q_ref)
    assert np.all(np.asarray(m)[~opaque] == 0) and not q[~opaque].any() and np.all(q[opaque][:, 3] == 255)
    if mode != RIEMERSMA:
        _both_stamp_paths(gpu, image, pal, tidx, mode, m_ref, q_ref)
    if alpha == "none":                                              # the RGB remap of the same pixels, plus the offset
        rgb_pal = np.ascontiguousarray(pal[1:17, :3])
        ok, m3, q3, msg = patolette_amd.remap(image, rgb_pal, dither=DITHER[mode])
        assert ok, msg
        assert np.array_equal(m, m3 + 1) and np.array_equal(q[..., :3], q3)
        m0, q0 = _run(image, rgb_pal, -1, mode)                      # ... and without a transparent entry, without it
        assert np.array_equal(m0, m3) and np.array_equal(q0[..., :3], q3) and np.all(q0[..., 3] == 255)


@pytest.mark.parametrize("mode", [NEAREST, RIEMERSMA, ORDERED])
@pytest.mark.parametrize("thr", [0, 1, 128, 256])
def test_thresholds(gpu, thr, mode):
    size, frames = (40, 56), 1
    m_ref, q_ref = _reference(size, frames, "disc", 17, mode, thr=thr)
    image, pal, tidx = _case(size, frames, "disc", 17, thr=thr)
    assert (image[..., 3] == 0).any() and (image[..., 3] == 255).any()
    m, q = _run(image, pal, tidx, mode, thr)
    _same(m, q, m_ref, q_ref)
    if thr == 0:
        assert np.asarray(m).min() >= 1
    if thr == 256:
        assert not np.asarray(m).any() and not q.any()


def test_spread(gpu):
    size, frames = (37, 53), 3
    image, pal, tidx = _case(size, frames, "half", 17)
    m0, q0 = _run(image, pal, tidx, ORDERED, spread=0)
    mn, qn = _run(image, pal, tidx, NEAREST)
    assert np.array_equal(m0, mn) and np.array_equal(q0, qn)        # spread 0 is the nearest mode, bit for bit
    _same(m0, q0, *_reference(size, frames, "half", 17, NEAREST))
    _same(*_run(image, pal, tidx, ORDERED, spread=4.0), *_reference(size, frames, "half", 17, ORDERED, spread=4.0))
    md, qd = _run(image, pal, tidx, ORDERED)
    default = patolette_amd.ordered_spread(np.ascontiguousarray(pal[1:17, :3]))        # of the opaque rows
    ms, qs = _run(image, pal, tidx, ORDERED, spread=default)
    assert default > 0 and np.array_equal(md, ms) and np.array_equal(qd, qs) and np.any(md != m0)
    _same(md, qd, *_reference(size, frames, "half", 17, ORDERED))


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c_call(gpu, image, pal8=None, palf=None, rows=None, tidx=0, mode=NEAREST, thr=128, spread=0.0, pmap=None, elem=1, quant=None, frames=None,
            width=None, height=None):
    fr = image if image.ndim == 4 else image[None]
    code = C.c_int(7)
    gpu.patolette_amd_remap_rgba_u8(fr.shape[0] if frames is None else frames, fr.shape[2] if width is None else width,
                                    fr.shape[1] if height is None else height, _vp(image), thr,
                                    None if palf is None else palf.ctypes.data_as(_native.dp), _vp(pal8),
                                    (pal8 if pal8 is not None else palf).shape[0] if rows is None else rows, tidx, mode, spread, _vp(pmap), elem,
                                    _vp(quant), C.byref(code))
    return code.value


@pytest.mark.parametrize("mode", [NEAREST, RIEMERSMA, ORDERED])
def test_elements_and_outputs(gpu, mode):
    """Every element size and every output alone, through the C entry; the statistics of a remap."""
    size, frames = (37, 53), 3
    image, pal, tidx = _case(size, frames, "half", 17, "u8")
    spread = 0.2 if mode == ORDERED else None
    m_ref, q_ref = _reference(size, frames, "half", 17, mode, "u8", spread=spread)
    for eb, dt in ((1, np.uint8), (2, np.uint16), (4, np.uint32), (8, np.uint64)):
        pmap, quant = np.full(m_ref.shape, 99, dtype=dt), np.full(q_ref.shape, 99, dtype=np.uint8)
        assert _c_call(gpu, image, pal8=pal, mode=mode, spread=spread or 0.0, pmap=pmap, elem=eb, quant=quant) == 0
        _same(pmap, quant, m_ref, q_ref)
        if mode != RIEMERSMA:
            gpu.patolette_amd_debug_rgba_stamp_quad(0)
            pmap[:] = 99
            assert _c_call(gpu, image, pal8=pal, mode=mode, spread=spread or 0.0, pmap=pmap, elem=eb) == 0      # the map alone
            gpu.patolette_amd_debug_rgba_stamp_quad(-1)
            _same(pmap, None, m_ref, None)
    st = patolette_amd.last_stats()
    assert st["ms_total"] > 0 and st["ms_map"] > 0
    assert st["n_clusters"] == 0 and st["ms_kmeans"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0
    if mode != RIEMERSMA:
        assert all(st[key] == 0 for key in st if key.startswith("dither_"))
    else:
        assert st["dither_segments"] >= frames                       # summed over the frames
    quant = np.full(q_ref.shape, 99, dtype=np.uint8)
    assert _c_call(gpu, image, pal8=pal, mode=mode, spread=spread or 0.0, quant=quant, elem=0) == 0             # quantized alone
    assert np.array_equal(quant, q_ref)
    assert _c_call(gpu, image, pal8=pal, mode=mode, spread=spread or 0.0) == 0                                   # no output at all
    m, q = _run(image, pal, tidx, mode, spread=spread, want_quantized=False)
    assert q is None
    _same(m, None, m_ref, None)


def test_two_pass_route_and_one_stamp_launch(gpu):
    """The nearest mode through the conversion fall-back and, where it applies, the fused kernel: the same bits; one launch of
    k_rgba_stamp per call for all frames, none in the Riemersma mode."""
    size, frames = (37, 53), 3
    image, pal, tidx = _case(size, frames, "half", 17)
    for mode in (NEAREST, ORDERED, RIEMERSMA):
        m_ref, q_ref = _reference(size, frames, "half", 17, mode)
        for two_pass in (0, 1):
            gpu.patolette_amd_debug_remap_two_pass(two_pass)
            _native.profile(True)
            m, q = _run(image, pal, tidx, mode)
            prof = _native.profile_results()
            _native.profile(False)
            _same(m, q, m_ref, q_ref)
            print("mode %d two_pass %d: %s" % (mode, two_pass, sorted(prof)))
            if mode == RIEMERSMA:
                assert "k_rgba_stamp" not in prof and prof["k_rgba_expand"]["launches"] == frames and prof["k_alpha_count"]["launches"] == frames
            else:
                assert prof["k_rgba_stamp"]["launches"] == 1 and "k_rgba_expand" not in prof
                assert ("k_ordered_map" in prof) == (mode == ORDERED)
    gpu.patolette_amd_debug_remap_two_pass(0)


def test_round_trip(gpu):
    """quantize_rgba, then its quantized image remapped onto its palette_rgba: the map comes back."""
    image, _, _ = _case((40, 56), 1, "disc", 17)
    ok, prgba, pmap, quant, pal, tidx, msg = patolette_amd.quantize_rgba(image, 16, dither=False, tile_size=0, kmeans_niter=2,
                                                                         kmeans_max_samples=4096)
    assert ok and tidx == 0, msg
    used = prgba[prgba[:, 3] == 255]
    assert len({tuple(r) for r in used[:, :3]}) == len(used) > 4     # distinct byte rows: an index is defined by its colour
    ok, m, q, msg = patolette_amd.remap_rgba(quant, prgba, dither=False)
    assert ok, msg
    assert np.array_equal(m, pmap) and np.array_equal(q, quant) and m.dtype == pmap.dtype


KW = dict(tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)


@pytest.mark.parametrize("frames", [1, 3])
def test_quantize_rgba_frames(gpu, frames, ob):
    size = (40, 56)
    image, _, _ = _case(size, 3, "half", 17)
    stack = np.ascontiguousarray(image[:frames])
    n = frames * size[0] * size[1]
    w = np.random.default_rng(3).random(n) + 0.5
    # explicit weights: the palette of quantize_rgba on the stacked image with the same weights
    ok, prgba, maps, quant, pal, tidx, msg = patolette_amd.quantize_rgba_frames(stack, 16, dither=False, weights=w, **KW)
    assert ok and tidx == 0, msg
    ok, prgba1, _, _, pal1, tidx1, msg = patolette_amd.quantize_rgba(stack.reshape(frames * size[0], size[1], 4), 16, dither=False, weights=w, **KW)
    assert ok and tidx1 == 0, msg
    assert np.array_equal(prgba, prgba1) and np.array_equal(pal, pal1)
    assert maps.shape == (frames,) + size and maps.dtype == np.uint8 and quant.shape == (frames,) + size + (4,)
    assert np.array_equal(quant, prgba[maps])
    # the maps: the reference remap of the RETURNED palette, in every mode
    for dither, mode in ((False, NEAREST), (True, RIEMERSMA), ("ordered", ORDERED)):
        ok, prgba2, maps, quant, pal2, tidx, msg = patolette_amd.quantize_rgba_frames(stack, 16, dither=dither, weights=w, **KW)
        assert ok and tidx == 0 and np.array_equal(pal2, pal) and np.array_equal(prgba2, prgba), msg
        m_ref, q_ref, gap = rgba_remap_ref.remap_rgba(ob, stack, pal, 0, 128, mode, want_gap=True)
        assert mode == RIEMERSMA or gap >= MIN_GAP
        _same(maps, quant, m_ref, q_ref)
        assert np.array_equal(quant, prgba[maps])
    # palette_only: the palette alone
    ok, prgba_po, m_none, q_none, pal_po, tidx, msg = patolette_amd.quantize_rgba_frames(stack, 16, palette_only=True, weights=w, **KW)
    assert ok and m_none is None and q_none is None and tidx == 0 and prgba_po.shape == (16, 4) and pal_po.shape == (16, 3), msg
    # all-opaque frames: the palette of quantize_frames
    opaque = stack.copy()
    opaque[..., 3] = 255
    ok, prgba_o, maps_o, _, pal_o, tidx, msg = patolette_amd.quantize_rgba_frames(opaque, 16, dither=False, **KW)
    assert ok and tidx == -1, msg
    ok, p8, _, _, p64, msg = patolette_amd.quantize_frames(opaque, 16, dither=False, **KW)
    assert ok, msg
    assert np.array_equal(pal_o, p64) and np.array_equal(prgba_o[:, :3], p8) and np.all(prgba_o[p8.any(axis=1), 3] == 255)
    assert np.asarray(maps_o).max() <= 15
    # all-transparent frames: entry 0 throughout
    clear = stack.copy()
    clear[..., 3] = 0
    ok, prgba_c, maps_c, quant_c, _, tidx, msg = patolette_amd.quantize_rgba_frames(clear, 16, dither=True, **KW)
    assert ok and tidx == 0 and not maps_c.any() and not quant_c.any() and not prgba_c.any(), msg


def test_quantize_rgba_frames_derives_weights_per_frame(gpu):
    h, w = 90, 120
    stack = np.ascontiguousarray(_case((h, w), 3, "half", 17)[0])
    per = [patolette_amd.saliency_weights(w, h, stack[f, :, :, :3].reshape(h * w, 3) / 255.0, 64) for f in range(3)]
    kw = dict(kmeans_niter=2, kmeans_max_samples=4096, dither=False)
    ok, prgba, maps, _, pal, tidx, msg = patolette_amd.quantize_rgba_frames(stack, 16, tile_size=64, **kw)
    assert ok, msg
    ok, prgba2, maps2, _, pal2, tidx2, msg = patolette_amd.quantize_rgba_frames(stack, 16, tile_size=0, weights=np.concatenate(per), **kw)
    assert ok, msg
    assert np.array_equal(pal, pal2) and np.array_equal(prgba, prgba2) and np.array_equal(maps, maps2) and tidx == tidx2 == 0


def test_downstream_measure_and_frame_deltas(gpu):
    image, pal, tidx = _case((37, 53), 3, "half", 17)
    m, q = _run(image, pal, tidx, ORDERED)
    opaque = image[..., 3] >= 128
    ok, entries, per_frame, _, msg = patolette_amd.measure(image, m, pal[:, :3], skip_index=0)
    assert ok, msg
    assert np.array_equal(per_frame[:, 0], opaque.reshape(3, -1).sum(axis=1)) and entries[0, 0] == 0
    assert entries[:, 0].sum() == opaque.sum()
    ok, deltas, rects, changed, shown, msg = patolette_amd.frame_deltas(m, 19, want_shown=True)     # exact: index 0 compares like any row
    assert ok, msg
    assert np.array_equal(shown, m) and np.array_equal(deltas[0], m[0]) and changed[0] == m[0].size
    assert np.array_equal(changed[1:], (m[1:] != m[:-1]).reshape(2, -1).sum(axis=1))


def test_errors_and_recovery(gpu):
    size = (40, 56)
    h, w = size
    image, pal, tidx = _case(size, 1, "half", 17, "u8")
    m_ref, q_ref = _reference(size, 1, "half", 17, NEAREST, "u8")
    palf = np.asfortranarray(pal.astype(np.float64) / 255.0)
    pmap = np.zeros(size, dtype=np.uint8)

    def good():
        pmap[:] = 255
        assert _c_call(gpu, image, pal8=pal, pmap=pmap) == 0
        _same(pmap, None, m_ref, None)

    def failed(code, want=-1, text=None):
        assert code == want
        if want == -1:
            assert _native.last_error().startswith("patolette_amd_remap_rgba:"), _native.last_error()
        if text:
            assert text in _native.last_error(), _native.last_error()
        good()

    good()
    # the flag: a transparent pixel and no transparent entry, in every mode, map wanted or not
    for mode in (NEAREST, RIEMERSMA, ORDERED):
        failed(_c_call(gpu, image, pal8=pal, tidx=-1, mode=mode, pmap=pmap), text="no transparent entry")
        failed(_c_call(gpu, image, pal8=pal, tidx=-1, mode=mode), text="no transparent entry")
        with pytest.raises(ValueError, match="no transparent entry"):
            patolette_amd.remap_rgba(image, pal, -1, dither=DITHER[mode])
        good()
        assert _c_call(gpu, image, pal8=pal, tidx=-1, mode=mode, thr=0, pmap=pmap) == 0       # nothing transparent: fine
    failed(_c_call(gpu, image, pal8=pal, mode=3, pmap=pmap), text="mode")
    failed(_c_call(gpu, image, pal8=pal, mode=-1, pmap=pmap), text="mode")
    failed(_c_call(gpu, image, pal8=pal, thr=257, pmap=pmap), text="alpha_threshold")
    failed(_c_call(gpu, image, pal8=pal, thr=-1, pmap=pmap), text="alpha_threshold")
    failed(_c_call(gpu, image, pal8=pal, tidx=1, pmap=pmap), text="transparent_index")
    failed(_c_call(gpu, image, pal8=pal, tidx=-2, pmap=pmap), text="transparent_index")
    failed(_c_call(gpu, image, pal8=pal, palf=palf, pmap=pmap), text="exactly one")
    failed(_c_call(gpu, image, rows=17, pmap=pmap), text="exactly one")
    failed(_c_call(gpu, image, pal8=pal, rows=0, pmap=pmap))
    failed(_c_call(gpu, image, pal8=pal, pmap=pmap, elem=3), text="map_elem_bytes")
    wide = np.zeros((257, 3), dtype=np.uint8)
    failed(_c_call(gpu, image, pal8=wide, pmap=pmap, elem=1), text="map_elem_bytes")
    failed(_c_call(gpu, image, pal8=pal[:1], pmap=pmap), text="no opaque")
    bad = palf.copy(order="F")
    bad[3, 1] = np.nan
    failed(_c_call(gpu, image, palf=bad, pmap=pmap), text="finite")
    failed(_c_call(gpu, image, palf=np.full((17, 3), -1.0, order="F"), pmap=pmap), text="unused-row")
    only0 = np.full((17, 3), -1.0, order="F")
    only0[0] = 0.0
    failed(_c_call(gpu, image, palf=only0, pmap=pmap), text="no opaque")
    for spread in (float("nan"), float("inf"), -0.25):
        failed(_c_call(gpu, image, pal8=pal, mode=ORDERED, spread=spread, pmap=pmap), text="spread")
    assert _c_call(gpu, image, pal8=pal, mode=NEAREST, spread=float("nan"), pmap=pmap) == 0     # read in the ordered mode only
    code = C.c_int(7)
    gpu.patolette_amd_remap_rgba_u8(1, w, h, None, 128, None, _vp(pal), 17, 0, 0, 0.0, _vp(pmap), 1, None, C.byref(code))
    failed(code.value, text="no pixels")
    failed(_c_call(gpu, image, pal8=pal, pmap=pmap, width=0), want=-2)
    failed(_c_call(gpu, image, pal8=pal, pmap=pmap, height=0), want=-2)
    failed(_c_call(gpu, image, pal8=pal, pmap=pmap, frames=0), want=-2)
    failed(_c_call(gpu, image, pal8=pal, pmap=pmap, frames=1 << 31), want=-4, text="too big")
    failed(_c_call(gpu, image, pal8=pal, pmap=pmap, mode=RIEMERSMA, frames=1 << 20), want=-4, text="2^31")
    failed(_c_call(gpu, image, pal8=pal, pmap=pmap, width=40001, height=40001), want=-4)


def test_workspace_history(gpu):
    """The same bits on a second call, after a larger call, and from a fresh workspace; no growth behind queued work."""
    size, frames = (37, 53), 3
    image, pal, tidx = _case(size, frames, "half", 17)
    other, pal_o, tidx_o = _case((96, 80), 4, "disc", 257, seed=9, kind="noise")
    for mode in (NEAREST, RIEMERSMA, ORDERED):
        gpu.patolette_amd_release_workspace()
        fresh, fresh_q = _run(image, pal, tidx, mode)
        _same(fresh, fresh_q, *_reference(size, frames, "half", 17, mode))
        gpu.patolette_amd_release_workspace()
        prev = gpu.patolette_amd_debug_workspace(1 | 2)
        try:
            before = gpu.patolette_amd_debug_late_growths()
            m1, q1 = _run(image, pal, tidx, mode)
            m2, q2 = _run(image, pal, tidx, mode)
            _run(other, pal_o, tidx_o, mode)
            ok, *_ = patolette_amd.quantize_rgba(other[0], 16, dither=True, **KW)
            assert ok
            m3, q3 = _run(image, pal, tidx, mode)
            assert gpu.patolette_amd_debug_late_growths() == before
        finally:
            gpu.patolette_amd_debug_workspace(prev)
            gpu.patolette_amd_release_workspace()
        for m, q in ((m1, q1), (m2, q2), (m3, q3)):
            assert np.array_equal(m, fresh) and np.array_equal(q, fresh_q)


def test_torch_flavour(gpu):
    """A torch CUDA tensor goes through patolette_amd_remap_rgba_u8_device: the numpy flavour's results, outputs on the input's device,
    pixels at an odd address included.  Own process: torch loads its HIP runtime before libpatolette_amd.so does."""
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
from tests.test_gpu_rgba_remap import _case, DITHER
for rows in (17, 300):
    image, pal, tidx = _case((37, 53), 3, "half", rows)
    t = torch.from_numpy(np.array(image)).cuda()
    for mode in (0, 1, 2):
        ok, m, q, msg = p.remap_rgba(image, pal, tidx, dither=DITHER[mode])
        assert ok, msg
        ok, mt, qt, msg = p.remap_rgba(t, pal, tidx, dither=DITHER[mode])
        assert ok, msg
        assert mt.device == t.device and qt.device == t.device
        assert mt.dtype == (torch.uint8 if rows + 2 <= 256 else torch.int32) and tuple(mt.shape) == m.shape
        assert np.array_equal(mt.cpu().numpy().astype(np.int64), m.astype(np.int64))
        assert np.array_equal(qt.cpu().numpy(), q)
        ok, mt2, qt2, msg = p.remap_rgba(t, torch.from_numpy(np.array(pal)), tidx, dither=DITHER[mode], want_quantized=False)
        assert ok and qt2 is None and np.array_equal(mt2.cpu().numpy(), mt.cpu().numpy())
        flat = torch.zeros(t.numel() + 1, dtype=torch.uint8, device=t.device)
        flat[1:] = t.reshape(-1)
        ok, mo, qo, msg = p.remap_rgba(flat[1:].reshape(t.shape), pal, tidx, dither=DITHER[mode])      # pixels not 4-byte aligned
        assert ok and np.array_equal(mo.cpu().numpy(), mt.cpu().numpy()) and np.array_equal(qo.cpu().numpy(), q), msg
    try:
        p.remap_rgba(t, np.ascontiguousarray(pal[1:rows, :3]), -1, dither=False)
    except ValueError as e:
        assert "no transparent entry" in str(e)
    else:
        raise AssertionError("no ValueError")
    ok, prgba, maps, quant, pal64, ti, msg = p.quantize_rgba_frames(t, 16, dither="ordered", tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
    assert ok and ti == 0 and maps.device == t.device and quant.device == t.device, msg
    ok, prgba2, maps2, quant2, _, _, msg = p.quantize_rgba_frames(image, 16, dither="ordered", tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
    assert ok and np.array_equal(prgba, prgba2) and np.array_equal(maps.cpu().numpy(), maps2) and np.array_equal(quant.cpu().numpy(), quant2), msg
print("TORCH-RGBA-REMAP-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-RGBA-REMAP-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
