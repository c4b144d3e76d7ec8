"""frame_deltas_local / patolette_amd_frame_deltas_local on the device against tests/local_delta_ref.py (numpy on the CPU oracle).

Every comparison with the reference is bit for bit over all elements of deltas, shown_rgb, rects and changed.  As in test_gpu_delta.py
a lossy comparison means something only away from the threshold: every lossy case first asserts that the REFERENCE's smallest relative
gap |D - tol^2| / tol^2 is at least 1e-9.  The seeds below were checked on the CPU for that (smallest gap met: see _reference's print).

The maps are the reference's own nearest maps (tests/remap_ref.py, the statement of `remap`) of every frame onto its table, made on
the CPU: no other device stage is involved.  Shapes: test_gpu_delta.py's smallest -- (40, 56) x 5; (37, 53) x 4, no multiple of 64;
(263, 301) x 6, where ballot words wrap rows; (36, 301) x 4, a multiple of 4 with an odd width (the four-position route when forced);
(1, 70) and (65, 1)."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import delta_ref, local_delta_ref, lzw_ref
from tests.test_gpu_remap import _image, _palette
from tests.util import ROOT, scene

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-9
SIZES = {"small": ((40, 56), 5), "odd64": ((37, 53), 4), "wrap": ((263, 301), 6), "quad": ((36, 301), 4)}
PREFIX = "patolette_amd_frame_deltas_local:"
TOLERANCES = (0.0, 0.02, 0.05)


@pytest.fixture(autouse=True)
def _defaults_again(gpu):
    yield
    _native.profile(False)
    gpu.patolette_amd_debug_delta_quad(-1)
    gpu.patolette_amd_debug_delta_local_tables(-1)


@functools.lru_cache(maxsize=None)
def _clip(size, F):
    frames = delta_ref.clip(size[0], size[1], F)
    frames.setflags(write=False)
    return frames


def _tables(kind, F):
    """(number of tables, the frames' tables or None) for "one" (P == 1), "each" (P == F) and "pairs" (P == 2: 0, 0, 1, 1, ...)."""
    if kind == "one":
        return 1, [0] * F
    if kind == "each":
        return F, None
    assert kind == "pairs"
    return 2, [(f // 2) % 2 for f in range(F)]


@functools.lru_cache(maxsize=None)
def _case(size, F, K, kind):
    """(palettes (P, K, 3) of random bytes, palette_of, the reference's nearest maps of every frame onto its table), computed once."""
    from oracle import binding as ob
    P, of = _tables(kind, F)
    palettes = np.stack([_palette(K, seed=2 + 5 * g) for g in range(P)])
    g_of = list(range(F)) if of is None else of
    frames = _clip(size, F)
    maps = np.stack([delta_ref.maps_of(ob, frames[f:f + 1], palettes[g_of[f]], "nearest")[0] for f in range(F)]).astype(np.uint8)
    palettes.setflags(write=False)
    maps.setflags(write=False)
    return palettes, of, maps


@functools.lru_cache(maxsize=None)
def _reference(size, F, K, kind, tolerance):
    from oracle import binding as ob
    palettes, of, maps = _case(size, F, K, kind)
    d, s, r, c, gap, tested, kept = local_delta_ref.frame_deltas(ob, maps, palettes, of, frames=_clip(size, F), tolerance=tolerance)
    print("local delta reference: %s F %d K %d %s tolerance %g: %d distances, %d kept, smallest relative gap %.3g"
          % (size, F, K, kind, tolerance, tested, kept, gap))
    if tolerance > 0:
        assert gap >= MIN_GAP
    for a in (d, s, r, c):
        a.setflags(write=False)
    return d, s, r, c, tested, kept


def _same(got, ref):
    """got: (deltas, rects, changed, shown_rgb) of the device; ref: the reference's tuple."""
    d, r, c, s = got
    d_ref, s_ref, r_ref, c_ref = ref[:4]
    assert d.shape == d_ref.shape and s.shape == s_ref.shape and r.shape == r_ref.shape and c.shape == c_ref.shape
    wrong = [int(np.sum(np.asarray(a).astype(np.int64) != b)) for a, b in ((d, d_ref), (s, s_ref), (r, r_ref), (c, c_ref))]
    print("deltas / shown_rgb / rects / changed: %s of %s differ from the reference" % (wrong, [d_ref.size, s_ref.size, r_ref.size, c_ref.size]))
    assert wrong == [0, 0, 0, 0]
    assert d.dtype == np.uint8 and s.dtype == np.uint8 and r.dtype == np.int32 and c.dtype == np.int64


@pytest.mark.parametrize("kind", ["one", "each", "pairs"])
@pytest.mark.parametrize("K", [2, 16, 255])
@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_tables_and_tolerances(gpu, name, K, kind):
    size, F = SIZES[name]
    palettes, of, maps = _case(size, F, K, kind)
    for tolerance in TOLERANCES:
        ref = _reference(size, F, K, kind, tolerance)
        if tolerance > 0 and K >= 16:
            assert 0 < ref[5] < ref[4]                                 # both outcomes occur
        ok, d, r, c, s, msg = patolette_amd.frame_deltas_local(maps, palettes, of, frames=_clip(size, F), tolerance=tolerance, want_shown=True)
        assert ok, msg
        _same((d, r, c, s), ref)
        assert np.array_equal(local_delta_ref.replay_rgb(d, palettes, of, K), s)                  # consequence (a)
        if tolerance == 0:
            g_of = list(range(F)) if of is None else of
            assert all(np.array_equal(s[f], palettes[g_of[f]][maps[f]]) for f in range(F))         # consequence (b)
    if K == 255:
        assert np.any(d == 255)                                        # T == 255 with K == 255


@pytest.mark.parametrize("tolerance", TOLERANCES)
def test_four_positions_per_lane_and_both_table_routes(gpu, tolerance):
    """(36, 301): the four-position route forced against the one-position route, each with the tables in LDS and in global memory."""
    size, F = SIZES["quad"]
    palettes, of, maps = _case(size, F, 16, "pairs")
    ref = _reference(size, F, 16, "pairs", tolerance)
    for quad in (0, 1):
        for tables in (0, 1):
            gpu.patolette_amd_debug_delta_quad(quad)
            gpu.patolette_amd_debug_delta_local_tables(tables)
            ok, d, r, c, s, msg = patolette_amd.frame_deltas_local(maps, palettes, of, frames=_clip(size, F), tolerance=tolerance, want_shown=True)
            assert ok, msg
            assert gpu.patolette_amd_debug_delta_local_route() == tables
            _same((d, r, c, s), ref)


def test_the_launchers_own_choice_of_route(gpu):
    """P K = 32 goes to LDS; five tables of 255 rows for four frames (1275 > 256 F) and twenty of them (5100 > 4096, which no switch
    moves into LDS) are read from global memory.  Same results as the reference either way."""
    from oracle import binding as ob
    size, F = SIZES["odd64"]
    palettes, of, maps = _case(size, F, 16, "pairs")
    ok, *_ = patolette_amd.frame_deltas_local(maps, palettes, of)
    assert ok and gpu.patolette_amd_debug_delta_local_route() == 1
    frames = _clip(size, F)
    for P, forced in ((5, -1), (20, 1)):
        big = np.stack([_palette(255, seed=40 + g) for g in range(P)])
        order = [P - 1, 2, 0, P - 1]
        m = np.stack([delta_ref.maps_of(ob, frames[f:f + 1], big[order[f]], "nearest")[0] for f in range(F)]).astype(np.uint8)
        for tolerance in (0.0, 0.05):
            ref = local_delta_ref.frame_deltas(ob, m, big, order, frames=frames, tolerance=tolerance)
            assert tolerance == 0 or ref[4] >= MIN_GAP
            gpu.patolette_amd_debug_delta_local_tables(forced)
            ok, d, r, c, s, msg = patolette_amd.frame_deltas_local(m, big, order, frames=frames, tolerance=tolerance, want_shown=True)
            assert ok, msg
            assert gpu.patolette_amd_debug_delta_local_route() == 0
            _same((d, r, c, s), ref)
        if P == 5:                                                     # ... and forced into LDS, where 1275 words fit
            gpu.patolette_amd_debug_delta_local_tables(1)
            ok, d, r, c, s, msg = patolette_amd.frame_deltas_local(m, big, order, frames=frames, tolerance=0.05, want_shown=True)
            assert ok and gpu.patolette_amd_debug_delta_local_route() == 1
            _same((d, r, c, s), ref)


def test_a_row_shared_between_two_tables_keeps_across_them(gpu):
    from oracle import binding as ob
    size, F = SIZES["small"]
    palettes, of, maps = _case(size, F, 16, "pairs")
    palettes, maps = palettes.copy(), maps.copy()
    palettes[1, 5] = palettes[0, 9]
    maps[1, 3:9, 2:30], maps[2, 3:9, 2:30] = 9, 5                       # of = 0, 0, 1, 1, 0: frame 2 is the first of table 1
    ref = local_delta_ref.frame_deltas(ob, maps, palettes, of)
    assert np.all(ref[0][2, 3:9, 2:30] == 16)
    ok, d, r, c, s, msg = patolette_amd.frame_deltas_local(maps, palettes, of, want_shown=True)
    assert ok, msg
    _same((d, r, c, s), ref)


@pytest.mark.parametrize("size", [(1, 70), (65, 1)])
def test_one_pixel_wide(gpu, size):
    from oracle import binding as ob
    frames = _image("scene", size, 3, 3)
    palettes = np.stack([_palette(16, seed=2 + g) for g in range(3)])
    maps = np.stack([delta_ref.maps_of(ob, frames[f:f + 1], palettes[f], "nearest")[0] for f in range(3)]).astype(np.uint8)
    ref = local_delta_ref.frame_deltas(ob, maps, palettes)
    ok, d, r, c, s, msg = patolette_amd.frame_deltas_local(maps, palettes, want_shown=True)
    assert ok, msg
    _same((d, r, c, s), ref)
    thin, long = (3, 2) if size[0] == 1 else (2, 3)
    assert np.all(c[1:] > 8) and np.all(r[:, thin] == 1) and np.all(r[1:, long] > 8)


@pytest.mark.parametrize("name", ["small", "odd64", "quad"])
def test_identical_tables_give_frame_deltas_on_the_device(gpu, name):
    """Consequence (c), device against device, at all three tolerances: one table, and F copies of it."""
    size, F = SIZES[name]
    palettes, _, maps = _case(size, F, 16, "one")
    frames = _clip(size, F)
    for tolerance in TOLERANCES:
        ok, d0, r0, c0, s0, msg = patolette_amd.frame_deltas(maps, palettes[0], frames=frames, tolerance=tolerance, want_shown=True)
        assert ok, msg
        for pals, of in ((palettes, [0] * F), (np.stack([palettes[0]] * F), None)):
            ok, d, r, c, s, msg = patolette_amd.frame_deltas_local(maps, pals, of, frames=frames, tolerance=tolerance, want_shown=True)
            assert ok, msg
            assert np.array_equal(d, d0) and np.array_equal(r, r0) and np.array_equal(c, c0) and np.array_equal(s, palettes[0][s0])


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c_call(gpu, maps, palettes, of, T, frames=None, channels=3, tolerance=0.0, delta=None, shown=None, rects=None, changed=None, dims=None,
            P=None, K=None):
    F, h, w = dims if dims is not None else maps.shape
    code = C.c_int(7)
    of = None if of is None else np.ascontiguousarray(of, dtype=np.int32)
    gpu.patolette_amd_frame_deltas_local(F, w, h, _vp(maps), _vp(palettes), palettes.shape[0] if P is None else P,
                                         palettes.shape[1] if K is None else K, None if of is None else of.ctypes.data_as(C.POINTER(C.c_int32)),
                                         T, _vp(frames), channels, tolerance, _vp(delta), _vp(shown),
                                         None if rects is None else rects.ctypes.data_as(C.POINTER(C.c_int32)),
                                         None if changed is None else changed.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(code))
    return code.value


def test_outputs_aliasing_and_channels_through_the_c_entry(gpu):
    size, F = SIZES["small"]
    frames = _clip(size, F)
    rgba = np.concatenate([frames, np.full(frames.shape[:3] + (1,), 7, dtype=np.uint8)], axis=-1)     # a 4th byte is ignored
    for K, T in ((16, 16), (16, 200), (255, 255)):
        palettes, of, maps = _case(size, F, K, "pairs")
        for tolerance in (0.0, 0.05):
            ref = _reference(size, F, K, "pairs", tolerance)
            d_ref = np.where(ref[0] == K, T, ref[0]).astype(np.uint8)
            for px, ch in ((frames, 3), (rgba, 4)):
                kw = dict(frames=px, channels=ch, tolerance=tolerance) if tolerance else {}
                d, s = np.zeros_like(maps), np.zeros(maps.shape + (3,), dtype=np.uint8)
                r, c = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.uint64)
                assert _c_call(gpu, maps, palettes, of, T, delta=d, shown=s, rects=r, changed=c, **kw) == 0
                assert np.array_equal(d, d_ref) and np.array_equal(s, ref[1]) and np.array_equal(r, ref[2])
                assert np.array_equal(c.astype(np.int64), ref[3])
            inout = maps.copy()                                        # delta_maps aliasing palette_maps
            assert _c_call(gpu, inout, palettes, of, T, delta=inout, **kw) == 0 and np.array_equal(inout, d_ref)
            d, s = np.zeros_like(maps), np.zeros(maps.shape + (3,), dtype=np.uint8)
            r, c = np.zeros((F, 4), dtype=np.int32), np.zeros(F, dtype=np.uint64)
            assert _c_call(gpu, maps, palettes, of, T, delta=d, **kw) == 0 and np.array_equal(d, d_ref)
            assert _c_call(gpu, maps, palettes, of, T, shown=s, **kw) == 0 and np.array_equal(s, ref[1])
            assert _c_call(gpu, maps, palettes, of, T, rects=r, **kw) == 0 and np.array_equal(r, ref[2])
            assert _c_call(gpu, maps, palettes, of, T, changed=c, **kw) == 0 and np.array_equal(c.astype(np.int64), ref[3])
            assert _c_call(gpu, maps, palettes, of, T, **kw) == 0


def test_errors_and_recovery(gpu):
    size, F = SIZES["small"]
    h, w = size
    palettes, of, maps = _case(size, F, 16, "pairs")
    frames = _clip(size, F)
    ref = _reference(size, F, 16, "pairs", 0.05)
    d = np.zeros_like(maps)
    r = np.zeros((F, 4), dtype=np.int32)

    def lossy(m=maps, **kw):
        args = dict(frames=frames, tolerance=0.05, delta=d, rects=r)
        args.update(kw)
        return _c_call(gpu, m, args.pop("palettes", palettes), args.pop("of", of), args.pop("T", 16), **args)

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
    # an element that is no row: the kernel's flag, in both modes, on either route
    for where in ((3, 17, 5), (0, 0, 0), (F - 1, h - 1, w - 1)):
        bad = maps.copy()
        bad[where] = 16
        failed(lossy(m=bad), "palette_rows")
        failed(_c_call(gpu, bad, palettes, of, 16, delta=d), "palette_rows")
        bad[where] = 255
        gpu.patolette_amd_debug_delta_local_tables(0)
        failed(lossy(m=bad), "palette_rows")
        gpu.patolette_amd_debug_delta_local_tables(-1)
    with pytest.raises(ValueError, match="palette_rows"):
        patolette_amd.frame_deltas_local(bad, palettes, of)
    good()
    # -1: the arguments
    failed(lossy(K=0), "palette_rows")
    failed(lossy(K=256, T=256), "palette_rows")
    failed(lossy(P=0), "palette_count")
    failed(lossy(P=65537), "palette_count")
    failed(lossy(T=15), "transparent_index")
    failed(lossy(T=256), "transparent_index")
    failed(lossy(of=[0, 0, 1, 1, 2]), "palette_of")
    failed(lossy(of=[0, 0, -1, 1, 0]), "palette_of")
    failed(lossy(of=None), "palette_count must equal frames")
    failed(lossy(channels=2), "channels")
    failed(lossy(channels=5), "channels")
    for tolerance in (-0.01, float("nan"), float("inf"), -float("inf")):
        failed(lossy(tolerance=tolerance), "tolerance")
    failed(lossy(frames=None), "pixels")
    code = C.c_int(7)
    o = np.ascontiguousarray(of, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    gpu.patolette_amd_frame_deltas_local(F, w, h, None, _vp(palettes), 2, 16, o, 16, None, 3, 0.0, _vp(d), None, None, None, C.byref(code))
    failed(code.value, "no maps")
    gpu.patolette_amd_frame_deltas_local(F, w, h, _vp(maps), None, 2, 16, o, 16, None, 3, 0.0, _vp(d), None, None, None, C.byref(code))
    failed(code.value, "no palettes")
    assert lossy(tolerance=-0.0) == 0                                  # -0.0 is not negative: the exact mode
    # -2 and -4
    assert lossy(dims=(0, h, w)) == -2
    assert lossy(dims=(F, 0, w)) == -2
    assert lossy(dims=(F, h, 0)) == -2
    good()
    assert lossy(dims=(1, 50000, 50000)) == -4 and _native.last_error().startswith(PREFIX)
    good()


def test_the_same_call_gives_the_same_bytes(gpu):
    size, F = SIZES["wrap"]
    palettes, of, maps = _case(size, F, 255, "each")
    frames = _clip(size, F)
    other = _image("noise", (96, 80), 1, 3)

    def run():
        ok, d, r, c, s, msg = patolette_amd.frame_deltas_local(maps, palettes, of, frames=frames, tolerance=0.02, want_shown=True)
        assert ok, msg
        return d, r, c, s

    first = run()
    second = run()
    ok, *_ = patolette_amd.remap(other, palettes[0], dither="ordered")
    assert ok
    ok, *_ = patolette_amd.frame_deltas(maps, 255)
    assert ok
    third = run()
    for got in (second, third):
        assert all(np.array_equal(a, b) for a, b in zip(got, first))
    _same(first, _reference(size, F, 255, "each", 0.02))


def test_last_stats_and_one_launch_of_each_kernel(gpu):
    size, F = SIZES["wrap"]
    palettes, of, maps = _case(size, F, 255, "each")
    for tolerance in (0.0, 0.02):
        _native.profile(True)
        ok, *_ = patolette_amd.frame_deltas_local(maps, palettes, of, frames=_clip(size, F), tolerance=tolerance, want_shown=True)
        prof = _native.profile_results()
        _native.profile(False)
        assert ok
        assert prof["k_frame_deltas_local"]["launches"] == 1 and prof["k_delta_boxes"]["launches"] == 1
        assert not set(prof) & {"k_frame_deltas", "k_convert_u8", "k_convert", "k_nn_map", "k_nn_map_u8", "k_ordered_map", "k_dither"}
        st = patolette_amd.last_stats()
        assert st["ms_total"] > 0 and st["ms_map"] > 0 and st["ms_upload"] > 0 and st["ms_download"] > 0
        assert st["ms_total"] >= st["ms_map"]
        assert all(st[key] == 0 for key in st if not key.startswith("ms_"))
        assert st["ms_convert"] == 0 and st["ms_gq"] == 0 and st["ms_lq"] == 0 and st["ms_kmeans"] == 0 and st["ms_saliency"] == 0


def test_torch_flavour(gpu):
    """Torch CUDA tensors go through patolette_amd_frame_deltas_local_device: the numpy flavour's results, deltas and shown_rgb on the
    maps' device.  Own process: torch loads its HIP runtime before libpatolette_amd.so does."""
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
from tests import test_gpu_local_delta as t
for name, K, kind in (("wrap", 16, "each"), ("odd64", 255, "pairs"), ("quad", 16, "pairs")):
    size, F = t.SIZES[name]
    palettes, of, maps = t._case(size, F, K, kind)
    frames = t._clip(size, F)
    m_t, f_t = torch.from_numpy(maps.copy()).cuda(), torch.from_numpy(frames.copy()).cuda()
    for tol in (0.0, 0.05):
        p._native.lib().patolette_amd_debug_delta_quad(-1)
        ok, d, r, c, s, msg = p.frame_deltas_local(maps, palettes, of, frames=frames, tolerance=tol, want_shown=True)
        assert ok, msg
        p._native.lib().patolette_amd_debug_delta_quad(1)           # four positions per lane where the tensors allow it
        ok, dt, rt, ct, st, msg = p.frame_deltas_local(m_t, palettes, of, frames=f_t, tolerance=tol, want_shown=True)
        assert ok, msg
        assert dt.device == m_t.device and st.device == m_t.device and dt.dtype == torch.uint8 and st.dtype == torch.uint8
        assert tuple(dt.shape) == d.shape and tuple(st.shape) == s.shape
        assert isinstance(rt, np.ndarray) and isinstance(ct, np.ndarray)
        assert np.array_equal(dt.cpu().numpy(), d) and np.array_equal(st.cpu().numpy(), s)
        assert np.array_equal(rt, r) and np.array_equal(ct, c)
    ok, dt2, rt2, ct2, none, msg = p.frame_deltas_local(m_t, torch.from_numpy(palettes.copy()), of)
    assert ok and none is None, msg
    try:
        p.frame_deltas_local(m_t, palettes, of, frames=frames, tolerance=0.05)
        raise SystemExit("host frames with device maps were accepted")
    except ValueError:
        pass
print("TORCH-LOCAL-DELTA-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "TORCH-NO-DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "TORCH-LOCAL-DELTA-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def two_scenes(h=40, w=56):
    """(6, h, w, 3) uint8: two scenes of three frames, tests.util.scene with two seeds, the second inverted; every frame of a scene
    with its own +-2 of noise."""
    rng = np.random.default_rng(11)
    out = []
    for seed, invert in ((5, False), (9, True)):
        base = np.round(scene(h, w, seed) * 255).astype(np.int64)
        base = 255 - base if invert else base
        for _ in range(3):
            out.append(np.clip(base + rng.integers(-2, 3, size=base.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


def _sse(a, b):
    return int(np.sum((a.astype(np.int64) - b.astype(np.int64)) ** 2))


def test_end_to_end_two_scenes_two_palettes(gpu, tmp_path):
    """(i) one palette of 16 for all six frames -> frame_deltas -> write_gif; (ii) one of 16 per scene -> frame_deltas_local -> write_gif
    with a local colour table.  Both files composite to what the deltas' entry says is shown, and (ii) is strictly closer to the
    source.  (The CPU oracle's quantiser gives 17 277 421 against 13 560 282 summed squared error for these frames.)"""
    frames = two_scenes()
    kw = dict(dither=False, tile_size=0, kmeans_niter=2, kmeans_max_samples=4096, want_quantized=False)
    ok, pal8, maps, _, _, msg = patolette_amd.quantize_frames(frames, 16, **kw)
    assert ok, msg
    ok, d, r, c, s, msg = patolette_amd.frame_deltas(maps, pal8, want_shown=True)
    assert ok, msg
    blob = patolette_amd.write_gif(None, d, pal8, r, transparent_index=16)
    head, parsed = local_delta_ref.parse_gif(blob)
    assert all(fr["table"] is None for fr in parsed)
    one = local_delta_ref.composite_rgb(head, parsed)
    assert np.array_equal(one, pal8[s])
    palettes, local_maps = [], []
    for scene_frames in (frames[:3], frames[3:]):
        ok, p8, m, _, _, msg = patolette_amd.quantize_frames(scene_frames, 16, **kw)
        assert ok, msg
        palettes.append(p8)
        local_maps.append(m)
    palettes, local_maps, of = np.stack(palettes), np.concatenate(local_maps), [0, 0, 0, 1, 1, 1]
    ok, d, r, c, shown, msg = patolette_amd.frame_deltas_local(local_maps, palettes, of, want_shown=True)
    assert ok, msg
    path = tmp_path / "two.gif"
    blob2 = patolette_amd.write_gif(path, d, palettes, r, transparent_index=16, palette_of=of)
    head, parsed = local_delta_ref.parse_gif(blob2)
    assert [fr["table"] is not None for fr in parsed] == [False, False, False, True, True, True]
    two = local_delta_ref.composite_rgb(head, parsed)
    assert np.array_equal(two, shown)
    try:
        from PIL import Image
        im = Image.open(str(path))
        assert im.n_frames == 6
        for f in range(6):
            im.seek(f)
            assert np.array_equal(np.asarray(im.convert("RGB")), shown[f]), f
    except ImportError:
        pass
    sse_one, sse_two = _sse(one, frames), _sse(two, frames)
    print("summed squared error: one palette %d, a palette per scene %d; bytes %d and %d" % (sse_one, sse_two, len(blob), len(blob2)))
    assert sse_two < sse_one


def test_near_tables_per_palette(gpu):
    """write_gif(near=(P, 256, 16)): every coded entry is the delta's own, or one of its row's candidates in that frame's table; the
    transparent index is untouched."""
    from oracle import binding as ob
    size, F = SIZES["small"]
    palettes, of, maps = _case(size, F, 16, "pairs")
    T = 16
    ok, d, r, c, shown, msg = patolette_amd.frame_deltas_local(maps, palettes, of, frames=_clip(size, F), tolerance=0.02, want_shown=True)
    assert ok, msg
    near = []
    for g in range(2):
        ok, table, msg = patolette_amd.gif_neighbours(palettes[g], 0.25, transparent_index=T)
        assert ok and table[:16, 0].max() > 0, msg
        near.append(table)
    near = np.stack(near)
    blob = patolette_amd.write_gif(None, d, palettes, r, transparent_index=T, palette_of=of, near=near)
    head, parsed = local_delta_ref.parse_gif(blob)
    replaced = 0
    for f, fr in enumerate(parsed):
        x0, y0, w, h = fr["rect"]
        idx = np.array(lzw_ref.decode(fr["stream"], fr["m"], w * h)).reshape(h, w)
        own = d[f, y0:y0 + h, x0:x0 + w].astype(np.int64)
        rows = near[of[f]][own]                                        # (h, w, 16)
        candidate = np.any((rows[..., 1:] == idx[..., None]) & (np.arange(1, 16) <= rows[..., :1]), axis=-1)
        assert np.all((idx == own) | candidate)
        assert np.array_equal(idx == T, own == T)
        replaced += int(np.sum(idx != own))
    assert replaced > 0
