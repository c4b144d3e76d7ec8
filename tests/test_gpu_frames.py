"""quantize_frames / patolette_amd_frames_u8: frames of one size, ONE palette, every frame mapped on its own.

  * one frame is quantize_u8, every output bit for bit; without dithering any number of frames is quantize_u8 of the stacked image;
  * against the oracle recipe (tests/frames_ref.py: the palette of the stacked pixels, then the reference's map stage frame by
    frame from an empty error queue): maps bit for bit, f64 palettes to 1e-9 -- no pixel is excluded from any comparison;
  * the frame-batched lane walk: forced (patolette_amd_dither_layout(1)) with default cuts, with cuts that make repairs happen and
    with solo passes, and at a size that takes it by default; always equal to the wavefront layout's frame-by-frame result;
  * saliency weights per frame, device tensors, four channels, palette_only, K > 256, workspace history, errors.
Content: tests.util.scene frames rounded to 8 bits and uniform noise (no posterised or flat content: no exact ties).
The dither knobs have no getters: a test that turns one puts the defaults back (0 / -1 / -1), as the other dither tests do."""
import ctypes as C

import numpy as np
import pytest

from tests import frames_ref
from tests.util import scene

pytestmark = pytest.mark.gpu


def _frames(f, h, w, seed, kind="scene", channels=3):
    rng = np.random.default_rng(seed)
    if kind == "scene":
        fr = np.stack([np.round(scene(h, w, seed + 7 * i) * 255).astype(np.uint8) for i in range(f)])
    else:
        fr = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    if channels == 4:
        fr = np.concatenate([fr, rng.integers(0, 256, (f, h, w, 1), dtype=np.uint8)], axis=3)
    return np.ascontiguousarray(fr)


def _same(a, b):
    """two result tuples (success, palette_u8, maps, quantized, palette, message): every output bit for bit"""
    assert a[0] and b[0], (a[-1], b[-1])
    for i in (1, 2, 3, 4):
        if a[i] is None or b[i] is None:
            assert a[i] is None and b[i] is None, i
        else:
            x, y = np.asarray(a[i]), np.asarray(b[i])
            assert x.dtype == y.dtype and np.array_equal(x.reshape(-1), y.reshape(-1)), i


def _against_oracle(ob, fr, K, got, **kw):
    ok, pal8, maps, quant, pal, msg = got
    assert ok, msg
    pal_o, maps_o = frames_ref.quantize_frames(ob, fr, K, **kw)
    err = float(np.max(np.abs(pal - pal_o)))
    mism = int(np.sum(maps.astype(np.int64) != maps_o))
    print("frames %s K=%d %s: palette max abs diff %.3g, map mismatches %d / %d" % (fr.shape, K, kw, err, mism, maps_o.size))
    assert err <= 1e-9
    assert mism == 0
    assert np.array_equal(pal8, np.clip(pal * 255, 0, 255).astype(np.uint8) * (pal[:, :1] != -1))
    if quant is not None:
        assert np.array_equal(quant, pal8[maps.astype(np.int64)])


@pytest.fixture
def knobs(gpu):
    """the dither knobs back to their defaults afterwards"""
    stall, cap = [], []

    class K:
        def layout(self, v): gpu.patolette_amd_dither_layout(v)
        def config(self, s, w): gpu.patolette_amd_dither_config(s, w)
        def stall_passes(self, n): stall.append(gpu.patolette_amd_debug_dither_stall_passes(n))
        def solo_cap(self, n): cap.append(gpu.patolette_amd_debug_dither_solo_cap(n))
    yield K()
    gpu.patolette_amd_dither_layout(-1)
    gpu.patolette_amd_dither_config(0, -1)
    if stall:
        gpu.patolette_amd_debug_dither_stall_passes(stall[0])
    if cap:
        gpu.patolette_amd_debug_dither_solo_cap(cap[0])


# ---- 1. one frame is quantize_u8; no dither is the stacked quantize_u8 -------------------------------------------------------
@pytest.mark.parametrize("dither", [True, False])
@pytest.mark.parametrize("cs", [2, 1])
def test_one_frame_is_quantize_u8(gpu, dither, cs):
    import patolette_amd as p
    fr = _frames(1, 72, 100, 5)
    kw = dict(dither=dither, color_space=cs, tile_size=512, kmeans_niter=3, kmeans_max_samples=4096)
    _same(p.quantize_frames(fr, 24, **kw), p.quantize_u8(fr[0], 24, **kw))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cs", [0, 1, 2])
def test_no_dither_is_the_stacked_image(gpu, ob, weighted, cs):
    import patolette_amd as p
    f, h, w = 4, 60, 88
    fr = _frames(f, h, w, 9, "noise" if cs == 0 else "scene")
    wts = ob.weights(f * h * w, 3) if weighted else None
    kw = dict(dither=False, color_space=cs, tile_size=0, kmeans_niter=3, kmeans_max_samples=4096, weights=wts)
    _same(p.quantize_frames(fr, 40, **kw), p.quantize_u8(fr.reshape(f * h, w, 3), 40, **kw))


def test_dither_shares_the_stacked_palette_not_its_map(gpu):
    import patolette_amd as p
    f, h, w = 3, 40, 56
    fr = _frames(f, h, w, 11)
    kw = dict(dither=True, tile_size=0, kmeans_niter=4, kmeans_max_samples=1024)
    a, b = p.quantize_frames(fr, 24, **kw), p.quantize_u8(fr.reshape(f * h, w, 3), 24, **kw)
    assert a[0] and b[0]
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[1], b[1])
    assert np.mean(a[2].reshape(-1) != b[2].reshape(-1)) > 0.05


# ---- 2. against the oracle recipe ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [0, 6])
@pytest.mark.parametrize("dither", [True, False])
@pytest.mark.parametrize("cs", [2, 1, 0])
@pytest.mark.parametrize("K", [16, 256])
@pytest.mark.parametrize("f,h,w,kind", [(2, 64, 96, "scene"), (5, 64, 96, "noise"), (2, 37, 101, "noise"), (5, 37, 101, "scene")])
def test_against_the_oracle(gpu, ob, f, h, w, kind, K, cs, dither, niter):
    import patolette_amd as p
    fr = _frames(f, h, w, 21 + f + K, kind)
    kw = dict(dither=dither, color_space=cs, kmeans_niter=niter, kmeans_max_samples=4096)
    _against_oracle(ob, fr, K, p.quantize_frames(fr, K, tile_size=0, **kw), **kw)


def test_against_the_oracle_weighted(gpu, ob):
    import patolette_amd as p
    fr = _frames(3, 48, 80, 4)
    wts = ob.weights(fr[..., 0].size, 8)
    kw = dict(dither=True, color_space=2, kmeans_niter=3, kmeans_max_samples=2048, weights=wts)
    _against_oracle(ob, fr, 32, p.quantize_frames(fr, 32, tile_size=0, **kw), **kw)


# ---- 3. the frame-batched lane walk -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default_cut", "repairs", "solo", "gives_up"])
@pytest.mark.parametrize("kind,cs", [("scene", 2), ("noise", 1)])
def test_batched_lane_walk(gpu, ob, native, knobs, kind, cs, mode):
    """F = 4 frames of 256 x 256 under patolette_amd_dither_layout(1): the lane layout walks all frames in one set of launches.  The
    cut puts the same number of runs into every frame; with a short warm-up boundaries fail and are repaired; with
    patolette_amd_debug_dither_stall_passes(0) every repair pass is one wavefront's walk, which must stop at the frame's end; with
    patolette_amd_debug_dither_solo_cap(0) the batched walk gives the stack up and the wavefront layout takes it frame by frame."""
    import patolette_amd as p
    f, h, w, K = 4, 256, 256, 64
    fr = _frames(f, h, w, 31, kind)
    kw = dict(dither=True, color_space=cs, kmeans_niter=2, kmeans_max_samples=8192)
    knobs.layout(0)
    waves = p.quantize_frames(fr, K, tile_size=0, **kw)
    assert waves[0]
    knobs.layout(1)
    assert gpu.patolette_amd_dither_layout_in_use(w, f * h, K) == 1
    if mode == "repairs":
        knobs.config(4 * 300 + 1, 24)               # rounded up to a multiple of F; 24 steps of warm-up settle few boundaries
    elif mode == "solo":
        knobs.config(4 * 64, 0)                     # no warm-up: every inner boundary fails the first check
        knobs.stall_passes(0)
    elif mode == "gives_up":
        knobs.config(4 * 64, 0)
        knobs.stall_passes(0)
        knobs.solo_cap(0)
    got = p.quantize_frames(fr, K, tile_size=0, **kw)
    st = p.last_stats()
    print(mode, kind, {k: v for k, v in st.items() if k.startswith("dither")})
    _same(got, waves)
    _against_oracle(ob, fr, K, got, **kw)
    if mode == "gives_up":
        return
    assert st["dither_segments"] % f == 0 and st["dither_segments"] > f
    if mode == "repairs":
        assert st["dither_segments"] == 4 * 301 and st["dither_repairs"] > 0
    if mode == "solo":
        assert st["dither_solo"] > 0 and st["dither_repairs"] > 0


def test_lane_layout_by_default(gpu, ob, knobs):
    """40 frames of 640 x 360: 9.2 Mpx together, the lane layout's territory with the knobs at their defaults, although one frame alone
    (0.23 Mpx) is far below it.  Against the oracle recipe frame by frame and against the wavefront layout."""
    import patolette_amd as p
    f, h, w, K = 40, 360, 640, 64
    base = _frames(4, h, w, 41)
    fr = np.ascontiguousarray(np.stack([np.roll(base[i % 4], 13 * i, axis=1) for i in range(f)]))
    kw = dict(dither=True, color_space=2, kmeans_niter=2, kmeans_max_samples=65536)
    assert f * h * w >= 1 << 23 and gpu.patolette_amd_dither_layout_in_use(w, f * h, K) == 1
    assert gpu.patolette_amd_dither_layout_in_use(w, h, K) == 0
    got = p.quantize_frames(fr, K, tile_size=0, **kw)
    st = p.last_stats()
    print({k: v for k, v in st.items() if k.startswith("dither")})
    assert st["dither_segments"] % f == 0 and st["dither_segments"] > f
    knobs.layout(0)
    _same(got, p.quantize_frames(fr, K, tile_size=0, **kw))
    _against_oracle(ob, fr, K, got, **kw)


# ---- 4. weights, inputs, outputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dither", [True, False])
def test_saliency_weights_are_per_frame(gpu, dither):
    import patolette_amd as p
    f, h, w = 3, 90, 120
    fr = _frames(f, h, w, 2)
    wts = np.concatenate([p.saliency_weights(w, h, fr[i].reshape(-1, 3) / 255.0, 64) for i in range(f)])
    kw = dict(dither=dither, kmeans_niter=2, kmeans_max_samples=4096)
    _same(p.quantize_frames(fr, 20, tile_size=64, **kw), p.quantize_frames(fr, 20, tile_size=0, weights=wts, **kw))


def test_four_channels_palette_only_and_large_palette(gpu, ob):
    import patolette_amd as p
    fr4 = _frames(3, 50, 70, 6, "scene", channels=4)
    rgb = np.ascontiguousarray(fr4[..., :3])
    kw = dict(tile_size=0, kmeans_niter=2, kmeans_max_samples=4096)
    for dither in (True, False):
        _same(p.quantize_frames(fr4, 16, dither=dither, **kw), p.quantize_frames(rgb, 16, dither=dither, **kw))
    # palette_only: the palette in the quantisation space, no maps
    ok, pal8, maps, quant, pal, msg = p.quantize_frames(rgb, 16, palette_only=True, **kw)
    assert ok and maps is None and quant is None
    pal_o, _ = frames_ref.quantize_frames(ob, rgb, 16, palette_only=True, kmeans_niter=2, kmeans_max_samples=4096)
    assert np.max(np.abs(pal - pal_o)) <= 1e-9
    # K > 256: 16-bit maps on the host, the wavefront layout
    fr = _frames(3, 64, 96, 8, "noise")
    for dither in (True, False):
        k2 = dict(dither=dither, color_space=2, kmeans_niter=0, kmeans_max_samples=4096)
        got = p.quantize_frames(fr, 300, tile_size=0, **k2)
        assert got[2].dtype == np.uint16
        _against_oracle(ob, fr, 300, got, **k2)
    ok, pal8, maps, quant, pal, msg = p.quantize_frames(fr, 300, tile_size=0, want_quantized=False, kmeans_niter=0)
    assert ok and quant is None and maps.shape == (3, 64, 96)


def test_torch_tensor_equals_numpy(gpu):
    """A torch CUDA tensor goes through patolette_amd_frames_u8_device: the numpy path's results, maps and frames left in HBM.  Own
    process: torch loads its HIP runtime before libpatolette_amd.so does."""
    import subprocess
    import sys
    from tests.util import ROOT
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
assert torch.cuda.is_available()
import patolette_amd as p
from tests.test_gpu_frames import _frames
fr = _frames(3, 50, 70, 3)
for dither in (False, True):
    for K in (16, 300):
        for tile in (0, 64):
            kw = dict(dither=dither, tile_size=tile, kmeans_niter=2, kmeans_max_samples=4096)
            ref = p.quantize_frames(fr, K, **kw)
            got = p.quantize_frames(torch.from_numpy(fr).cuda(), K, **kw)
            assert ref[0] and got[0] and got[2].is_cuda and got[3].is_cuda
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[4], ref[4])
            assert np.array_equal(got[2].cpu().numpy().astype(np.int64), ref[2].astype(np.int64))
            assert np.array_equal(got[3].cpu().numpy(), ref[3])
print("TORCH-FRAMES-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "TORCH-FRAMES-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 5. workspace history ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["waves", "lanes", "saliency_nodither"])
def test_result_does_not_depend_on_workspace_history(gpu, knobs, cfg):
    """The same call on a fresh engine, after a larger unrelated call and with fresh memory poisoned: identical bytes, and no buffer
    replaced while work was queued."""
    import patolette_amd as p
    if cfg == "lanes":
        fr, K = _frames(4, 256, 256, 51), 48
        kw = dict(dither=True, tile_size=0, kmeans_niter=2, kmeans_max_samples=8192)
        knobs.layout(1)
    elif cfg == "waves":
        fr, K = _frames(5, 70, 110, 52, "noise"), 300
        kw = dict(dither=True, tile_size=0, kmeans_niter=2, kmeans_max_samples=4096, color_space=1)
    else:
        fr, K = _frames(3, 90, 120, 53), 24
        kw = dict(dither=False, tile_size=64, kmeans_niter=2, kmeans_max_samples=4096, color_space=1)
    prev = gpu.patolette_amd_debug_workspace(0)
    gpu.patolette_amd_debug_workspace(prev | 2)
    try:
        late0 = gpu.patolette_amd_debug_late_growths()
        gpu.patolette_amd_release_workspace()
        fresh = p.quantize_frames(fr, K, **kw)
        big = np.random.default_rng(1).integers(0, 256, (700, 900, 3), dtype=np.uint8)
        assert p.quantize_u8(big, 200, dither=True, tile_size=256, kmeans_niter=1)[0]
        stale = p.quantize_frames(fr, K, **kw)
        gpu.patolette_amd_debug_workspace(prev | 3)
        gpu.patolette_amd_release_workspace()
        poisoned = p.quantize_frames(fr, K, **kw)
        _same(fresh, stale)
        _same(fresh, poisoned)
        assert gpu.patolette_amd_debug_late_growths() == late0, "a workspace buffer was replaced while work was queued"
    finally:
        gpu.patolette_amd_debug_workspace(prev)
        gpu.patolette_amd_release_workspace()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors(gpu, native):
    import patolette_amd as p
    fr = _frames(2, 20, 30, 1)
    with pytest.raises(ValueError):
        p.quantize_frames(fr[0], 8)                                 # rank
    with pytest.raises(ValueError):
        p.quantize_frames(fr.astype(np.float64), 8)                 # dtype
    with pytest.raises(ValueError):
        p.quantize_frames(fr[..., :2], 8)                           # channels
    with pytest.raises(ValueError):
        p.quantize_frames(fr, 8, weights=np.ones(20 * 30))          # weights for one frame only
    with pytest.raises(ValueError):
        p.quantize_frames(fr, 8, tile_size=-1)
    ok, *_, msg = p.quantize_frames(fr, 0, tile_size=0)
    assert not ok and msg == "Palette size should be greater than 0."
    ok, *_, msg = p.quantize_frames(fr[:0], 8, tile_size=0)
    assert not ok and msg == "Image dimensions should be greater than 0."
    opts = native.QuantizationOptions(True, False, 2, 0, 0, False)
    code = C.c_int(7)
    args = (None, 3, None, 0.0, 8, C.byref(opts), None, None, None, 1, None, C.byref(code))
    gpu.patolette_amd_frames_u8(0, 30, 20, *args)
    assert code.value == -2
    gpu.patolette_amd_frames_u8(2, 30, 0, *args)
    assert code.value == -2
    gpu.patolette_amd_frames_u8(1 << 20, 64, 64, *args)             # 2^32 pixels: beyond what the dither numbers
    assert code.value == -4 and "2^31" in native.last_error()
    gpu.patolette_amd_frames_u8(2, 30, 20, None, 5, None, 0.0, 8, C.byref(opts), None, None, None, 1, None, C.byref(code))
    assert code.value == -1
