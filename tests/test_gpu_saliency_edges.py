"""The saliency stage (saliency.hip) at its edges: what tests/test_gpu_saliency.py leaves out.

Raster scans (`patolette_amd_mbd` against `orc_mbd`, bit for bit): visited row counts at 63 / 64 / 65 and 127 / 128 / 129 (strip
edges of both scans), visited column counts at 1, 2 and around the 32-step chunk edges, many strips with one chunk and one strip
with many chunks, content whose visits are decided by exact ties, two exact metamorphic identities that need no oracle, and
independence from what the skewed state buffer held before (order of sizes; NaN-poisoned fresh memory).

Weights (`saliency_weights` against oracle/saliency.py `get_weights`): the bar is the project's 1e-9 relative on the weights,
taken at tile_size = sqrt(rows * cols) / 2, so that weight - 1 = 4 sal^2 and the bar holds the saliency itself to a few 1e-9
(at tile_size = 512 on a small image weight - 1 is ~0.02 sal^2 and the same bar lets 5e-8 through).  Why 1e-9 is not more than the
oracle supports: the band covariances of every case below have condition numbers <= 2e3 (measured on the CPU: noise 1e1 .. 1e3,
scene <= 2e3 from (10,10) up; the scene at (4,25) has a 4-pixel band with 6e5 and is not used there), so the Mahalanobis terms
carry ~cond * 2^-53 * a few = 1e-12, and pow / cbrt / exp a few ulp.

The constant-channel-mean image: exit code -7 (degenerate saliency map), never NaN weights with success.
"""
import ctypes as C
import functools
from math import sqrt

import numpy as np
import pytest

from tests.util import constant_mean_image, posterised_noise, scene, tie_images

pytestmark = pytest.mark.gpu
fp = C.POINTER(C.c_float)

GRID_ROWS = (4, 5, 65, 66, 67, 68, 130, 131, 132)                         # rows - 2 and rows - 3 at 63 / 64 / 65, 127 / 128 / 129
GRID_COLS = (4, 5, 34, 35, 36, 37, 66, 67, 68, 99, 100, 131)             # cols - 2 and cols - 3 at 1, 2, 32 / 64 / 96 +- 1, 128 / 129
STRIP_SHAPES = ((1100, 36), (1100, 5), (20, 300), (5, 4100), (700, 300))  # many strips x few chunks ... one strip x many chunks


def _mbd_gpu(native, img32, iters=3):
    img32 = np.ascontiguousarray(img32, dtype=np.float32)
    rows, cols = img32.shape
    out = np.zeros((rows, cols), dtype=np.float32)
    rc = native.lib().patolette_amd_mbd(rows, cols, img32.ctypes.data_as(fp), iters, out.ctypes.data_as(fp))
    assert rc == 0, (rows, cols, iters, rc)
    return out


def _where(got, want):
    """Row, column and forward-scan strip of the first differing pixel (for the failure message)."""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad) == 0:
        return None
    r, c = (int(v) for v in bad[0])
    return {"differing": len(bad), "row": r, "col": c, "forward_strip": (r - 1) // 64, "got": float(got[r, c]), "want": float(want[r, c])}


def _same_bits(got, want):
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _mbd_content(kind, rows, cols):
    if kind == "noise":
        img = np.random.default_rng(rows * 10007 + cols).random((rows, cols), dtype=np.float32)
    elif kind == "posterised":
        img = posterised_noise(rows, cols, rows * 10007 + cols)
    elif kind == "scene8":
        img = (np.round(scene(rows, cols, 3) * 255) / 255).mean(axis=2).astype(np.float32)
    else:
        img = tie_images(rows, cols)[kind]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _mbd_want(kind, rows, cols, iters):
    from oracle import binding
    want = binding.mbd(_mbd_content(kind, rows, cols), iters)
    want.setflags(write=False)
    return want


def _grid_cases():
    return [(r, c, kind, it) for r in GRID_ROWS for c in GRID_COLS for kind in ("noise", "posterised") for it in (1, 2, 3, 5)]


def test_mbd_shape_grid_bit_exact_in_either_order_of_sizes(gpu, native, ob):
    """Every (rows, cols) of the grid, iters 1, 2, 3, 5, noise and 8-level posterised noise: == orc_mbd bit for bit.  The grid runs
    from the largest shape down (the state buffers are allocated once and every smaller shape finds a larger one's leftovers in the
    cells it never writes) and again from the smallest up after the workspace has been released (every growth is fresh memory):
    the maps of the two runs must be the same bits."""
    cases = sorted(_grid_cases(), key=lambda t: (t[0] * t[1], t[0]))
    gpu.patolette_amd_release_workspace()
    down = {}
    for rows, cols, kind, iters in reversed(cases):
        got = _mbd_gpu(native, _mbd_content(kind, rows, cols), iters)
        want = _mbd_want(kind, rows, cols, iters)
        assert _same_bits(got, want), (rows, cols, kind, iters, _where(got, want))
        down[(rows, cols, kind, iters)] = got
    gpu.patolette_amd_release_workspace()
    for key in cases:
        rows, cols, kind, iters = key
        got = _mbd_gpu(native, _mbd_content(kind, rows, cols), iters)
        assert _same_bits(got, down[key]), (key, _where(got, down[key]))


@pytest.mark.parametrize("rows,cols", STRIP_SHAPES)
def test_mbd_many_strips_and_many_chunks(gpu, native, ob, rows, cols):
    for kind in ("noise", "posterised", "scene8"):
        got = _mbd_gpu(native, _mbd_content(kind, rows, cols), 3)
        want = _mbd_want(kind, rows, cols, 3)
        assert _same_bits(got, want), (kind, _where(got, want))


@pytest.mark.parametrize("rows,cols", [(67, 130), (131, 100)])
def test_mbd_tie_content(gpu, native, ob, rows, cols):
    """Flat, integer ramps (horizontal, vertical, diagonal), checkerboard, one bright pixel, a 0/1 step edge: the visit's
    `d <= min(b1, b2)` and `b1 <= b2` are ties at almost every pixel."""
    for kind in ("flat", "hramp", "vramp", "diag", "checker", "bright", "step"):
        for iters in (1, 2, 3):
            got = _mbd_gpu(native, _mbd_content(kind, rows, cols), iters)
            want = _mbd_want(kind, rows, cols, iters)
            assert _same_bits(got, want), (kind, iters, _where(got, want))


@pytest.mark.parametrize("rows,cols", [(67, 130), (1100, 36)])
def test_mbd_exact_metamorphic_identities(gpu, native, rows, cols):
    """No oracle: on an f32 image of integers 0..255 every max, min and difference of the scans is an exact integer, so
    mbd(255 - img) == mbd(img) (a barrier is max - min along a path; the paths and the tie order of b1 / b2 are unchanged) and
    mbd(2 img) == 2 mbd(img), bit for bit."""
    img = np.random.default_rng(rows + cols).integers(0, 256, size=(rows, cols)).astype(np.float32)
    for iters in (1, 3):
        base = _mbd_gpu(native, img, iters)
        inside = np.isfinite(base)                  # (one inverse scan alone leaves row 1 and column 1 at +inf: never visited)
        assert np.all(base[inside] == np.round(base[inside])) and base[inside].max() <= 255 and inside[2:-1, 2:-1].all()
        neg = _mbd_gpu(native, np.float32(255) - img, iters)
        assert _same_bits(neg, base), ("negated", iters, _where(neg, base))
        dbl = _mbd_gpu(native, np.float32(2) * img, iters)
        assert _same_bits(dbl, np.float32(2) * base), ("doubled", iters, _where(dbl, np.float32(2) * base))


def test_mbd_ignores_nan_in_cells_it_never_writes(gpu, native, ob):
    """patolette_amd_debug_workspace bit 0: fresh f32 memory starts as NaN, the raster scans' state included, so the cells of the
    skewed copy that belong to no pixel (k_mbd_skew never writes them; the scans' lanes read them) hold NaN.  The maps must not
    change.  The workspace is released first so that every buffer is allocated, and poisoned, under the flag."""
    prev = gpu.patolette_amd_debug_workspace(0)
    try:
        gpu.patolette_amd_debug_workspace(prev | 1)
        for rows, cols in sorted(STRIP_SHAPES, key=lambda s: s[0] * s[1]):      # ascending: every shape grows the buffers afresh
            gpu.patolette_amd_release_workspace()
            for kind in ("noise", "posterised", "scene8"):
                got = _mbd_gpu(native, _mbd_content(kind, rows, cols), 3)
                want = _mbd_want(kind, rows, cols, 3)
                assert _same_bits(got, want), (rows, cols, kind, _where(got, want))
    finally:
        gpu.patolette_amd_debug_workspace(prev)
        gpu.patolette_amd_release_workspace()


# ---------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------
ALL_CONTENT = ("scene", "noise", "posterised", "scene8", "dark", "dim")


@functools.lru_cache(maxsize=None)
def _rgb(kind, rows, cols):
    """(rows, cols, 3) float64 in [0,1].  dark: noise * 0.06, on both sides of the companding's 0.04045, every pixel on the low
    branch of the Lab cube root; dim: noise * 0.12, on both sides of 0.04045 and of the cube root's 0.008856."""
    seed = rows * 7 + cols
    rng = np.random.default_rng(seed)
    if kind == "noise":
        img = rng.random((rows, cols, 3))
    elif kind == "dark":
        img = rng.random((rows, cols, 3)) * 0.06
    elif kind == "dim":
        img = rng.random((rows, cols, 3)) * 0.12
    else:
        img = scene(rows, cols, seed)
        if kind == "posterised":
            img = np.floor(img * 8).clip(0, 7) / 7
        elif kind == "scene8":
            img = np.round(img * 255) / 255
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _weights_want(kind, rows, cols, tile):
    from oracle import saliency
    want = saliency.get_weights(_rgb(kind, rows, cols), tile)
    want.setflags(write=False)
    return want


def _half_tile(rows, cols):
    return sqrt(rows * cols) / 2            # n / tile^2 = 4


def _check_weights(got, want, rows, cols, tile):
    n = rows * cols
    assert np.all(np.isfinite(want))
    assert got.shape == (n,) and np.all(np.isfinite(got))
    assert np.all(got >= 1.0) and np.all(got <= 1.0 + n / tile ** 2)
    err = np.max(np.abs(got - want) / want)
    print("max relative error of the weights %.3g" % err)
    assert np.allclose(got, want, rtol=1e-9, atol=0), err


def _weight_cases():
    cases = []
    for shape in ((10, 10), (4, 25), (25, 4)):                 # smallest accepted: 100 pixels, a border band of one row / column
        cases += [shape + (k,) for k in ("noise", "dark")]
    for shape in ((11, 1000), (1000, 11)):                     # rows == bt + 1, cols == bt + 1
        cases += [shape + (k,) for k in ALL_CONTENT]
    for shape in ((1100, 36), (300, 400)):
        cases += [shape + (k,) for k in ALL_CONTENT]
    cases += [(131, 1031, "scene"), (131, 1031, "noise")]
    # the grid-stride loops: n = 1 120 000 > 2^20 = 4096 blocks x 256 (streaming passes), and the first band, 105 x 2800 =
    # 294 000 pixels > 262 144 = 1024 blocks x 256 (k_sal_band); the oracle takes ~1 s here
    cases += [(400, 2800, "scene")]
    return cases


@pytest.mark.parametrize("rows,cols,kind", _weight_cases())
def test_saliency_weights_match_oracle_at_half_tile(gpu, rows, cols, kind):
    import patolette_amd as p
    tile = _half_tile(rows, cols)
    got = p.saliency_weights(cols, rows, _rgb(kind, rows, cols).reshape(-1, 3), tile)
    _check_weights(got, _weights_want(kind, rows, cols, tile), rows, cols, tile)


def test_saliency_weights_match_oracle_at_default_tile(gpu):
    import patolette_amd as p
    rows, cols = 300, 400
    got = p.saliency_weights(cols, rows, _rgb("scene", rows, cols).reshape(-1, 3))
    _check_weights(got, _weights_want("scene", rows, cols, 512.0), rows, cols, 512.0)


def test_saliency_weights_grey_image_clean_outcome(gpu):
    """R = G = B: the Lab covariance is rank-deficient up to rounding, the reference's own answer is rounding noise -> no parity.
    Either the singular-covariance error, or finite weights in range that a second identical call reproduces bit for bit."""
    import patolette_amd as p
    rows, cols = 120, 160
    g8 = np.round(scene(rows, cols, 9).mean(axis=2) * 255)
    colors = np.repeat((g8 / 255).reshape(-1, 1), 3, axis=1)
    tile = _half_tile(rows, cols)
    try:
        first = p.saliency_weights(cols, rows, colors, tile)
    except np.linalg.LinAlgError:
        return
    assert np.all(np.isfinite(first)) and np.all(first >= 1.0) and np.all(first <= 1.0 + rows * cols / tile ** 2)
    second = p.saliency_weights(cols, rows, colors, tile)
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))


def test_saliency_weights_are_reproducible_across_other_shapes(gpu):
    """devutil.h: exact binned sums, integer-keyed maxima -> the same call gives the same bits, whatever ran in between."""
    import patolette_amd as p
    rows, cols = 300, 400
    colors = _rgb("scene", rows, cols).reshape(-1, 3)
    tile = _half_tile(rows, cols)
    first = p.saliency_weights(cols, rows, colors, tile)
    p.saliency_weights(1031, 131, _rgb("noise", 131, 1031).reshape(-1, 3), _half_tile(131, 1031))
    p.saliency_weights(2800, 400, _rgb("scene", 400, 2800).reshape(-1, 3), _half_tile(400, 2800))
    second = p.saliency_weights(cols, rows, colors, tile)
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
    _check_weights(second, _weights_want("scene", rows, cols, tile), rows, cols, tile)


@pytest.mark.parametrize("rows,cols", [(131, 259), (1100, 36)])
@pytest.mark.parametrize("channels", [3, 4])
def test_three_sources_agree(gpu, rows, cols, channels):
    """The 8-bit entry (companding from the 256-entry table), the planar f64 entry and the row-major f64 entry derive the same
    weights: palette and map are the same bits as the planar entry fed saliency_weights' output -- which the tests above hold to
    the oracle."""
    import patolette_amd as p
    K, tile = 24, _half_tile(rows, cols)
    kw = dict(kmeans_niter=2, kmeans_max_samples=8192)
    rgb8 = np.round(_rgb("scene", rows, cols) * 255).astype(np.uint8)
    img8 = rgb8 if channels == 3 else np.concatenate([rgb8, np.full((rows, cols, 1), 255, dtype=np.uint8)], axis=2)
    c8 = rgb8.reshape(-1, 3).astype(np.float64)
    c8 /= 255
    ok8, _, pm8, _, palf, msg = p.quantize_u8(img8, K, tile_size=tile, **kw)
    assert ok8, msg
    w = p.saliency_weights(cols, rows, c8, tile)
    want = _weights_want_8bit(rows, cols, tile)
    assert np.allclose(w, want, rtol=1e-9, atol=0), np.max(np.abs(w - want) / want)
    planar = np.asfortranarray(c8)
    ok1, pal1, pm1, msg = p.quantize(cols, rows, planar, K, tile_size=0, weights=w, **kw)
    assert ok1, msg
    assert np.array_equal(palf, pal1) and np.array_equal(pm8.reshape(-1).astype(np.uintp), pm1)
    ok2, pal2, pm2, msg = p.quantize(cols, rows, np.ascontiguousarray(c8), K, tile_size=tile, **kw)       # row-major entry, derived
    assert ok2, msg
    assert np.array_equal(pal2, pal1) and np.array_equal(pm2, pm1)
    ok3, pal3, pm3, msg = p.quantize(cols, rows, planar, K, tile_size=tile, **kw)                        # planar entry, derived
    assert ok3, msg
    assert np.array_equal(pal3, pal1) and np.array_equal(pm3, pm1)


@functools.lru_cache(maxsize=None)
def _weights_want_8bit(rows, cols, tile):
    from oracle import saliency
    c8 = np.round(_rgb("scene", rows, cols) * 255).astype(np.uint8).astype(np.float64) / 255
    return saliency.get_weights(c8, tile)


# ---------------------------------------------------------------------------------------------------------------------------
# the constant-mean image
# ---------------------------------------------------------------------------------------------------------------------------
def _c_quantize_rows(native, cols, rows, colors, K, tile):
    """patolette_amd_quantize_rows through the C ABI: its exit code."""
    colors = np.ascontiguousarray(colors, dtype=np.float64)
    opts = native.QuantizationOptions(True, False, 2, 2, 8192, False)
    pal = np.zeros(3 * K)
    pmap = np.zeros(rows * cols, dtype=np.uintp)
    code = C.c_int(99)
    native.lib().patolette_amd_quantize_rows(cols, rows, colors.ctypes.data_as(native.dp), None, float(tile), K, C.byref(opts),
                                             pal.ctypes.data_as(native.dp), pmap.ctypes.data_as(native.zp), C.byref(code))
    return code.value


@pytest.mark.parametrize("rows,cols", [(40, 40), (67, 130)])
def test_constant_channel_mean_is_reported_not_weighted_with_nan(gpu, native, ob, rows, cols):
    """Every pixel a permutation of (0.25, 0.5, 0.75): the colours vary, their mean is 0.5 everywhere, the barrier distance is 0
    everywhere and the reference's weights are NaN (tests/test_oracle_saliency.py).

    Before this test existed the stage divided by the zero maximum: D / dmax = 0 / 0, fmax dropped the NaNs, the folded maxima
    stayed -inf.  Measured on that build at 40 x 40: `patolette_amd_saliency_weights` returned 0 with 1600 of 1600 weights NaN, and
    `quantize(tile_size=64)`, which feeds those weights to the quantisers, had not returned after 120 s and was killed (the
    8-bit entry was not tried after that).

    Now: the stage flags a folded maximum that is 0 or not finite (kSalDegenerate = -4, beside `singular`), the full-path entries
    report exit code -7, Python raises ValueError with that code's message, and the thread's engine stays usable."""
    import patolette_amd as p
    from oracle import saliency
    L = native.lib()
    msg7 = L.get_patolette_exit_code_info_message(-7).decode()
    assert "degenerate" in msg7 and "NaN" in msg7 and L.get_patolette_exit_code_info_message(-8) is None
    img = constant_mean_image(rows, cols, rows + cols)
    colors = img.reshape(-1, 3)
    # the stage alone: C ABI -4 and nothing non-finite handed out as a success; Python ValueError
    out = np.zeros(rows * cols)
    planar = np.asfortranarray(colors)
    rc = L.patolette_amd_saliency_weights(cols, rows, planar.ctypes.data_as(native.dp), 20.0, out.ctypes.data_as(native.dp))
    assert rc == -4, (rc, np.isfinite(out).all())
    with pytest.raises(ValueError) as ei:
        p.saliency_weights(cols, rows, colors, 20.0)
    assert str(ei.value) == msg7
    # quantize with tile_size > 0: exit code -7 / ValueError (both f64 layouts)
    assert _c_quantize_rows(native, cols, rows, colors, 8, 64.0) == -7
    for data in (colors, planar):
        with pytest.raises(ValueError) as ei:
            p.quantize(cols, rows, data, 8, tile_size=64, kmeans_niter=2, kmeans_max_samples=8192)
        assert str(ei.value) == msg7
    # the 8-bit entry: bytes 64 / 128 / 192 (multiples of a quarter of 256) -- the f32 channel mean the device forms is one constant
    b = np.array([64, 128, 192], dtype=np.float64) / 255
    means = {np.float32(((b[i] + b[j]) + b[k]) / 3.0) for i, j, k in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))}
    assert len(means) == 1
    img8 = np.round(img * 256).astype(np.uint8)
    assert set(np.unique(img8)) == {64, 128, 192}
    for im in (img8, np.concatenate([img8, np.full((rows, cols, 1), 255, dtype=np.uint8)], axis=2)):
        with pytest.raises(ValueError) as ei:
            p.quantize_u8(im, 8, tile_size=64, kmeans_niter=2, kmeans_max_samples=8192)
        assert str(ei.value) == msg7
    # tile_size = 0 derives nothing: the image itself is quantisable
    ok, pal, pmap, msg = p.quantize(cols, rows, colors, 6, tile_size=0, kmeans_niter=0)
    assert ok and np.all(np.isfinite(pal)), msg
    # the engine that failed serves the next ordinary call, and it matches the oracle
    good = scene(rows, cols, 21)
    tile = _half_tile(rows, cols)
    got = p.saliency_weights(cols, rows, good.reshape(-1, 3), tile)
    _check_weights(got, saliency.get_weights(good, tile), rows, cols, tile)


def test_singular_border_still_wins_over_degenerate_map(gpu):
    """A flat image is both (constant mean, singular covariance): the reference raises LinAlgError before it divides."""
    import patolette_amd as p
    with pytest.raises(np.linalg.LinAlgError):
        p.saliency_weights(40, 40, np.full((1600, 3), 0.25), 20.0)
