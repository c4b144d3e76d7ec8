"""ColorHistogram on the GPU against the integer model of tests/hist_ref.py: every export is compared bit for bit.

  1. sizes: n x 1 images of 7 colours for every n in 1..130 and around 256, 4096, 65536 -- 3 and 4 channels, numpy arrays and CUDA
     tensors, tensors that start 0..3 bytes into a larger buffer (the bytewise loader);
  2. key layout, 3. contention on one bin, 4. chunk invariance (whole, by frame, reversed, row slabs, merged) of export and palette;
  5. the full table: all 2^24 colours;
  6. weights: the rounding cases, weight 0, refused adds (the export is unchanged), overflow in one call, across calls, in one row,
     in a merge, and inside one block's LDS table (an image large enough for a block to walk two tiles);
  7. derived weights equal the per-frame saliency weights given explicitly; a frame that fails saliency changes nothing;
  8. alpha thresholds; 9. the palette: the quantiser's result bit for bit, the colours themselves up to K, zero weights dropped,
     and better than the fixed 6x6x6 cube on a clip.
Two tables (unweighted 128 MB, weighted 256 MB) serve the whole module; every test clears the one it uses first."""
import numpy as np
import pytest

from tests import hist_ref
from tests.util import scene

pytestmark = pytest.mark.gpu

SIZES = list(range(1, 131)) + [255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537]
SEVEN = np.array([[0, 0, 0], [255, 255, 255], [12, 200, 7], [12, 200, 8], [200, 12, 7], [90, 90, 90], [1, 0, 255]], dtype=np.uint8)


@pytest.fixture(scope="module")
def hist(gpu):
    import patolette_amd as p
    with p.ColorHistogram() as h:
        yield h


@pytest.fixture(scope="module")
def whist(gpu):
    import patolette_amd as p
    with p.ColorHistogram(weighted=True) as h:
        yield h


def seven(n, channels, seed):
    """n x 1 pixels drawn from 7 colours, runs of equal colours included; a 4th channel is noise"""
    rng = np.random.default_rng(seed)
    idx = np.repeat(rng.integers(0, 7, n), rng.integers(1, 4, n))[:n]
    px = SEVEN[idx]
    if channels == 4:
        px = np.concatenate([px, rng.integers(0, 256, (n, 1), dtype=np.uint8)], axis=1)
    return np.ascontiguousarray(px.reshape(n, 1, channels))


def same_export(h, want):
    colors, counts, weights = h.export()
    wc, wn, ww = want
    assert colors.dtype == np.uint8 and counts.dtype == np.int64 and weights.dtype == np.float64
    assert colors.shape == wc.shape and np.array_equal(colors, wc)
    assert np.array_equal(counts, wn)
    assert np.array_equal(weights.view(np.uint64), ww.view(np.uint64))
    assert h.pixels == int(wn.sum()) and h.colors == len(wn)


def clip(f, h, w, seed):
    """half smooth scene, half noise"""
    rng = np.random.default_rng(seed)
    fr = np.stack([np.round(scene(h, w, seed + 3 * i) * 255).astype(np.uint8) for i in range(f)])
    fr[:, :, w // 2:] = rng.integers(0, 256, (f, h, w - w // 2, 3), dtype=np.uint8)
    return np.ascontiguousarray(fr)


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 4])
def test_sizes_numpy(hist, channels):
    for n in SIZES:
        px = seven(n, channels, n)
        same_export(hist.clear().add(px), hist_ref.model(px))


def test_sizes_tensors_and_misaligned_starts(gpu):
    """CUDA tensors go through patolette_amd_hist_add_u8_device where they lie; a tensor that starts 1, 2 or 3 bytes into its buffer
    takes the bytewise loader.  Own process: torch loads its HIP runtime before libpatolette_amd.so does."""
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
from tests import hist_ref
from tests.test_gpu_hist import SIZES, seven, same_export
with p.ColorHistogram() as h:
    for channels in (3, 4):
        for n in SIZES:
            px = seven(n, channels, n)
            want = hist_ref.model(px)
            for off in ((0, 1, 2, 3) if n <= 70 or n >= 255 else (n %% 4,)):
                buf = torch.zeros(n * channels + 3, dtype=torch.uint8, device="cuda")
                t = buf[off:off + n * channels].view(n, 1, channels)
                t.copy_(torch.from_numpy(px))
                assert t.is_contiguous() and t.data_ptr() %% 4 == (buf.data_ptr() + off) %% 4
                same_export(h.clear().add(t), want)
    frames = torch.from_numpy(np.stack([seven(300, 4, s).reshape(20, 15, 4) for s in range(3)])).cuda()
    same_export(h.clear().add(frames, alpha_threshold=100), hist_ref.model(frames.cpu().numpy(), None, 100))
with p.ColorHistogram(weighted=True) as hw:
    px = seven(5000, 3, 1)
    w = np.random.default_rng(3).random(5000) * 3
    same_export(hw.add(torch.from_numpy(px).cuda(), weights=torch.from_numpy(w).cuda()), hist_ref.model(px, w))
    same_export(hw.clear().add(torch.from_numpy(px).cuda(), weights=w), hist_ref.model(px, w))
print("TORCH-HIST-OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "TORCH-HIST-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 2. key layout ----------------------------------------------------------------------------------------------------------------
def test_key_layout(hist):
    cols = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.uint8)
    mult = np.array([3, 5, 7, 11, 13, 17, 19, 23])
    px = np.repeat(cols, mult, axis=0)
    px = px[np.random.default_rng(0).permutation(len(px))].reshape(-1, 1, 3)
    colors, counts, weights = hist.clear().add(px).export()
    # ascending by R << 16 | G << 8 | B
    assert colors.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 255], [0, 1, 0], [0, 255, 0], [1, 0, 0], [255, 0, 0], [255, 255, 255]]
    assert counts.tolist() == [3, 23, 13, 19, 11, 17, 7, 5]
    assert weights.tolist() == [3.0, 23.0, 13.0, 19.0, 11.0, 17.0, 7.0, 5.0]
    same_export(hist, hist_ref.model(px))


# ---- 3. contention ----------------------------------------------------------------------------------------------------------------
def test_contention_on_one_bin(hist):
    n = 300000
    px = np.empty((n, 1, 3), dtype=np.uint8)
    px[:] = (17, 34, 51)
    hist.clear().add(px)
    assert hist.pixels == n and hist.colors == 1
    colors, counts, weights = hist.export()
    assert colors.tolist() == [[17, 34, 51]] and counts.tolist() == [n] and weights.tolist() == [float(n)]
    hist.add(px)
    assert hist.pixels == 2 * n and hist.colors == 1
    assert hist.export()[1].tolist() == [2 * n]


# ---- 4. chunk invariance ----------------------------------------------------------------------------------------------------------
def _ways(f, rows):
    """name -> for each histogram the (frames, rows) index pairs of the chunks it gets, in the order it gets them"""
    whole = slice(None)
    yield "whole", [[(whole, whole)]]
    yield "by frame", [[(i, whole) for i in range(f)]]
    yield "reversed", [[(i, whole) for i in reversed(range(f))]]
    yield "row slabs", [[(whole, slice(r, r + 5)) for r in range(0, rows, 5)]]
    yield "merged", [[(slice(0, 3), whole)], [(slice(3, f), whole)]]


@pytest.mark.parametrize("weighted", [False, True])
def test_chunk_invariance(gpu, hist, whist, weighted):
    import patolette_amd as p
    fr = clip(8, 36, 64, 5)
    w = np.random.default_rng(9).random(fr.shape[:3]) * 4 if weighted else None
    h = whist if weighted else hist
    want = hist_ref.model(fr, w)
    first = None
    with p.ColorHistogram(weighted=weighted) as second:
        for name, parts in _ways(fr.shape[0], fr.shape[1]):
            h.clear()
            second.clear()
            for target, chunks in zip((h, second), parts):
                for at in chunks:
                    target.add(np.ascontiguousarray(fr[at]), weights=np.ascontiguousarray(w[at]) if weighted else None)
            if len(parts) == 2:
                h.merge(second)
            same_export(h, want)
            ok, pal8, pal, msg = h.palette(16, kmeans_niter=4, kmeans_max_samples=4096)
            assert ok, msg
            if first is None:
                first = (pal8, pal)
            assert np.array_equal(pal8, first[0]) and np.array_equal(pal.view(np.uint64), first[1].view(np.uint64)), name


# ---- 5. the full table --------------------------------------------------------------------------------------------------------------
def test_full_table(hist):
    k = np.random.default_rng(1).permutation(1 << 24).astype(np.uint32)
    px = np.stack([k >> 16, (k >> 8) & 255, k & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    hist.clear().add(px).add(px[:64])
    assert hist.colors == 1 << 24 and hist.pixels == (1 << 24) + 64 * 4096
    colors, counts, weights = hist.export()
    keys = colors[:, 0].astype(np.int64) << 16 | colors[:, 1].astype(np.int64) << 8 | colors[:, 2]
    assert np.array_equal(keys, np.arange(1 << 24))
    want = np.ones(1 << 24, dtype=np.int64)
    want[k[:64 * 4096]] = 2
    assert np.array_equal(counts, want) and np.array_equal(weights, want.astype(np.float64))


# ---- 6. weights -------------------------------------------------------------------------------------------------------------------
def test_weight_rounding(whist):
    cases = np.array([2.0 ** -33, 3 * 2.0 ** -33, 1.0, 2.0 ** 20, 0.0, 5 * 2.0 ** -33, 0.3, 1e-12, 7.25])
    rng = np.random.default_rng(2)
    for colours in (1, 7):
        n = 4000
        px = SEVEN[rng.integers(0, colours, n)].reshape(n, 1, 3)
        w = cases[rng.integers(0, len(cases), n)]
        same_export(whist.clear().add(px, weights=w), hist_ref.model(px, w))
    # one pixel per rounding case: the sums are the cases themselves
    for v, u in ((2.0 ** -33, 0), (3 * 2.0 ** -33, 2), (1.0, 2 ** 32), (2.0 ** 20, 2 ** 52)):
        colors, counts, weights = whist.clear().add(SEVEN[2:3].reshape(1, 1, 3), weights=[v]).export()
        assert counts.tolist() == [1] and weights.tolist() == [u / 2.0 ** 32]


def test_weight_zero_is_exported(whist):
    px = SEVEN[[3, 3, 4]].reshape(3, 1, 3)
    colors, counts, weights = whist.clear().add(px, weights=[0.0, 0.0, 0.0]).export()
    assert colors.tolist() == [[12, 200, 8], [200, 12, 7]] and counts.tolist() == [2, 1] and weights.tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        whist.palette(4)                                                # no colour with a weight above 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -2.0 ** -40, 2.0 ** 20 + 1])
def test_refused_add_changes_nothing(whist, bad):
    n = 5000
    px = seven(n, 3, 4)
    w0 = np.random.default_rng(5).random(n)
    before = whist.clear().add(px, weights=w0).export()
    for at in (0, n // 2 + 1, n - 1):
        w = w0.copy()
        w[at] = bad
        with pytest.raises(ValueError):
            whist.add(px, weights=w)
        after = whist.export()
        for a, b in zip(before, after):
            assert np.array_equal(a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1))
    same_export(whist, hist_ref.model(px, w0))


def _one_colour(n, shape=None):
    px = np.empty((n, 1, 3) if shape is None else shape + (3,), dtype=np.uint8)
    px[:] = (9, 8, 7)
    return px


def test_overflow(gpu, whist):
    import patolette_amd as p
    big = 2.0 ** 20
    # 4095 * 2^52 units fit
    colors, counts, weights = whist.clear().add(_one_colour(4095), weights=np.full(4095, big)).export()
    assert counts.tolist() == [4095] and weights.tolist() == [4095 * big]
    # one more in a later call
    with pytest.raises(OverflowError):
        whist.add(_one_colour(1), weights=[big])
    with p.ColorHistogram(weighted=True) as other:
        for use in (lambda: whist.add(_one_colour(1), weights=[0.0]), lambda: whist.merge(other), lambda: other.merge(whist),
                    lambda: whist.pixels, lambda: whist.colors, lambda: whist.export(), lambda: whist.palette(4)):
            with pytest.raises(OverflowError):
                use()
        # merge: 4095 + 1
        whist.clear().add(_one_colour(4095), weights=np.full(4095, big))
        other.add(_one_colour(1), weights=[big])
        with pytest.raises(OverflowError):
            whist.merge(other)
        with pytest.raises(OverflowError):
            whist.export()
        assert other.export()[1].tolist() == [1]
    # one more in the same call, as a column and as the row the issue names.  At this size a block walks one tile of 2048 pixels, so
    # two blocks hold 2^63 units each and the wrap is met at the global bin; test_overflow_inside_one_block wraps a block's own sum
    for px in (_one_colour(4096), _one_colour(0, (1, 4096))):
        with pytest.raises(OverflowError):
            whist.clear().add(px, weights=np.full(4096, big))
        with pytest.raises(OverflowError):
            whist.export()
    # clear makes it usable again
    same_export(whist.clear().add(_one_colour(10), weights=np.full(10, 0.5)), hist_ref.model(_one_colour(10), np.full(10, 0.5)))


@pytest.mark.parametrize("start", [0, 37 * 4096])
def test_overflow_inside_one_block(whist, start):
    """The in-block partial sum.  2048 x 2048 pixels are 2048 tiles; from 2 * 4 * 256 tiles on a block walks two tiles or more, so
    4096 consecutive pixels that begin at a multiple of 4096 -- both starts here lie inside one block's stretch whether a block
    walks 2, 4 or 8 tiles -- are summed by ONE block: 256 lanes' runs of 2^56 units meet in one LDS slot and make exactly 2^64 there.  Every other pixel is
    another colour at weight 0, so nothing but the slot's own carry can tell: a slot that wrapped to 0 unnoticed would be skipped by
    the flush and the add would succeed with weight 0."""
    n, big = 2048 * 2048, 2.0 ** 20
    px = np.zeros((2048, 2048, 3), dtype=np.uint8)
    flat = px.reshape(-1, 3)
    flat[start:start + 4096] = (9, 8, 7)
    w = np.zeros(n)
    w[start:start + 4096] = big
    with pytest.raises(OverflowError):
        whist.clear().add(px, weights=w)
    with pytest.raises(OverflowError):
        whist.export()
    # one unit-carrying pixel less fits, in the same block: 4095 * 2^52 units
    w[start + 2077] = 0.0
    colors, counts, weights = whist.clear().add(px, weights=w).export()
    assert colors.tolist() == [[0, 0, 0], [9, 8, 7]] and counts.tolist() == [n - 4096, 4096] and weights.tolist() == [0.0, 4095 * big]
    # the same 4096 pixels across two blocks' stretches: 2^63 in each, met at the global bin
    w[:] = 0.0
    w[start + 2048:start + 2048 + 4096] = big
    flat[:] = 0
    flat[start + 2048:start + 2048 + 4096] = (9, 8, 7)
    with pytest.raises(OverflowError):
        whist.clear().add(px, weights=w)


# ---- 7. derived weights -------------------------------------------------------------------------------------------------------------
def test_derived_weights_are_the_frames_saliency_weights(whist):
    import patolette_amd as p
    f, h, w = 3, 90, 120                                                # the derived-weights case of tests/test_gpu_frames.py
    fr = np.stack([np.round(scene(h, w, 2 + 7 * i) * 255).astype(np.uint8) for i in range(f)])
    wts = np.concatenate([p.saliency_weights(w, h, fr[i].reshape(-1, 3) / 255.0, 64) for i in range(f)])
    derived = whist.clear().add(fr, tile_size=64).export()
    same_export(whist.clear().add(fr, weights=wts), derived)
    same_export(whist, hist_ref.model(fr, wts))
    # a frame whose border is constant fails saliency as quantize_frames does; nothing has entered, the earlier frames included
    bad = fr.copy()
    bad[2, :14] = bad[2, -14:] = 80
    bad[2, :, :14] = bad[2, :, -14:] = 80
    with pytest.raises((ValueError, np.linalg.LinAlgError)) as expected:
        p.quantize_frames(bad, 8, tile_size=64, dither=False)
    with pytest.raises(expected.type):
        whist.add(bad, tile_size=64)
    same_export(whist, derived)


# ---- 8. alpha ---------------------------------------------------------------------------------------------------------------------
def test_alpha_thresholds(hist):
    rng = np.random.default_rng(6)
    px = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    px[..., :3] //= 64                                                  # few colours: every key meets every alpha
    px[0, :6, 3] = (0, 1, 127, 128, 254, 255)
    for thr in (0, 1, 128, 255):
        same_export(hist.clear().add(px, alpha_threshold=thr), hist_ref.model(px, None, thr))
    same_export(hist.clear().add(px), hist_ref.model(px))               # no threshold: every pixel enters
    px[..., 3] = 0
    hist.clear().add(px, alpha_threshold=1)
    assert hist.pixels == 0 and hist.colors == 0 and hist.export()[0].shape == (0, 3)
    with pytest.raises(ValueError):
        hist.palette(8)


# ---- 9. the palette -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_palette_is_the_quantisers(hist, whist, weighted):
    import patolette_amd as p
    img = np.round(scene(64, 96, 8) * 255).astype(np.uint8)
    h = whist if weighted else hist
    if weighted:
        h.clear().add(img, weights=0.25 + np.random.default_rng(7).random((64, 96)))
    else:
        h.clear().add(img)
    colors, counts, weights = h.export()
    assert len(colors) > 257
    for K in (2, 16, 256):
        for cs in (p.ColorSpace_ICtCp, p.ColorSpace_CIELuv):
            for niter in (0, 32):
                ok, pal8, pal, msg = h.palette(K, color_space=cs, kmeans_niter=niter)
                ref = p.quantize_u8(colors[None], K, dither=False, tile_size=0, weights=weights, want_quantized=False, color_space=cs,
                                    kmeans_niter=niter)
                assert ok and ref[0], (msg, ref[-1])
                assert pal8.dtype == np.uint8 and np.array_equal(pal8, ref[1]), (K, cs, niter)
                assert np.array_equal(pal.view(np.uint64), ref[4].view(np.uint64)), (K, cs, niter)


def _distinct(m, seed):
    k = np.sort(np.random.default_rng(seed).choice(1 << 24, m, replace=False))
    return np.stack([k >> 16, (k >> 8) & 255, k & 255], axis=1).astype(np.uint8)


def test_palette_of_few_colours_is_those_colours(hist):
    import patolette_amd as p
    cols = _distinct(200, 1)
    img = cols[np.random.default_rng(2).integers(0, 200, (40, 50))]
    img.reshape(-1, 3)[:200] = cols[::-1]                               # every colour is there
    ok, pal8, pal, msg = hist.clear().add(img).palette(256)
    assert ok, msg
    assert np.array_equal(pal8[:200], cols) and not pal8[200:].any()
    assert np.array_equal(pal[:200], cols / 255.0) and np.all(pal[200:] == -1.0) and pal.flags.f_contiguous
    ok, maps, quant, msg = p.remap(img, pal, dither=False)
    assert ok and np.array_equal(quant, img)
    ok, entries, per_frame, _, msg = p.measure(img, maps, pal, ictcp=False)
    assert ok and per_frame[:, 1].sum() == 0 and per_frame[:, 0].sum() == img.shape[0] * img.shape[1]
    # either side of the rule: 256 colours at K = 256 are returned, 257 are quantised
    cols = _distinct(257, 3)
    ok, pal8, pal, msg = hist.clear().add(cols[:256].reshape(16, 16, 3)).palette(256, kmeans_niter=2)
    assert ok and np.array_equal(pal8, cols[:256]) and np.array_equal(pal, cols[:256] / 255.0)
    ok, pal8, pal, msg = hist.add(cols[256:].reshape(1, 1, 3)).palette(256, kmeans_niter=2)
    colors, counts, weights = hist.export()
    assert np.array_equal(colors, cols)
    ref = p.quantize_u8(colors[None], 256, dither=False, tile_size=0, weights=weights, want_quantized=False, kmeans_niter=2)
    assert ok and ref[0] and np.array_equal(pal8, ref[1]) and np.array_equal(pal.view(np.uint64), ref[4].view(np.uint64))
    assert not np.array_equal(pal8, cols[:256])


def test_zero_weight_colours_do_not_count(whist):
    cols = _distinct(300, 4)
    w = np.ones(300)
    w[::3] = 0.0                                                        # 100 colours weigh nothing: M' = 200 <= 256
    px = np.concatenate([cols, cols]).reshape(600, 1, 3)
    ok, pal8, pal, msg = whist.clear().add(px, weights=np.concatenate([w, w])).palette(256)
    assert ok, msg
    assert whist.colors == 300
    keep = cols[w > 0]
    assert np.array_equal(pal8[:200], keep) and not pal8[200:].any()
    assert np.array_equal(pal[:200], keep / 255.0) and np.all(pal[200:] == -1.0)


def test_palette_beats_the_colour_cube(hist):
    """A condition, not a measurement: on an 8 x 90 x 160 clip whose colours sit in the sub-cube [64, 192)^3, the nearest remap onto
    palette(256) has a lower total sse than onto the fixed 6x6x6 cube.  On the CPU (the oracle's patolette() on the clip's distinct
    colours with their counts as weights, then its nearest map) the clip leaves a wide gap: sse 10 623 852 against 109 671 608 for
    the cube, a factor of 10."""
    import patolette_amd as p
    fr = cube_clip()
    ok, pal8, pal, msg = hist.clear().add(fr).palette(256)
    assert ok, msg
    v = np.array([0, 51, 102, 153, 204, 255], dtype=np.uint8)
    cube = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)
    sse = []
    for palette in (pal, cube):
        ok, maps, _, msg = p.remap(fr, palette, dither=False, want_quantized=False)
        assert ok, msg
        ok, _, per_frame, _, msg = p.measure(fr, maps, palette, ictcp=False)
        assert ok, msg
        sse.append(int(per_frame[:, 1].sum()))
    print("sse onto palette(256): %d, onto the 6x6x6 cube: %d" % tuple(sse))
    assert sse[0] < sse[1]


def cube_clip():
    """the clip of the chunk test at 8 x 90 x 160, its colours squeezed into [64, 192)^3"""
    return (clip(8, 90, 160, 5) // 2 + 64).astype(np.uint8)
