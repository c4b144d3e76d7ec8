"""The masked Riemersma restatement (tests/rgba_ref.py) is the reference's own walk, checked against the CPU oracle alone.

  * all pixels opaque: the restatement is oracle.dither bit for bit (square and non-square shapes);
  * opaque iff x < W' with W' x H at the same Hilbert level as W x H: the reference's square is the same, so the in-image walk of
    the narrow image IS the masked walk of the wide one -- the restatement on the wide image equals oracle.dither of the narrow
    one, pixel numbers remapped.
(The oracle is never run on a 1 x M image: its square would be M x M.)"""
import numpy as np
import pytest

from tests import rgba_ref


def _inputs(ob, n, K, seed):
    flat = ob.image(n, seed)
    img = ob.convert("srgb_to_rec2020", flat.copy())
    pal = np.random.default_rng(seed).random((K, 3))
    pal = ob.convert("srgb_to_rec2020", ob.planar(pal).copy()).reshape(3, K).T.copy()
    return img, img.reshape(3, n).T.copy(), pal


@pytest.mark.parametrize("w,h,K", [(16, 16, 4), (37, 23, 16), (9, 64, 7), (64, 5, 32), (2, 1, 2)])
def test_all_opaque_is_the_oracle_walk(ob, w, h, K):
    n = w * h
    flat, rows, pal = _inputs(ob, n, K, 3 + w)
    want = ob.dither(flat, w, h, pal).astype(np.int64)
    got = rgba_ref.masked_dither(ob, rows, w, h, pal, np.ones(n, bool))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("w,h,wn,K", [(40, 30, 33, 8), (64, 40, 37, 16), (23, 50, 17, 5), (30, 17, 29, 12)])
def test_narrow_image_is_the_masked_wide_image(ob, w, h, wn, K):
    assert rgba_ref.hilbert_level(w, h) == rgba_ref.hilbert_level(wn, h)
    n = w * h
    _, rows, pal = _inputs(ob, n, K, 11 + wn)
    x = np.arange(n) % w
    opaque = x < wn
    got = rgba_ref.masked_dither(ob, rows, w, h, pal, opaque)
    assert np.all(got[~opaque] == -1)
    narrow = rows.reshape(h, w, 3)[:, :wn, :].reshape(-1, 3)
    want = ob.dither(ob.planar(narrow), wn, h, pal).astype(np.int64)
    np.testing.assert_array_equal(got.reshape(h, w)[:, :wn].reshape(-1), want)


def test_transparent_pixels_leave_the_queue_alone(ob):
    # a mask that drops pixels in the middle of the walk: the choices before the first hole are the unmasked chain's, and the
    # chain after it is the chain over the remaining pixels (not the unmasked one shifted)
    w, h, K = 32, 32, 6
    n = w * h
    flat, rows, pal = _inputs(ob, n, K, 5)
    order = ob.hilbert_order(w, h).astype(np.int64)
    opaque = np.ones(n, bool)
    opaque[order[300:340]] = False
    got = rgba_ref.masked_dither(ob, rows, w, h, pal, opaque)
    full = ob.dither(flat, w, h, pal).astype(np.int64)
    np.testing.assert_array_equal(got[order[:300]], full[order[:300]])
    assert np.all(got[order[300:340]] == -1)
    rest = rgba_ref.chain(rows, order[:300].tolist() + order[340:].tolist(), pal)
    np.testing.assert_array_equal(got[order[340:]], [rest[int(p)] for p in order[340:]])
