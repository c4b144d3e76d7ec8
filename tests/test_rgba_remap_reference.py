"""The remap with alpha: its reference (tests/rgba_remap_ref.py) against its consequences on the CPU oracle alone, and every
ValueError of remap_rgba and quantize_rgba_frames, each raised before the library is touched."""
import os

import numpy as np
import pytest

from tests import ordered_ref, remap_ref, rgba_ref, rgba_remap_ref
from tests.util import ROOT, scene


def _frames(f, h, w, seed=3):
    rng = np.random.default_rng(seed)
    rgb = np.stack([np.round(scene(h, w, seed + i) * 255).astype(np.uint8) for i in range(f)])
    alpha = np.where(rng.random((f, h, w)) < 0.4, 0, 255).astype(np.uint8)
    return np.concatenate([rgb, alpha[..., None]], axis=-1)


def _palette_rgba(rows, seed=1):
    rng = np.random.default_rng(seed)
    codes = rng.choice(1 << 24, size=rows - 1, replace=False)
    pal = np.zeros((rows, 4), dtype=np.uint8)
    pal[1:, 0], pal[1:, 1], pal[1:, 2], pal[1:, 3] = codes >> 16, (codes >> 8) & 255, codes & 255, 255
    return pal


@pytest.mark.parametrize("mode", [rgba_remap_ref.NEAREST, rgba_remap_ref.RIEMERSMA, rgba_remap_ref.ORDERED])
def test_consequences(ob, mode):
    f, h, w = 2, 20, 28
    frames, prgba = _frames(f, h, w), _palette_rgba(9)
    maps, quant, _ = rgba_remap_ref.remap_rgba(ob, frames, prgba, mode=mode)
    opaque = frames[..., 3] >= 128
    assert opaque.any() and not opaque.all()
    assert np.all(maps[~opaque] == 0) and np.all(maps[opaque] >= 1) and maps.max() <= 8
    assert np.array_equal(quant, prgba[maps])
    assert np.all(quant[~opaque] == 0) and np.all(quant[opaque][:, 3] == 255)
    rgb_pal = np.ascontiguousarray(prgba[1:, :3])
    if mode == rgba_remap_ref.NEAREST:
        inner, _ = remap_ref.remap(ob, frames, rgb_pal, dither=False)
        assert np.array_equal(maps[opaque], 1 + inner[opaque])
    elif mode == rgba_remap_ref.ORDERED:
        inner, _, _ = ordered_ref.remap(ob, frames, rgb_pal, ordered_ref.ordered_spread(rgb_pal))
        assert np.array_equal(maps[opaque], 1 + inner[opaque])
        m0, q0, _ = rgba_remap_ref.remap_rgba(ob, frames, prgba, mode=mode, spread=0.0)
        mn, qn, _ = rgba_remap_ref.remap_rgba(ob, frames, prgba, mode=rgba_remap_ref.NEAREST)
        assert np.array_equal(m0, mn) and np.array_equal(q0, qn)
    else:
        # the RGB under transparent pixels cannot matter, frames are walked one by one, and the walk is not the nearest map
        hidden = frames.copy()
        hidden[~opaque, :3] = 77
        assert np.array_equal(rgba_remap_ref.remap_rgba(ob, hidden, prgba, mode=mode)[0], maps)
        for i in range(f):
            assert np.array_equal(rgba_remap_ref.remap_rgba(ob, frames[i], prgba, mode=mode)[0], maps[i])
        assert np.any(maps != rgba_remap_ref.remap_rgba(ob, frames, prgba, mode=rgba_remap_ref.NEAREST)[0])
    # the three palette forms name the same palette
    as_u8 = np.ascontiguousarray(prgba[:, :3])
    as_f = np.full((12, 3), -1.0)
    as_f[:9] = as_u8 / 255.0
    for form in (as_u8, as_f):
        m2, q2, _ = rgba_remap_ref.remap_rgba(ob, frames, form, 0, mode=mode)
        assert np.array_equal(m2, maps) and np.array_equal(q2[..., 3], quant[..., 3])
        assert np.array_equal(q2, rgba_remap_ref.split(form, 0)[2][m2])           # (a float palette's bytes are its own clip-and-truncate)


def test_all_opaque_is_the_rgb_remap(ob):
    frames, prgba = _frames(2, 20, 28), _palette_rgba(9)
    frames[..., 3] = 255
    rgb_pal = np.ascontiguousarray(prgba[1:, :3])
    for mode, dither in ((rgba_remap_ref.NEAREST, False), (rgba_remap_ref.RIEMERSMA, True)):
        inner, q = remap_ref.remap(ob, frames, rgb_pal, dither=dither)
        maps, quant, _ = rgba_remap_ref.remap_rgba(ob, frames, prgba, mode=mode)
        assert np.array_equal(maps, 1 + inner) and np.array_equal(quant[..., :3], q)
        m2, q2, _ = rgba_remap_ref.remap_rgba(ob, frames, rgb_pal, -1, mode=mode)
        assert np.array_equal(m2, inner) and np.array_equal(q2[..., :3], q) and np.all(q2[..., 3] == 255)
    # the masked walk with nothing masked is the oracle's own walk
    h, w = frames.shape[1:3]
    px = frames[0, :, :, :3].reshape(h * w, 3).astype(np.float64) / 255.0
    img = ob.unplanar(ob.convert("srgb_to_rec2020", ob.planar(px)), h * w)
    pmap = ob.unplanar(ob.convert("srgb_to_rec2020", ob.planar(rgb_pal / 255.0)), 8)
    walk = rgba_ref.masked_dither(ob, img, w, h, pmap, np.ones(h * w, dtype=bool)).reshape(h, w)
    assert np.array_equal(walk, remap_ref.remap(ob, frames[0], rgb_pal, dither=True)[0])


def test_two_by_two_written_out(ob):
    """Black, white and a transparent entry; every number by hand.  Nearest in ICtCp: dark grey -> black, light grey -> white."""
    prgba = np.array([[0, 0, 0, 0], [0, 0, 0, 255], [255, 255, 255, 255], [0, 0, 0, 0]], dtype=np.uint8)   # (row 3: unused)
    image = np.array([[[10, 10, 10, 255], [250, 250, 250, 128]],
                      [[255, 255, 255, 127], [240, 240, 240, 0]]], dtype=np.uint8)
    maps, quant, _ = rgba_remap_ref.remap_rgba(ob, image, prgba, mode=rgba_remap_ref.NEAREST)
    assert np.array_equal(maps, [[1, 2], [0, 0]])                  # alpha 128 is opaque, 127 is not
    assert np.array_equal(quant, [[[0, 0, 0, 255], [255, 255, 255, 255]], [[0, 0, 0, 0], [0, 0, 0, 0]]])
    maps, _, _ = rgba_remap_ref.remap_rgba(ob, image, prgba, alpha_threshold=0, mode=rgba_remap_ref.NEAREST)
    assert np.array_equal(maps, [[1, 2], [2, 2]])
    maps, quant, _ = rgba_remap_ref.remap_rgba(ob, image, prgba, alpha_threshold=256, mode=rgba_remap_ref.NEAREST)
    assert not maps.any() and not quant.any()
    # no transparent entry: the same two colours as rows 0 and 1
    maps, quant, _ = rgba_remap_ref.remap_rgba(ob, image, prgba[1:3], alpha_threshold=0, mode=rgba_remap_ref.NEAREST)
    assert np.array_equal(maps, [[0, 1], [1, 1]]) and np.all(quant[..., 3] == 255)


def test_symbols_declared_and_bound():
    import patolette_amd
    from patolette_amd import _native
    with open(os.path.join(ROOT, "include", "patolette_amd.h")) as fh:
        header = fh.read()
    for name in ("patolette_amd_remap_rgba_u8", "patolette_amd_remap_rgba_u8_device", "patolette_amd_debug_rgba_stamp_quad"):
        assert name + "(" in header
        assert name in _native.SYMBOLS
    assert len(_native.SYMBOLS["patolette_amd_remap_rgba_u8"][1]) == 15
    assert _native.SYMBOLS["patolette_amd_remap_rgba_u8"][1] == _native.SYMBOLS["patolette_amd_remap_rgba_u8_device"][1]
    assert "remap_rgba" in patolette_amd.__all__ and "quantize_rgba_frames" in patolette_amd.__all__


def test_symbols_exported(native):
    L = native.lib()                                               # loading needs no GPU
    assert L.patolette_amd_remap_rgba_u8 and L.patolette_amd_remap_rgba_u8_device and L.patolette_amd_debug_rgba_stamp_quad


def test_bad_arguments_raise_before_the_library_is_touched(monkeypatch):
    import patolette_amd
    from patolette_amd import _native

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_native, "lib", no_library)
    good = np.zeros((4, 5, 4), dtype=np.uint8)
    prgba = _palette_rgba(5)
    pal3 = np.ascontiguousarray(prgba[:, :3])

    def bad(*args, **kw):
        with pytest.raises(ValueError):
            patolette_amd.remap_rgba(*args, **kw)

    bad(good.astype(np.float64), prgba)                            # a float image
    bad(good[..., :3], prgba)                                      # three channels
    bad(np.zeros((4, 5), dtype=np.uint8), prgba)
    bad(np.zeros((2, 2, 4, 5, 4), dtype=np.uint8), prgba)
    bad(good, prgba, alpha_threshold=257)
    bad(good, prgba, alpha_threshold=-1)
    bad(good, prgba, alpha_threshold=12.5)
    bad(good, prgba, alpha_threshold=True)
    bad(good, prgba, dither="bayer")
    bad(good, prgba, dither="ordered", spread=-1.0)
    bad(good, prgba, dither="ordered", spread=float("nan"))
    bad(good, prgba, transparent_index=1)
    bad(good, prgba, transparent_index=0.0)
    bad(good, prgba, transparent_index=-1)                         # contradicts the rows: row 0 has alpha 0
    bad(good, prgba[1:], transparent_index=0)                      # contradicts the rows: row 0 has alpha 255
    bad(good, prgba.astype(np.float64))                            # (K, 4) must be bytes
    inner = prgba.copy()
    inner[2, 3] = 0
    bad(good, inner)                                               # an alpha-0 row that is not row 0
    half = prgba.copy()
    half[3, 3] = 128
    bad(good, half)                                                # an alpha that is neither 0 nor 255
    half = prgba.copy()
    half[0, 3] = 7
    bad(good, half)
    bad(good, np.zeros((3, 4), dtype=np.uint8))                    # nothing but unused rows
    bad(good, prgba[:1])                                           # the transparent entry alone
    bad(good, pal3[:1], transparent_index=0)                       # no opaque row left
    bad(good, np.full((3, 3), -1.0))
    only0 = np.full((3, 3), -1.0)
    only0[0] = 0.0
    bad(good, only0, transparent_index=0)
    bad(good, np.zeros((0, 3), dtype=np.uint8))
    bad(good, np.zeros((4, 3), dtype=np.int64))
    bad(good, np.zeros((4, 5), dtype=np.uint8))                    # five columns
    bad(good, np.zeros(4, dtype=np.uint8))

    def bad_frames(*args, **kw):
        with pytest.raises(ValueError):
            patolette_amd.quantize_rgba_frames(*args, **kw)

    frames = np.zeros((2, 4, 5, 4), dtype=np.uint8)
    bad_frames(frames[0], 4)                                       # one image: not a stack
    bad_frames(frames[..., :3], 4)
    bad_frames(frames.astype(np.float32), 4)
    bad_frames(frames, 4, tile_size=-1)
    bad_frames(frames, 4, alpha_threshold=300)
    bad_frames(frames, 4, alpha_threshold=1.5)
    bad_frames(frames, 4, dither="riemersma")
    bad_frames(frames, 4, dither="ordered", spread=-0.5)
    bad_frames(frames, 4, tile_size=0, weights=np.ones(39))        # F*H*W = 40 values
