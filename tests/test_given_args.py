"""What remap, frame_deltas and measure say to unusable arguments, pinned whole: (exit code, patolette_amd_last_error()).

The three entries reject their arguments before an engine is initialised, so every row runs without a GPU.  Shapes are the
smallest: 2 frames of 4x4, a 16-row palette.  A row names the arguments it changes from a valid call; `None` for the text means
that the call records nothing (validate()'s -2 / -4: last_error stays what the previous call left).
frame_deltas_rgba, remap_rgba and gif_lzw follow with tables of the same form, one row per test their entries make, in the entries'
order; rows that are wrong in two ways pin that order.
"""
import ctypes as C

import numpy as np
import pytest

F, W, H, K = 2, 4, 4, 16
BIG = 40000                                                  # BIG x BIG pixels is validate()'s cap

PIX = np.zeros((F, H, W, 3), dtype=np.uint8)
PAL8 = (np.arange(3 * K, dtype=np.uint8) * 5).reshape(K, 3)
PALF = np.asfortranarray(PAL8 / 255.0)                       # planar (K,3) f64, as the ABI takes it
MAPS = {eb: np.zeros(F * H * W, dtype="u%d" % eb) for eb in (1, 2, 4, 8)}
OUT = np.zeros(3 * F * H * W * 8, dtype=np.uint8)            # any output of any entry fits


def _pal(fill_from=K, poke=None):
    p = PALF.copy(order="F")
    p[fill_from:] = -1.0
    if poke:
        p[poke[0], poke[1]] = poke[2]
    return p


def _ptr(a, typ=C.c_void_p):
    return None if a is None else a.ctypes.data_as(typ)


def _remap(native, flavour, mode, a):
    L, code = native.lib(), C.c_int(99)
    name = {"nearest": "remap_u8", "dither": "remap_u8", "ordered": "remap_ordered_u8"}[mode]
    arg = a["spread"] if mode == "ordered" else int(mode == "dither")
    getattr(L, "patolette_amd_" + name + flavour)(
        a["frames"], a["width"], a["height"], _ptr(a["pixels"]), a["channels"], _ptr(a["palette"], native.dp), _ptr(a["palette_u8"]),
        a["rows"], arg, _ptr(a["map"]), a["eb"], _ptr(a["quant"]), C.byref(code))
    return code.value


def _deltas(native, flavour, a):
    L, code = native.lib(), C.c_int(99)
    getattr(L, "patolette_amd_frame_deltas" + flavour)(
        a["frames"], a["width"], a["height"], _ptr(a["maps"]), a["eb"], a["rows"], a["T"], _ptr(a["pixels"]), a["channels"],
        _ptr(a["palette"], native.dp), _ptr(a["palette_u8"]), a["tolerance"], _ptr(OUT), _ptr(OUT), None, None, C.byref(code))
    return code.value


def _measure(native, flavour, a):
    L, code = native.lib(), C.c_int(99)
    cnt = np.zeros(K + F, dtype=np.uint64)
    getattr(L, "patolette_amd_measure" + flavour)(
        a["frames"], a["width"], a["height"], _ptr(a["pixels"]), a["channels"], _ptr(a["maps"]), a["eb"], _ptr(a["palette"], native.dp),
        _ptr(a["palette_u8"]), a["rows"], a["skip"], _ptr(cnt, C.POINTER(C.c_uint64)), None, None, None, None, None, None, None,
        C.byref(code))
    return code.value


NO_DEVICE = "patolette_amd: no HIP device available (this library has no CPU fallback)"

# the palette parse, the same for the three entries save the name (frame_deltas: with a tolerance above 0 only)
def _palette_rows(name):
    return [
        (dict(palette=_pal(0), palette_u8=None), -1, name + ": every palette row is the unused-row fill (-1, -1, -1)"),
        (dict(palette=_pal(poke=(3, 1, np.nan)), palette_u8=None), -1, name + ": the palette holds a value that is not finite"),
        (dict(palette=_pal(poke=(0, 2, np.inf)), palette_u8=None), -1, name + ": the palette holds a value that is not finite"),
        (dict(palette=_pal(12, poke=(11, 0, -np.inf)), palette_u8=None), -1, name + ": the palette holds a value that is not finite"),
    ]


REMAP_VALID = dict(frames=F, width=W, height=H, pixels=PIX, channels=3, palette=None, palette_u8=PAL8, rows=K, spread=0.25,
                   map=OUT, eb=1, quant=OUT)
R = "patolette_amd_remap"
REMAP_BAD_U8 = R + ": bad channels / map_elem_bytes (1, 2, 4 or 8, able to hold palette_rows - 1)"
REMAP_ONE_OF = R + ": pass exactly one of palette and palette_u8"
REMAP_ROWS = [      # (changed arguments, code, text); the cap's two texts go by mode, below
    (dict(frames=0), -2, None),
    (dict(width=0), -2, None),
    (dict(height=0), -2, None),
    (dict(width=BIG + 1, height=BIG), -4, None),
    (dict(palette_u8=None), -1, REMAP_ONE_OF),
    (dict(palette=_pal()), -1, REMAP_ONE_OF),
    (dict(rows=0), -1, R + ": the palette needs at least one row"),
    (dict(rows=(1 << 31) + 1), -1, R + ": the palette needs at least one row"),
    (dict(channels=2), -1, REMAP_BAD_U8),
    (dict(channels=5), -1, REMAP_BAD_U8),
    (dict(eb=3), -1, REMAP_BAD_U8),
    (dict(eb=0), -1, REMAP_BAD_U8),
    (dict(eb=1, rows=257), -1, REMAP_BAD_U8),
    (dict(eb=2, rows=65537), -1, REMAP_BAD_U8),
    (dict(pixels=None), -1, R + ": no pixels"),
] + _palette_rows(R)
REMAP_CAP = {"nearest": (dict(frames=2, width=BIG, height=BIG), R + ": frames * width * height is too big"),
             "ordered": (dict(frames=2, width=BIG, height=BIG), R + ": frames * width * height is too big"),
             "dither": (dict(frames=3, width=1 << 15, height=1 << 15),
                        R + ": frames * width * height exceeds 2^31 pixels (the dither numbers pixels with 32 bits)")}
REMAP_SPREAD = [(dict(spread=s), -1, R + ": spread must be finite and not negative") for s in (np.nan, np.inf, -0.5)]

D = "patolette_amd_frame_deltas"
DELTAS_VALID = dict(frames=F, width=W, height=H, maps=MAPS[1], eb=1, rows=K, T=255, pixels=PIX, channels=3, palette=None,
                    palette_u8=PAL8, tolerance=0.0)
D_EB = D + ": map_elem_bytes must be 1, 2, 4 or 8 (device maps: 1 or 4)"
D_FIT = D + (": transparent_index does not fit an element of map_elem_bytes: no index is free for it -- make the palette with one row "
             "less, or pass wider elements")
D_ONE_OF = D + ": a tolerance above 0 needs exactly one of palette and palette_u8"
LOSSY = dict(tolerance=0.01)
DELTAS_ROWS = [
    (dict(frames=0), -2, None),
    (dict(width=0), -2, None),
    (dict(width=BIG + 1, height=BIG), -4, None),
    (dict(frames=2, width=BIG, height=BIG), -4, D + ": frames * width * height is too big"),
    (dict(eb=3), -1, D_EB),
    (dict(eb=0), -1, D_EB),
    (dict(eb=16), -1, D_EB),
    (dict(maps=None), -1, D + ": no maps"),
    (dict(rows=0), -1, D + ": palette_rows must lie in [1, 2^31]"),
    (dict(rows=(1 << 31) + 1, T=1 << 40, eb=4), -1, D + ": palette_rows must lie in [1, 2^31]"),
    (dict(T=K - 1), -1, D + ": transparent_index must be at least palette_rows (an index no entry uses)"),
    (dict(T=0), -1, D + ": transparent_index must be at least palette_rows (an index no entry uses)"),
    (dict(T=256), -1, D_FIT),
    (dict(T=1 << 32, eb=4, maps=MAPS[4]), -1, D_FIT),
    (dict(tolerance=np.nan), -1, D + ": tolerance must be finite and not negative"),
    (dict(tolerance=np.inf), -1, D + ": tolerance must be finite and not negative"),
    (dict(tolerance=-1.0), -1, D + ": tolerance must be finite and not negative"),
    (dict(LOSSY, channels=5), -1, D + ": channels must be 3 or 4"),
    (dict(LOSSY, pixels=None), -1, D + ": a tolerance above 0 needs the frames' pixels"),
    (dict(LOSSY, palette_u8=None), -1, D_ONE_OF),
    (dict(LOSSY, palette=_pal()), -1, D_ONE_OF),
] + [(dict(LOSSY, **ch), code, text) for ch, code, text in _palette_rows(D)]
# 2- and 8-byte elements: host maps only
DELTAS_BY_FLAVOUR = {"": [(dict(eb=2, maps=MAPS[2], T=1 << 16), -1, D_FIT)],
                     "_device": [(dict(eb=2, maps=MAPS[2]), -1, D_EB), (dict(eb=8, maps=MAPS[8]), -1, D_EB)]}

M = "patolette_amd_measure"
MEASURE_VALID = dict(frames=F, width=W, height=H, pixels=PIX, channels=3, maps=MAPS[1], eb=1, palette=None, palette_u8=PAL8, rows=K,
                     skip=-1)
M_EB = M + ": map_elem_bytes must be 1, 2, 4 or 8 (device maps: 1 or 4)"
M_ONE_OF = M + ": pass exactly one of palette and palette_u8"
MEASURE_ROWS = [
    (dict(frames=0), -2, None),
    (dict(height=0), -2, None),
    (dict(width=BIG + 1, height=BIG), -4, None),
    (dict(frames=2, width=BIG, height=BIG), -4, M + ": frames * width * height is too big"),
    (dict(channels=2), -1, M + ": channels must be 3 or 4"),
    (dict(channels=5), -1, M + ": channels must be 3 or 4"),
    (dict(eb=3), -1, M_EB),
    (dict(eb=0), -1, M_EB),
    (dict(pixels=None), -1, M + ": no pixels"),
    (dict(maps=None), -1, M + ": no maps"),
    (dict(palette_u8=None), -1, M_ONE_OF),
    (dict(palette=_pal()), -1, M_ONE_OF),
    (dict(rows=0), -1, M + ": palette_rows must lie in [1, 2^31]"),
    (dict(rows=(1 << 31) + 1), -1, M + ": palette_rows must lie in [1, 2^31]"),
    (dict(skip=-2), -1, M + ": skip_index must be -1 (none) or an index"),
    (dict(skip=-(1 << 62)), -1, M + ": skip_index must be -1 (none) or an index"),
] + _palette_rows(M)
MEASURE_BY_FLAVOUR = {"": [], "_device": [(dict(eb=2, maps=MAPS[2]), -1, M_EB), (dict(eb=8, maps=MAPS[8]), -1, M_EB)]}

PIX4 = np.full((F, H, W, 4), 255, dtype=np.uint8)            # RGBA, every pixel opaque


def _deltas_rgba(native, flavour, a):
    L, code = native.lib(), C.c_int(99)
    getattr(L, "patolette_amd_frame_deltas_rgba" + flavour)(
        a["frames"], a["width"], a["height"], _ptr(a["maps"]), a["eb"], a["rows"], _ptr(a["pixels"]), a["channels"],
        _ptr(a["palette"], native.dp), _ptr(a["palette_u8"]), a["tolerance"], a["loop"], _ptr(OUT), _ptr(OUT), None, None, None,
        C.byref(code))
    return code.value


def _remap_rgba(native, flavour, a):
    L, code = native.lib(), C.c_int(99)
    getattr(L, "patolette_amd_remap_rgba_u8" + flavour)(
        a["frames"], a["width"], a["height"], _ptr(a["pixels"]), a["thr"], _ptr(a["palette"], native.dp), _ptr(a["palette_u8"]), a["rows"],
        a["tindex"], a["mode"], a["spread"], _ptr(a["map"]), a["eb"], _ptr(a["quant"]), C.byref(code))
    return code.value


def _gif_lzw(native, flavour, a):
    L, code = native.lib(), C.c_int(99)
    rects = None if a["rects"] is None else np.ascontiguousarray(a["rects"], dtype=np.int32)
    getattr(L, "patolette_amd_gif_lzw" + flavour)(
        a["frames"], a["width"], a["height"], _ptr(a["maps"]), _ptr(rects, C.POINTER(C.c_int32)), a["mcs"], a["segment"], _ptr(a["out"]),
        a["capacity"], _ptr(a["offsets"], C.POINTER(C.c_uint64)), C.byref(code))
    return code.value


DR = "patolette_amd_frame_deltas_rgba"
DELTAS_RGBA_VALID = dict(frames=F, width=W, height=H, maps=MAPS[1], eb=1, rows=K, pixels=PIX, channels=3, palette=None, palette_u8=PAL8,
                         tolerance=0.0, loop=0)
DR_EB = DR + ": map_elem_bytes must be 1, 2, 4 or 8 (device maps: 1 or 4)"
DR_ONE_OF = DR + ": a tolerance above 0 needs exactly one of palette and palette_u8"
DR_TOL = DR + ": tolerance must be finite and not negative"
DR_NOT_FINITE = DR + ": the palette holds a value that is not finite"
DELTAS_RGBA_ROWS = [
    (dict(frames=0), -2, None),
    (dict(width=0), -2, None),
    (dict(height=0), -2, None),
    (dict(width=BIG + 1, height=BIG), -4, None),
    (dict(frames=2, width=BIG, height=BIG), -4, DR + ": frames * width * height is too big"),
    (dict(eb=3), -1, DR_EB),
    (dict(eb=0), -1, DR_EB),
    (dict(eb=16), -1, DR_EB),
    (dict(maps=None), -1, DR + ": no maps"),
    (dict(rows=0), -1, DR + ": palette_rows must lie in [1, 2^31]"),
    (dict(rows=(1 << 31) + 1, eb=4), -1, DR + ": palette_rows must lie in [1, 2^31]"),
    (dict(tolerance=np.nan), -1, DR_TOL),
    (dict(tolerance=np.inf), -1, DR_TOL),
    (dict(tolerance=-1.0), -1, DR_TOL),
    (dict(loop=2), -1, DR + ": loop must be 0 or 1"),
    (dict(loop=-1), -1, DR + ": loop must be 0 or 1"),
    (dict(LOSSY, channels=2), -1, DR + ": channels must be 3 or 4"),
    (dict(LOSSY, channels=5), -1, DR + ": channels must be 3 or 4"),
    (dict(LOSSY, pixels=None), -1, DR + ": a tolerance above 0 needs the frames' pixels"),
    (dict(LOSSY, palette_u8=None), -1, DR_ONE_OF),
    (dict(LOSSY, palette=_pal()), -1, DR_ONE_OF),
    # the palette parse; row 0 is the transparent entry, zeroed before the parse, so an f64 palette always keeps a row
    (dict(LOSSY, palette=_pal(poke=(3, 1, np.nan)), palette_u8=None), -1, DR_NOT_FINITE),
    (dict(LOSSY, palette=_pal(12, poke=(11, 0, -np.inf)), palette_u8=None), -1, DR_NOT_FINITE),
    # wrong in two ways: the first test in the entry's order speaks
    (dict(eb=3, maps=None), -1, DR_EB),
    (dict(maps=None, rows=0), -1, DR + ": no maps"),
    (dict(rows=0, tolerance=np.nan), -1, DR + ": palette_rows must lie in [1, 2^31]"),
    (dict(tolerance=np.nan, loop=2), -1, DR_TOL),
    (dict(LOSSY, loop=2, channels=5), -1, DR + ": loop must be 0 or 1"),
    (dict(LOSSY, channels=5, pixels=None, palette_u8=None), -1, DR + ": channels must be 3 or 4"),
    (dict(LOSSY, pixels=None, palette_u8=None), -1, DR + ": a tolerance above 0 needs the frames' pixels"),
    # the exact mode reads neither pixels nor palette: nothing about them is tested (the row count still is)
    (dict(channels=5, pixels=None, palette_u8=None, rows=0), -1, DR + ": palette_rows must lie in [1, 2^31]"),
]
DELTAS_RGBA_BY_FLAVOUR = {"": [], "_device": [(dict(eb=2, maps=MAPS[2]), -1, DR_EB), (dict(eb=8, maps=MAPS[8]), -1, DR_EB)]}

RR = "patolette_amd_remap_rgba"
REMAP_RGBA_VALID = dict(frames=F, width=W, height=H, pixels=PIX4, thr=128, palette=None, palette_u8=PAL8, rows=K, tindex=0, mode=0,
                        spread=0.25, map=OUT, eb=1, quant=OUT)
RR_BAD_EB = RR + ": bad map_elem_bytes (1, 2, 4 or 8, able to hold palette_rows - 1)"
RR_ONE_OF = RR + ": pass exactly one of palette and palette_u8"
RR_THR = RR + ": alpha_threshold must lie in [0, 256]"
RR_TINDEX = RR + ": transparent_index must be -1 (none) or 0 (row 0)"
RR_NO_OPAQUE = RR + ": no opaque palette row remains beside the transparent entry"
REMAP_RGBA_ROWS = [     # the cap's two texts, the mode's and the spread's go by mode, below
    (dict(frames=0), -2, None),
    (dict(width=0), -2, None),
    (dict(height=0), -2, None),
    (dict(width=BIG + 1, height=BIG), -4, None),
    (dict(thr=-1), -1, RR_THR),
    (dict(thr=257), -1, RR_THR),
    (dict(tindex=1), -1, RR_TINDEX),
    (dict(tindex=-2), -1, RR_TINDEX),
    (dict(palette_u8=None), -1, RR_ONE_OF),
    (dict(palette=_pal()), -1, RR_ONE_OF),
    (dict(rows=0), -1, RR + ": the palette needs at least one row"),
    (dict(rows=(1 << 31) + 1), -1, RR + ": the palette needs at least one row"),
    (dict(eb=3), -1, RR_BAD_EB),
    (dict(eb=0), -1, RR_BAD_EB),
    (dict(eb=1, rows=257), -1, RR_BAD_EB),
    (dict(eb=2, rows=65537), -1, RR_BAD_EB),
    (dict(pixels=None), -1, RR + ": no pixels"),
] + _palette_rows(RR) + [
    (dict(rows=1), -1, RR_NO_OPAQUE),
    (dict(palette=_pal(1), palette_u8=None), -1, RR_NO_OPAQUE),
    # wrong in two ways: the first test in the entry's order speaks
    (dict(thr=-1, tindex=1), -1, RR_THR),
    (dict(tindex=1, palette_u8=None), -1, RR_TINDEX),
    (dict(palette_u8=None, rows=0), -1, RR_ONE_OF),
    (dict(rows=0, eb=3), -1, RR + ": the palette needs at least one row"),
    (dict(eb=3, pixels=None), -1, RR_BAD_EB),
    (dict(pixels=None, palette=_pal(0), palette_u8=None), -1, RR + ": no pixels"),
]
REMAP_RGBA_CAP = {0: (dict(frames=2, width=BIG, height=BIG), RR + ": frames * width * height is too big"),
                  2: (dict(frames=2, width=BIG, height=BIG), RR + ": frames * width * height is too big"),
                  1: (dict(frames=3, width=1 << 15, height=1 << 15),
                      RR + ": frames * width * height exceeds 2^31 pixels (the dither numbers pixels with 32 bits)")}
RR_MODE = RR + ": mode must be 0 (nearest), 1 (Riemersma) or 2 (ordered)"
REMAP_RGBA_MODE = [(dict(mode=3), -1, RR_MODE), (dict(mode=-1), -1, RR_MODE), (dict(mode=3, thr=-1), -1, RR_MODE),
                   (dict(mode=3, frames=2, width=BIG, height=BIG), -4, RR + ": frames * width * height is too big")]
REMAP_RGBA_SPREAD = [(dict(spread=s), -1, RR + ": spread must be finite and not negative") for s in (np.nan, np.inf, -0.5)] + \
                    [(dict(spread=np.nan, rows=1), -1, RR_NO_OPAQUE)]

G = "patolette_amd_gif_lzw"
GIF_VALID = dict(frames=F, width=W, height=H, maps=MAPS[1], rects=None, mcs=4, segment=0, out=OUT, capacity=OUT.size,
                 offsets=np.zeros(F + 1, dtype=np.uint64))
G_RECT = G + ": every rectangle must lie inside the frame and have w, h >= 1"
G_MCS = G + ": min_code_size must lie in [2, 8]"
G_SEG = G + ": segment must be 0 (the default) or lie in [1, 2^24]"
FULL = [0, 0, W, H]
GIF_ROWS = [
    (dict(frames=0), -2, None),
    (dict(width=0), -2, None),
    (dict(height=0), -2, None),
    (dict(width=BIG + 1, height=BIG), -4, None),
    (dict(frames=2, width=BIG, height=BIG), -4, G + ": frames * width * height is too big"),
    (dict(maps=None), -1, G + ": no maps"),
    (dict(offsets=None), -1, G + ": no offsets"),
    (dict(out=None, capacity=1), -1, G + ": no out"),
    (dict(mcs=1), -1, G_MCS),
    (dict(mcs=9), -1, G_MCS),
    (dict(segment=(1 << 24) + 1), -1, G_SEG),
    (dict(rects=[FULL, [0, 0, 0, H]]), -1, G_RECT),                  # w = 0
    (dict(rects=[FULL, [0, 0, W, 0]]), -1, G_RECT),                  # h = 0
    (dict(rects=[FULL, [1, 0, W, H]]), -1, G_RECT),                  # x0 + w > width
    (dict(rects=[FULL, [0, 2, W, H - 1]]), -1, G_RECT),              # y0 + h > height
    (dict(rects=[FULL, [-1, 0, 2, 2]]), -1, G_RECT),                 # a negative x0
    (dict(rects=[FULL, [0, -1, 2, 2]]), -1, G_RECT),
    (dict(rects=[[0, 0, W + 1, H], FULL]), -1, G_RECT),              # the first frame's
    # wrong in two ways: the first test in the entry's order speaks
    (dict(maps=None, offsets=None), -1, G + ": no maps"),
    (dict(offsets=None, out=None, capacity=1), -1, G + ": no offsets"),
    (dict(out=None, capacity=1, mcs=1), -1, G + ": no out"),
    (dict(mcs=9, segment=(1 << 24) + 1), -1, G_MCS),
    (dict(segment=(1 << 24) + 1, rects=[FULL, [0, 0, 0, H]]), -1, G_SEG),
]


def _sentinel(native):
    """Leaves a known text in last_error: measure's skip_index complaint (a fail_args site like any other)."""
    assert _measure(native, "", dict(MEASURE_VALID, skip=-2)) == -1
    return native.last_error()


def _check(native, flavour, call, valid, rows):
    """Every row: the exit code and last_error whole.  A row that records nothing leaves what the call before it recorded."""
    no_device = native.lib().patolette_amd_device_count() <= 0
    seen = 0
    for changes, code, text in rows:
        before = _sentinel(native)
        got = call(dict(valid, **changes))
        assert (got, native.last_error()) == (code, before if text is None else text), changes
        seen += 1
    # a valid call: refused for want of a device and nothing worse.  Where there is one it runs (the host flavour: these are host arrays)
    if no_device or flavour == "":
        got = call(dict(valid))
        assert (got, native.last_error()) == (-1, NO_DEVICE) if no_device else got == 0, native.last_error()
    return seen


@pytest.mark.parametrize("flavour", ["", "_device"])
@pytest.mark.parametrize("mode", ["nearest", "dither", "ordered"])
def test_remap_argument_messages(native, flavour, mode):
    cap = [(REMAP_CAP[mode][0], -4, REMAP_CAP[mode][1])]
    rows = REMAP_ROWS + cap + (REMAP_SPREAD if mode == "ordered" else [])
    assert _check(native, flavour, lambda a: _remap(native, flavour, mode, a), REMAP_VALID, rows) == len(rows)


@pytest.mark.parametrize("flavour", ["", "_device"])
def test_frame_deltas_argument_messages(native, flavour):
    rows = DELTAS_ROWS + DELTAS_BY_FLAVOUR[flavour]
    assert _check(native, flavour, lambda a: _deltas(native, flavour, a), DELTAS_VALID, rows) == len(rows)


@pytest.mark.parametrize("flavour", ["", "_device"])
def test_measure_argument_messages(native, flavour):
    rows = MEASURE_ROWS + MEASURE_BY_FLAVOUR[flavour]
    assert _check(native, flavour, lambda a: _measure(native, flavour, a), MEASURE_VALID, rows) == len(rows)


@pytest.mark.parametrize("flavour", ["", "_device"])
def test_frame_deltas_rgba_argument_messages(native, flavour):
    rows = DELTAS_RGBA_ROWS + DELTAS_RGBA_BY_FLAVOUR[flavour]
    assert _check(native, flavour, lambda a: _deltas_rgba(native, flavour, a), DELTAS_RGBA_VALID, rows) == len(rows)


@pytest.mark.parametrize("flavour", ["", "_device"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_remap_rgba_argument_messages(native, flavour, mode):
    cap = [(REMAP_RGBA_CAP[mode][0], -4, REMAP_RGBA_CAP[mode][1])]
    rows = REMAP_RGBA_ROWS + cap + REMAP_RGBA_MODE + (REMAP_RGBA_SPREAD if mode == 2 else [])
    valid = dict(REMAP_RGBA_VALID, mode=mode)
    assert _check(native, flavour, lambda a: _remap_rgba(native, flavour, a), valid, rows) == len(rows)


@pytest.mark.parametrize("flavour", ["", "_device"])
def test_gif_lzw_argument_messages(native, flavour):
    assert _check(native, flavour, lambda a: _gif_lzw(native, flavour, a), GIF_VALID, GIF_ROWS) == len(GIF_ROWS)
