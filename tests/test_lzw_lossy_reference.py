"""tests/lzw_lossy_ref.py against itself and against the independent decoder of tests/lzw_ref.py, `gif_neighbours` through the library
against the numpy reference, and the argument checks of gif_lzw_lossy / gif_neighbours / write_gif(near=...) that come before any
library call (no GPU).

The consequences of the rule as include/patolette_amd.h letters them: (a) the stream decodes to `coded`; (b) it is the exact coder's
stream of `coded`; (c) every coded element is the map's or one of its row's candidates; (e) an empty table gives the exact coder's
bytes; (f) the first symbol of every segment is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import patolette_amd
from patolette_amd import _native
from tests import lzw_lossy_ref, lzw_ref

LENGTHS = list(range(1, 140))
SEGMENTS = [7, 50, 64, 350, 8192]                                   # those of tests/test_lzw_reference.py
MS = [2, 3, 5, 8]
TABLES = {"empty": lambda m: lzw_lossy_ref.empty_table(), "pairing": lzw_lossy_ref.pairing_table, "dense": lzw_lossy_ref.dense_table}


def _allowed(x, coded, near):
    """(c): every coded element is the symbol or one of its row's candidates."""
    for s, c in zip(np.asarray(x).tolist(), np.asarray(coded).tolist()):
        if c != s and c not in near[s, 1:1 + near[s, 0]].tolist():
            return False
    return True


def test_decode_inverts_encode_and_the_consequences():
    changed = {name: 0 for name in TABLES}
    for m in MS:
        for name, make in TABLES.items():
            near = make(m)
            for n in LENGTHS:
                x = lzw_ref.contents("noise", n, m)
                for segment in SEGMENTS:
                    if segment != 8192 and n > 3 * segment:
                        continue
                    stream, coded = lzw_lossy_ref.encode_lossy(x, m, near, segment)
                    assert coded.shape == x.shape
                    assert lzw_ref.decode(stream, m, n) == coded.tolist(), (m, name, n, segment)                 # (a)
                    assert stream == lzw_ref.encode(coded, m, segment), (m, name, n, segment)                    # (b)
                    assert _allowed(x, coded, near), (m, name, n, segment)                                       # (c)
                    assert np.array_equal(coded[::segment], x[::segment]), (m, name, n, segment)                 # (f)
                    assert len(stream) <= lzw_ref.bound(n, segment)
                    if name == "empty":
                        assert stream == lzw_ref.encode(x, m, segment) and np.array_equal(coded, x)              # (e)
                    changed[name] += int(np.sum(coded != x))
    assert changed["empty"] == 0 and changed["pairing"] > 0 and changed["dense"] > changed["pairing"]


def _pack(codes):
    """(code, width) pairs, first code lowest, the last byte padded with zero bits."""
    acc, at = 0, 0
    for code, width in codes:
        assert 0 <= code < 1 << width
        acc |= code << at
        at += width
    return acc.to_bytes((at + 7) // 8, "little")


# Hand-written cases: (m, symbols, near rows {s: candidates}, the codes with their widths, coded).
# m = 2: Clear 4, end 5, the first entry is 6 at 3 bits; entering code 8 = 2^3 makes the width 4.
# m = 4: Clear 16, end 17, the first entry is 18, all at 5 bits here.
HAND = {
    # 3 2 3 0 enter (3,2) = 6, (2,3) = 7, (3,0) = 8 (width 4), then 3 is the prefix and (0,3) = 9 is entered.  The last 2: (3,2) = 6 and
    # its candidate's (3,0) = 8 are both in the dictionary; the exact pair wins, and the pending prefix is 6, not 8.
    "exact beats neighbour": (2, [3, 2, 3, 0, 3, 2], {2: [0]}, [(4, 3), (3, 3), (2, 3), (3, 3), (0, 4), (6, 4), (5, 4)], [3, 2, 3, 0, 3, 2]),
    # 3 0 3 1 enter (3,0) = 6, (0,3) = 7, (3,1) = 8 (width 4), (1,3) = 9.  The last 2: (3,2) is not there; of its candidates 1 and 0,
    # both of which are, the first one listed wins: 8 with the row (1, 0), 6 with the row (0, 1).
    "an earlier neighbour beats a later one": (2, [3, 0, 3, 1, 3, 2], {2: [1, 0]}, [(4, 3), (3, 3), (0, 3), (3, 3), (1, 4), (8, 4), (5, 4)],
                                               [3, 0, 3, 1, 3, 1]),
    "... in the other order": (2, [3, 0, 3, 1, 3, 2], {2: [0, 1]}, [(4, 3), (3, 3), (0, 3), (3, 3), (1, 4), (6, 4), (5, 4)], [3, 0, 3, 1, 3, 0]),
    # 1 0 1 enter (1,0) = 18 and (0,1) = 19.  The 15: (1,15) is not there, nor is (1,c) for the 14 candidates 2 .. 15; the 15th, 0, is.
    "the 15th candidate is found": (4, [1, 0, 1, 15], {15: list(range(2, 16)) + [0]}, [(16, 5), (1, 5), (0, 5), (18, 5), (17, 5)], [1, 0, 1, 0]),
    # the same row with the count 0 (set below): its bytes are not read, the 15 is a plain miss
    "a count-0 row": (4, [1, 0, 1, 15], {15: []}, [(16, 5), (1, 5), (0, 5), (1, 5), (15, 5), (17, 5)], [1, 0, 1, 15]),
}


def hand_table(name):
    m, _, rows, _, _ = HAND[name]
    near = lzw_lossy_ref.empty_table()
    for s, cands in rows.items():
        near[s, 0] = len(cands)
        near[s, 1:1 + len(cands)] = cands
    if name == "a count-0 row":
        near[15, 1:] = 0                                             # symbol 0 would match if the row were read
        near[15, 1] = 0
    return near


@pytest.mark.parametrize("name", list(HAND))
def test_hand_written_cases(name):
    m, x, _, want_codes, want_coded = HAND[name]
    codes = []
    stream, coded = lzw_lossy_ref.encode_lossy(x, m, hand_table(name), codes=codes)
    assert codes == want_codes
    assert stream == _pack(want_codes)
    assert coded.tolist() == want_coded
    assert lzw_ref.decode(stream, m, len(x)) == want_coded


def test_the_full_dictionary_with_a_table():
    """9216 symbols of noise at m = 8 in one segment under the pairing table: the dictionary fills, and the Clear that is no segment
    boundary comes at 12 bits."""
    x = lzw_ref.contents("noise", 96 * 96, 8)
    near = lzw_lossy_ref.pairing_table(8)
    codes = []
    stream, coded = lzw_lossy_ref.encode_lossy(x, 8, near, 65536, codes)
    clears = [i for i, (c, w) in enumerate(codes) if c == 256]
    assert clears[0] == 0 and len(clears) - 1 >= 1 and all(codes[i][1] == 12 for i in clears[1:])
    assert lzw_ref.decode(stream, 8, x.size) == coded.tolist()
    assert stream == lzw_ref.encode(coded, 8, 65536)
    assert _allowed(x, coded, near) and np.any(coded != x)
    assert len(stream) <= lzw_ref.bound(x.size, 65536)


# ----------------------------------------------------------------------------------------------------------------------
# gif_neighbours
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pal(rows, kind, trailing=0, seed=0):
    """Random rows; "dup": every third row repeats an earlier one; f64 palettes may end in `trailing` unused (-1, -1, -1) rows."""
    rng = np.random.default_rng(100 * rows + seed)
    p8 = rng.integers(0, 256, size=(rows, 3)).astype(np.uint8)
    if "dup" in kind:
        for i in range(2, rows, 3):
            p8[i] = p8[rng.integers(0, i)]
    if kind.startswith("u8"):
        pal = p8
    else:
        pal = np.concatenate([(p8.astype(np.float64) + rng.random((rows, 3)) * 0.5) / 255.5, np.full((trailing, 3), -1.0)])
        if "dup" in kind:
            for i in range(2, rows, 3):
                pal[i] = pal[int(np.flatnonzero((p8[:i] == p8[i]).all(axis=1))[0])]
    pal.setflags(write=False)
    return pal


NEIGHBOUR_CASES = [(rows, kind, trailing) for rows in (1, 2, 5, 16, 17, 255, 256) for kind, trailing in (("u8", 0), ("f64", 0), ("u8 dup", 0), ("f64 dup", 0))]
NEIGHBOUR_CASES += [(5, "f64", 3), (17, "f64 dup", 1), (250, "f64", 6)]


@pytest.mark.parametrize("rows,kind,trailing", NEIGHBOUR_CASES)
def test_gif_neighbours_equals_the_reference(native, ob, rows, kind, trailing):
    pal = _pal(rows, kind, trailing)
    seen = {"most": 0, "dup": 0}
    # 0.6: more than 15 rows within reach of the larger palettes.  Two identical rows lie equally far from any third one, an order the
    # rule below calls undecided: palettes with duplicates are taken at tolerances that reach the duplicates alone
    for tolerance in ((0.0, 0.0002) if "dup" in kind else (0.0, 0.03, 0.1, 0.6)):
        for transparent in (None, 0, rows - 1, rows // 2, 255):
            for most in (0, 1, 15):
                if most != 15 and transparent not in (None, 0):
                    continue
                undecided = []
                want = lzw_lossy_ref.neighbours(pal, tolerance, transparent, most, undecided)
                assert undecided == [], undecided                   # the palettes are such that numpy and the library cannot differ
                ok, got, msg = patolette_amd.gif_neighbours(pal, tolerance, transparent, most)
                assert ok and got.shape == (256, 16) and got.dtype == np.uint8, msg
                assert np.array_equal(got, want), (tolerance, transparent, most, np.argwhere(got != want)[:4].tolist())
                assert np.all(got[rows:] == 0) and np.all(got[:, 0] <= most)
                if transparent is not None and transparent < rows:   # excluded both ways
                    assert got[transparent, 0] == 0
                    assert not any(transparent in got[s, 1:1 + got[s, 0]].tolist() for s in range(rows))
                seen["most"] = max(seen["most"], int(np.sum(lzw_lossy_ref.distances(pal) <= tolerance * tolerance, axis=1).max()) - 1)
                if tolerance == 0.0 and most == 15 and transparent is None:
                    D = lzw_lossy_ref.distances(pal)
                    same = (D == 0.0) & ~np.eye(D.shape[0], dtype=bool)
                    seen["dup"] += int(same.sum())
                    for s in range(D.shape[0]):                      # identical rows only, by index
                        assert got[s, 1:1 + got[s, 0]].tolist() == np.flatnonzero(same[s])[:15].tolist()
    if rows >= 17 and "dup" not in kind:
        assert seen["most"] > 15
    if "dup" in kind and rows >= 5:
        assert seen["dup"] > 0


def test_gif_neighbours_failures(native):
    L = native.lib()
    near = np.zeros((256, 16), dtype=np.uint8)
    p8 = np.ascontiguousarray(_pal(16, "u8"))
    pf = np.asfortranarray(_pal(16, "f64"))

    def call(palette=None, palette_u8=p8, rows=16, transparent=-1, tolerance=0.1, most=15, out=near):
        code = C.c_int(7)
        L.patolette_amd_gif_neighbours(None if palette is None else palette.ctypes.data_as(C.POINTER(C.c_double)),
                                       None if palette_u8 is None else palette_u8.ctypes.data_as(C.c_void_p), rows, transparent, tolerance, most,
                                       None if out is None else out.ctypes.data_as(C.c_void_p), C.byref(code))
        return code.value

    def failed(code, *words):
        text = _native.last_error()
        assert code == -1 and text.startswith("patolette_amd_gif_neighbours:") and all(w in text for w in words), (code, text)

    assert call() == 0
    assert call(palette=pf, palette_u8=None) == 0
    failed(call(palette=pf), "exactly one")
    failed(call(palette_u8=None), "exactly one")
    failed(call(rows=0), "palette_rows")
    failed(call(rows=257), "palette_rows")
    failed(call(transparent=-2), "transparent_index")
    failed(call(transparent=256), "transparent_index")
    for t in (-0.1, float("nan"), float("inf")):
        failed(call(tolerance=t), "tolerance")
    failed(call(most=-1), "max_neighbours")
    failed(call(most=16), "max_neighbours")
    failed(call(out=None), "near_out")
    bad = pf.copy(order="F")
    bad[3, 1] = float("nan")
    failed(call(palette=bad, palette_u8=None), "not finite")
    fill = np.asfortranarray(np.full((4, 3), -1.0))
    failed(call(palette=fill, palette_u8=None, rows=4), "unused-row fill")
    assert call() == 0


# ----------------------------------------------------------------------------------------------------------------------
# the Python surface
# ----------------------------------------------------------------------------------------------------------------------
def test_value_errors_come_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "lib", no_library)
    maps = np.zeros((2, 5, 7), dtype=np.uint8)
    pal = np.zeros((16, 3), dtype=np.uint8)
    near = lzw_lossy_ref.pairing_table(8)
    count16, cand16, cand_m4 = near.copy(), near.copy(), lzw_lossy_ref.pairing_table(4)
    count16[200, 0] = 16
    cand16[3, 0], cand16[3, 2] = 2, 16                              # readable at m = 4 only as far as the count says
    cand_m4[9, 0], cand_m4[9, 5] = 5, 16
    bad_lossy = [
        dict(maps=maps.astype(np.uint16)), dict(maps=np.zeros(5, dtype=np.uint8)), dict(maps=[[1, 2]]),
        dict(rects=np.zeros((3, 4), dtype=np.int32)), dict(rects=[[0, 0, 8, 5], [0, 0, 7, 5]]), dict(rects=[[0, 0, 0, 3], [0, 0, 7, 5]]),
        dict(min_code_size=1), dict(min_code_size=9), dict(min_code_size=2.0), dict(min_code_size=True),
        dict(segment=0), dict(segment=2 ** 24 + 1), dict(segment=64.0),
        dict(near=None), dict(near=near.astype(np.int32)), dict(near=near[:255]), dict(near=near.reshape(-1)), dict(near=near[:, :15]),
        dict(near=np.zeros((16, 16), dtype=np.uint8), min_code_size=4), dict(near=count16), dict(near=cand16, min_code_size=4),
        dict(near=cand_m4, min_code_size=4), dict(near=lzw_lossy_ref.dense_table(8), min_code_size=7),
    ]
    for kw in bad_lossy:
        args = dict(maps=maps, near=near)
        args.update(kw)
        with pytest.raises(ValueError):
            patolette_amd.gif_lzw_lossy(**args)
    ok_tables = [dict(near=count16, min_code_size=7), dict(near=cand_m4, min_code_size=5)]     # rows and bytes that are not read
    cand16[3, 0] = 1
    ok_tables.append(dict(near=cand16, min_code_size=4))
    for kw in ok_tables + [dict()]:
        args = dict(maps=maps, near=lzw_lossy_ref.empty_table())
        args.update(kw)
        with pytest.raises(AssertionError, match="the library was called"):
            patolette_amd.gif_lzw_lossy(**args)
    bad_neighbours = [
        dict(palette=np.zeros((257, 3), dtype=np.uint8)), dict(palette=np.zeros((16, 4), dtype=np.uint8)), dict(palette=np.zeros((0, 3))),
        dict(palette=np.zeros((16, 3), dtype=np.int32)), dict(palette=np.full((4, 3), np.nan)),
        dict(tolerance=-0.1), dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(tolerance="0.1"), dict(tolerance=None),
        dict(transparent_index=256), dict(transparent_index=-1), dict(transparent_index=1.5), dict(transparent_index=True),
        dict(max_neighbours=16), dict(max_neighbours=-1), dict(max_neighbours=3.0), dict(max_neighbours=True),
    ]
    for kw in bad_neighbours:
        args = dict(palette=pal, tolerance=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            patolette_amd.gif_neighbours(**args)
    with pytest.raises(AssertionError, match="the library was called"):
        patolette_amd.gif_neighbours(pal, 0.1, 255, 3)
    bad_gif = [dict(near=near.astype(np.int32)), dict(near=near[:16]), dict(near=lzw_lossy_ref.dense_table(8)), dict(near=count16, transparent_index=255),
               dict(near=lzw_lossy_ref.empty_table(), segment=0), dict(near=lzw_lossy_ref.empty_table(), maps=maps.astype(np.uint16))]
    for kw in bad_gif:                                               # (16 rows: m = 4, and the dense table of m = 8 names rows beyond it)
        args = dict(file=None, maps=maps, palette_u8=pal)
        args.update(kw)
        with pytest.raises(ValueError):
            patolette_amd.write_gif(**args)
    with pytest.raises(AssertionError, match="the library was called"):
        patolette_amd.write_gif(None, maps, pal, near=lzw_lossy_ref.pairing_table(4))


def test_the_symbols_are_declared_bound_and_exported(native):
    from tests.test_abi import declared_functions
    names = {"patolette_amd_gif_lzw_lossy", "patolette_amd_gif_lzw_lossy_device", "patolette_amd_gif_neighbours"}
    assert names <= declared_functions("patolette_amd.h") and names <= set(native.SYMBOLS)
    L = native.lib()
    assert all(hasattr(L, n) for n in names)
    assert {"gif_lzw_lossy", "gif_neighbours"} <= set(patolette_amd.__all__)
    import inspect
    assert list(inspect.signature(patolette_amd.write_gif).parameters)[-2:] == ["segment", "near"]
    assert inspect.signature(patolette_amd.write_gif).parameters["near"].default is None


# ----------------------------------------------------------------------------------------------------------------------
# what it is for
# ----------------------------------------------------------------------------------------------------------------------
BAYER4 = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], dtype=np.float64)


def dithered_gradient(h=48, w=96, rows=16):
    """A horizontal grey ramp on `rows` evenly spaced greys, ordered-dithered with the 4 x 4 Bayer matrix: (maps (h, w) uint8, palette)."""
    level = np.tile(np.linspace(0.0, rows - 1.0, w), (h, 1))
    threshold = (np.tile(BAYER4, (h // 4, w // 4)) + 0.5) / 16.0
    maps = np.minimum(np.floor(level + threshold), rows - 1).astype(np.uint8)
    pal = np.repeat(np.round(np.linspace(0, 255, rows)).astype(np.uint8)[:, None], 3, axis=1)
    return maps, pal


def test_the_lossy_stream_is_shorter_on_an_ordered_dithered_gradient(ob):
    """16 greys 17 / 255 apart lie 0.008 .. 0.011 from the next one in ICtCp (0.016 between the two darkest) and 0.016 and more from the
    one after it: at tolerance 0.012 every grey from 2 to 14 has exactly its neighbours on either side as candidates (asserted), and the
    Bayer pattern, which breaks the exact coder's matches, no longer does."""
    maps, pal = dithered_gradient()
    near = lzw_lossy_ref.neighbours(pal, 0.012)
    assert np.all(near[2:15, 0] == 2) and all(sorted(near[s, 1:3].tolist()) == [s - 1, s + 1] for s in range(2, 15))
    x = maps.reshape(-1)
    exact = lzw_ref.encode(x, 4)
    stream, coded = lzw_lossy_ref.encode_lossy(x, 4, near)
    assert lzw_ref.decode(stream, 4, x.size) == coded.tolist()
    assert np.max(np.abs(coded.astype(int) - x.astype(int))) <= 1
    print("exact %d bytes, lossy %d bytes, %.1f %% of the entries changed" % (len(exact), len(stream), 100.0 * np.mean(coded != x)))
    assert len(stream) < len(exact)


def test_the_table_rules_hold_under_sanitizers(tmp_path):
    """csrc/lzw_near.h -- the coder's check of a table and the builder -- as a stand-alone program over buffers of exactly the
    documented sizes (tests/lzw_near_check.cpp), in the manner of tests/test_given_host.py."""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lzw_near_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(here, "..", "patolette_amd", "csrc"), os.path.join(here, "lzw_near_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "tables checked" in run.stdout and "follow the rule" in run.stdout
