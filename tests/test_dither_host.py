"""The dither drivers' host arithmetic (csrc/dither_host.h) on the CPU under sanitizers.

dither_host_check.cpp is a stand-alone program over the header alone; this test writes its cases, runs it as a child process and holds
every line to tests/dither_ref.py: the lane layout's three grids and the margins of its f32 first pass bit for bit with lane_geometry
(palettes of 8 .. 256 rows, no extent, extent on one axis, an infinite and a NaN entry, either side of the 2^20 pixels at which the
first grid goes from 32 to 64 cells across), the two cuts of the curve, the layout rule and the stall rule with their restatements
there, and the properties the kernels' comments rely on.
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dither_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "patolette_amd", "csrc")
CUS = 256


def palettes():
    rng = np.random.default_rng(23)
    for k in (8, 9, 64, 65, 128, 129, 256):
        yield "k%d" % k, rng.random((k, 3))
    yield "equal_rows", np.tile(rng.random(3), (16, 1))
    one_axis = np.tile(rng.random(3), (16, 1))
    one_axis[:, 1] = rng.random(16)
    yield "one_axis", one_axis
    for name, bad in (("inf", np.inf), ("minus_inf", -np.inf), ("nan", np.nan), ("nan_first", np.nan)):
        pal = rng.random((16, 3))
        pal[0 if name == "nan_first" else 5, 1] = bad
        yield name, pal


def lane_cut_cases():
    """(segments, warm, cus, npix, nframe, frames)"""
    for npix in (64, 65, 255, 256, 65536):
        for segments, warm in ((0, -1), (1, -1), (npix // 64 + 1, -1), (0, 0), (0, 10 ** 6), (7, 3)):
            yield segments, warm, CUS, npix, npix, 1
    for frames, n in itertools.product((2, 3, 7), (64, 100)):
        for segments, warm in ((0, -1), (1, 0), (frames * n // 64 + 1, -1), (frames * 2 + 1, -1), (0, 10 ** 6)):
            yield segments, warm, CUS, frames * n, n, frames
    yield 0, -1, CUS, 1 << 26, 1 << 26, 1                       # the default cut of 8192^2: 512 runs per CU
    yield 0, -1, CUS, 1 << 31, 1 << 31, 1
    yield 10 ** 6, -1, CUS, 1 << 31, 1 << 31, 1                 # more runs asked for than grid.y has rows of 8
    yield 0, -1, CUS, 3 << 22, 1 << 22, 3
    yield 0, -1, CUS, 600000 * 64, 64, 600000                   # more frames than 8 * 65535: not possible, and must not divide by zero


def wave_cut_cases():
    """(segments, warm, cus, npix, width, height)"""
    for w, h in ((15, 15), (16, 1), (16, 16), (1024, 1024), (96, 80)):
        for segments, warm in ((0, -1), (1, -1), (w * h // 64 + 1, -1), (0, 0), (0, 10 ** 6), (5, 100)):
            yield segments, warm, CUS, w * h, w, h
    yield 0, -1, CUS, 70000, 512, 512                           # a masked image: the opaque count, the whole image's sides


def hexes(words):
    return [float.fromhex(w) for w in words]


def test_dither_host_arithmetic_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "dither_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I", CSRC, os.path.join(HERE, "dither_host_check.cpp"), "-o", exe], check=True)

    geoms = [(name, pal, npix) for name, pal in palettes() for npix in ((1 << 20) - 1, 1 << 20)]
    lane_cuts, wave_cuts = list(lane_cut_cases()), list(wave_cut_cases())
    rules = [(s, l, n, k) for s in (0, 1, 2) for l in (-1, 0, 1) for n in (65535, 65536, (1 << 23) - 1, 1 << 23) for k in (7, 8, 256, 257)]
    possible = [(f, n, k) for f in (0, 1, 2, 8 * 65535, 8 * 65535 + 1) for n in (63, 64) for k in (7, 8, 256, 257)]
    stalls = [[100, 50, 44, 43, 43, 5, 5, 4], [8, 7, 6, 5], [1, 1, 1], [0], [524279, 524279, 458745, 458744, 1], [16, 14, 13, 12, 0, 0]]
    lines = ["geom %d %d %s" % (pal.shape[0], npix, " ".join(float(v).hex() for v in pal.T.reshape(-1))) for _, pal, npix in geoms]
    lines += ["lanecut %d %d %d %d %d %d" % c for c in lane_cuts] + ["wavecut %d %d %d %d %d %d" % c for c in wave_cuts]
    lines += ["rule %d %d %d %d" % c for c in rules] + ["possible %d %d %d" % c for c in possible] + ["weights"]
    lines += ["stall %d %s" % (len(s), " ".join(map(str, s))) for s in stalls]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = iter(run.stdout.splitlines())
    assert len(run.stdout.splitlines()) == len(lines)

    def same_bits(a, b):
        return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))

    for name, pal, npix in geoms:
        words = next(out).split()
        with np.errstate(all="ignore"):
            ref = dither_ref.lane_geometry(pal, npix)
            wp = (pal * dither_ref.FW).T.reshape(-1)
        for lv in range(3):
            g = words[13 * lv:13 * lv + 13]
            lo, hi, inv, cw, G = hexes(g[0:3]), hexes(g[3:6]), hexes(g[6:9]), hexes(g[9:12]), int(g[12])
            assert G == ref.G[lv] == ((64 if npix >= 1 << 20 else 32) if lv < 2 else 32), name
            assert same_bits(lo, ref.lo[lv]) and same_bits(hi, ref.hi[lv]) and same_bits(inv, ref.inv[lv]), (name, lv)
            assert same_bits(cw, ref.cw[lv]), (name, lv)
        amb = np.array(hexes(words[39:42]))
        assert same_bits(amb, [float(ref.amb), float(ref.amb_p), float(ref.amb_x)]), (name, amb, ref.amb, ref.amb_p, ref.amb_x)
        assert same_bits(amb.astype(np.float32).astype(np.float64), amb)                   # (they are f32 values)
        assert same_bits(hexes(words[42:]), wp), name
        if name in ("equal_rows",):
            assert np.all(np.array(hexes(words[3:6])) - np.array(hexes(words[0:3])) <= 2.1e-3)          # extent 0: the grid is the 1e-3 margin
        if name in ("inf", "minus_inf"):
            assert np.isinf(amb[0]) and np.isinf(amb[1]) and np.isfinite(amb[2]), name

    for c in lane_cuts:
        segments, warm, cus, npix, nframe, frames = c
        S, Lmax, fruns, w = map(int, next(out).split())
        assert (S, Lmax, fruns, w) == dither_ref.lane_cut(*c), c
        if not dither_ref.lanes_possible(frames, nframe, 8):
            continue                                                                           # (the callers never cut such a stack)
        # what the kernels' comments rely on
        assert 1 <= S <= 8 * 65535, c
        assert Lmax == -(-npix // S) and w <= npix // S, c
        assert (fruns == 0 and frames == 1) or S == frames * fruns, c
        assert npix // S >= 64 or S == 1, c                                                    # a run of 64 pixels at least

    for c in wave_cuts:
        segments, warm, cus, npix, width, height = c
        S, w = map(int, next(out).split())
        assert (S, w) == dither_ref.wave_cut(*c), c
        assert S >= 1 and (S == 1 or (npix // S >= 128 and max(width, height) >= 16)), c

    for c in rules:
        assert int(next(out)) == int(dither_ref.lane_rule(*c)), c
    for c in possible:
        assert int(next(out)) == int(dither_ref.lanes_possible(*c)), c
    assert same_bits(hexes(next(out).split()), dither_ref.weights())
    for s in stalls:
        assert list(map(int, next(out).split())) == dither_ref.stall_steps(s), s
