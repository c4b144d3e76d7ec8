"""The palette-given entries' host rules (csrc/given.h) on the CPU under sanitizers.

given_check.cpp is a stand-alone program over the header alone: the caller's palette (u8 and f64, trailing fill rows, a fill row that
stays, values that are not finite, the bytes of values outside [0, 1]), 2- and 8-byte index elements into the device's 4 (skip
index, saturation, the collision with a saturated skip index), 1- and 4-byte device elements into 1, 2, 4 and 8 over ranges, and the
device's values of the transparent and skip indices; each compared with a restatement of the documented rule, in heap buffers of
exactly the documented sizes.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "patolette_amd", "csrc")


def test_given_rules_hold_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "given_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "given_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "palettes agree" in run.stdout
