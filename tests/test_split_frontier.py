"""The split loops' shared greedy step (csrc/split_frontier.h) against the whole-frontier loop, on the CPU under sanitizers.

frontier_check.cpp is a stand-alone program over the header alone: random candidate trees (K at the block edges, 1 to 12 base
clusters, exact ties, values below DELTA, undecided rows that block the step), the blocked form and lq_replay_plain compared on
return value, result, commits and stopped_early, with and without the sabotaged step.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "patolette_amd", "csrc")


def test_shared_step_equals_plain_loop(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "frontier_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "frontier_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "trees agree" in run.stdout
