"""bench.py's multi-GPU contract: `python bench.py --gpus N` starts N RCCL ranks itself and reports the ranks
the group really had; the torch.distributed path on one rank measures the same thing as the plain path."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import ROOT


def _bench(*flags, timeout=900, full=True):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    # --full for the kernel events (roofline); none of its costly legs
    extra = ["--full", "--no-cpu-baseline", "--no-extras", "--extra-streams", "0"] if full else []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra + list(flags),
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = None
    for ln in r.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = json.loads(ln)
    return r, line


@pytest.mark.gpu
def test_rccl_path_on_one_rank_measures_what_the_plain_path_measures(gpu):
    r0, plain = _bench("--gpus", "1", "--steps", "12", "--warmup", "3")
    assert r0.returncode == 0 and plain is not None, r0.stdout[-2000:] + r0.stderr[-2000:]
    r1, dist = _bench("--gpus", "1", "--force-dist", "--steps", "12", "--warmup", "3")
    assert r1.returncode == 0 and dist is not None, r1.stdout[-2000:] + r1.stderr[-2000:]
    assert plain["n_gpus"] == 1 and dist["n_gpus"] == 1
    assert "RCCL gather" in dist["config"]["final_gather"] and plain["config"]["final_gather"].startswith("none")
    assert abs(dist["value"] / plain["value"] - 1.0) < 0.10, (plain["value"], dist["value"])
    assert dist["roofline"]["kernel"] == plain["roofline"]["kernel"]


@pytest.mark.gpu
def test_gpus_n_starts_n_ranks_or_fails_loudly(gpu):
    """`bench.py --gpus 2` with no launcher around it: two ranks on a box with two GPUs (n_gpus == 2 in the line), a non-zero
    exit and NO line on a one-GPU box -- never a one-GPU measurement labelled as something else."""
    have = gpu.patolette_amd_device_count()
    r, line = _bench("--gpus", "2", "--steps", "2", "--warmup", "1", timeout=600)
    if have >= 2:
        assert r.returncode == 0 and line is not None and line["n_gpus"] == 2, r.stdout[-2000:] + r.stderr[-2000:]
        assert line["scaling"] == "weak"
    else:
        assert r.returncode != 0 and line is None, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("streams", [1, 2])
def test_n_greater_one_code_path_runs_on_ranks_sharing_a_device(gpu, streams, tmp_path):
    """bench.py's N > 1 branch (batch shard + final gather) EXECUTED on a one-GPU box: two ranks share the device
    (`--oversubscribe`: gloo + host staging for the collective, because RCCL refuses two ranks on one GPU); sharding by rank, the
    per-step asynchronous gather of the u8 maps, the palette gather, the index arithmetic of `map_ptr` and the max-over-ranks
    timing are the lines the RCCL run executes.  Rank 0 then quantises every rank's images itself, one call per image: what the
    gather delivered must be those maps and palettes bit for bit."""
    r, line = _bench("--gpus", "2", "--oversubscribe", "--check-gather", "--steps", "4", "--warmup", "2", "--config", "c2",
                     "--streams", str(streams), "--dump-outputs", str(tmp_path), timeout=600)
    assert r.returncode == 0 and line is not None, r.stdout[-2000:] + r.stderr[-2000:]
    assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    # the last step's outputs of both ranks, as rank 0 gathered them
    pal, pmap = np.load(tmp_path / "palette.npy"), np.load(tmp_path / "index_map.npy")
    assert pal.shape == (2 * streams, 256, 3) and pmap.shape == (2 * streams, 1920 * 1080)
    assert pmap.min() >= 0 and pmap.max() <= 255 and np.all(pmap == np.round(pmap))
    assert "TEST MODE" in line["config"]["final_gather"]
    gc = line["gather_check"]
    assert gc["ranks"] == 2 and gc["maps_compared"] == 2 * 4 * streams
    assert gc["map_mismatches"] == 0 and gc["palettes_identical"]
    # whole-job value = the pixels of BOTH ranks over the max-over-ranks time
    px = 1920 * 1080 * 4 * 2 * streams
    assert abs(line["value"] - px / (line["ms_per_step"] * 4e-3) / 1e6) <= 2e-3 * line["value"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_the_last_one_returned(gpu, native, tmp_path):
    """A plain run (no --full) times its steps and reports nothing else; --dump-outputs holds what the last timed step returned.
    c2, one warm-up, two steps: the pool has three images, the last step quantises the one of seed 2, and one separate call on
    that image gives the same palette and index map (the map is whole at this size)."""
    r, line = _bench("--config", "c2", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path), full=False, timeout=600)
    assert r.returncode == 0 and line is not None, r.stdout[-2000:] + r.stderr[-2000:]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    for k in ("roofline", "first_call", "cpu_baseline", "parity", "throughput_concurrent", "small_image", "north_star_kernels"):
        assert line[k] is None, k
    assert line["kernels"] == {} and line["config"]["kernel_events_in_timed_region"] == "none"
    assert sorted(os.listdir(tmp_path)) == ["index_map.npy", "palette.npy"]
    pal, pmap = np.load(tmp_path / "palette.npy"), np.load(tmp_path / "index_map.npy")
    w, h, K = 1920, 1080, 256
    n = w * h
    assert pal.dtype == np.float64 and pal.shape == (1, K, 3)
    assert pmap.dtype == np.float32 and pmap.shape == (1, n)
    img = gpu.patolette_amd_malloc(3 * n * 8)
    dmap = gpu.patolette_amd_malloc(n)
    try:
        assert img and dmap and gpu.patolette_amd_fill_image(img, n, 2) == 0
        opts = native.QuantizationOptions(False, False, 2, 0, 512 ** 2, False)
        want_pal = np.zeros((K, 3), dtype=np.float64, order="F")
        code = C.c_int(9)
        gpu.patolette_amd_device(w, h, img, None, K, C.byref(opts), want_pal.ctypes.data_as(native.dp), dmap, 1, C.byref(code))
        assert code.value == 0, native.last_error()
        want_map = np.empty(n, dtype=np.uint8)
        assert gpu.patolette_amd_memcpy_d2h(want_map.ctypes.data_as(C.c_void_p), dmap, n) == 0
    finally:
        gpu.patolette_amd_free(img)
        gpu.patolette_amd_free(dmap)
    assert np.array_equal(pal[0], want_pal)
    assert np.array_equal(pmap[0], want_map.astype(np.float32))
