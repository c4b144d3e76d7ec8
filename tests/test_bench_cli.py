"""bench.py's command line on a box WITHOUT a GPU (the driver's contract): the HIP path has no CPU fallback, so
every way of starting it must fail loudly -- and `--gpus N` must never quietly measure fewer ranks than it was asked for."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    if env:
        e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def _no_gpu(native):
    return native.lib().patolette_amd_device_count() <= 0


def test_one_gpu_without_a_device_fails_loudly(native):
    if not _no_gpu(native):
        pytest.skip("a HIP device is visible")
    r = _run("--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-extras")
    assert r.returncode != 0
    assert "no HIP device" in (r.stdout + r.stderr)
    assert "\"metric\"" not in r.stdout                       # no line, not even a partial one


def test_more_gpus_than_devices_is_refused_before_any_rank_starts(native):
    if not _no_gpu(native):
        pytest.skip("a HIP device is visible")
    r = _run("--gpus", "2", "--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert "--gpus 2" in (r.stdout + r.stderr) and "HIP device" in (r.stdout + r.stderr)


def test_world_size_that_differs_from_gpus_is_refused():
    """Under an external launcher (WORLD_SIZE set) the line must describe the ranks that exist: `--gpus 4` inside a 2-rank launch is
    a contradiction, not a 4-GPU measurement."""
    r = _run("--gpus", "4", "--steps", "1", "--warmup", "0", env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in (r.stdout + r.stderr)


def test_unknown_configuration_is_an_argument_error():
    r = _run("--config", "nope")
    assert r.returncode == 2 and "invalid choice" in r.stderr


def test_steps_below_one_is_an_argument_error():
    r = _run("--steps", "0")
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_outputs_samples_large_maps_within_64_mb(tmp_path):
    """--dump-outputs on a 4096x4096 step of two images: whole maps as float32 would be 134 MB, so every map is sampled at the
    same fixed pixels, and the sample is the same from call to call."""
    import numpy as np
    import bench
    n = 4096 * 4096
    rng = np.random.default_rng(1)
    maps = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(2)]
    pals = [rng.random((256, 3)) for _ in range(2)]
    bench.dump_outputs(str(tmp_path / "a"), pals, maps, n)
    bench.dump_outputs(str(tmp_path / "b"), pals, maps, n)
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["index_map.npy", "index_map_pixels.npy", "palette.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= 64 * 10 ** 6
    assert a["palette.npy"].dtype == np.float64 and np.array_equal(a["palette.npy"], np.stack(pals))
    px = a["index_map_pixels.npy"]
    assert px.dtype == np.float64 and np.all(np.diff(px) > 0) and 0 <= px[0] and px[-1] < n
    m = a["index_map.npy"]
    assert m.dtype == np.float32 and m.shape == (2, len(px))
    for row, full in zip(m, maps):
        assert np.array_equal(row, full[px.astype(np.int64)].astype(np.float32))
    for f in a:
        assert np.array_equal(a[f], np.load(tmp_path / "b" / f))
