"""Caller threads that overlap in time must get what one thread gets alone, bit for bit.

include/patolette_amd.h promises every calling thread an engine of its own from a per-device pool, per-thread last_error /
last_stats / last_split_trace / set_invariant_sums, and engines that go back to the pool when their thread exits.  What the
threads share on the host -- the once-per-device kernel attributes (PerDeviceOnce), the sRGB cube's ICtCp box, the size-only tables'
switches, the process-wide knobs, the pool itself -- is reached only when calls overlap, which no other module makes them do.

tests/threads_worker.py holds ONE table of seeded jobs (every entry point; K = 8, 64, 300; three colour spaces; dither on and
off; KMeans off, sampled and full; weights explicit, derived and none; a fused remap of 2^22 pixels; an image above 2 Mpixel; a
batch from a caller thread).  Each scenario is one fresh child process (the cold ones need a process in which no call has
happened yet), started with subprocess and sys.executable, one at a time, each under its own time limit:

    serial       the table once on one thread: the expected values (everything a call returns and reports)
    cold_mixed   six threads make their FIRST call together, each on another job, then walk the rest of the table
    cold_same    six threads make their first call together on the SAME job (the fused remap; K = 256 with KMeans)
    soak         six threads, three passes each from their own offsets, fresh memory poisoned, late growths counted
    churn        short-lived threads come and go beside two long-lived ones while the main thread releases the workspace
    state        two threads in lockstep: a failing call beside a good one, invariant sums on beside off
    two_devices  three threads per GPU (skipped with one GPU)

The parent compares every concurrent result with the serial file bit for bit (arrays above 1 MiB by SHA-256) and the small jobs
of the cold_mixed run with the CPU oracle at the suite's bars: maps bit for bit, f64 palettes to 1e-9.

Time limit of a concurrent child: it cannot sensibly need more than the serial child's wall time (measured here, start of the
process to its end) times the table walks it makes; five times that product is allowed for a shared machine, 120 s at least.
A child that dies (a signal, exit status 134 / 139, a thread that never came back, the time limit) fails its test with the
child's stderr, and every later test of the module skips: nothing more is started on the GPU, nothing is tried again.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import frames_ref, remap_ref, rgba_ref
from tests import threads_worker as tw

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "threads_worker.py")
SERIAL_LIMIT = 900.0           # the serial child has no measurement to go by yet
_DEAD = {"why": None}          # set when a child died: the remaining tests skip


def _child(scenario, out, args=(), limit=SERIAL_LIMIT):
    """Run one child to its end -> (npz, wall seconds, stderr).  Fails the test on any non-zero exit; marks the module dead on a death."""
    if _DEAD["why"]:
        pytest.skip("an earlier child died (%s): nothing more is started on the GPU" % _DEAD["why"])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [WORKER, scenario, out] + list(args)
    t0 = time.monotonic()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)     # (kills the child when the limit passes)
    except subprocess.TimeoutExpired as ex:
        _DEAD["why"] = "%s ran into its limit of %.0f s" % (scenario, limit)
        err = ex.stderr.decode("utf-8", "replace") if isinstance(ex.stderr, bytes) else (ex.stderr or "")
        pytest.fail("%s\n%s" % (_DEAD["why"], err[-6000:]))
    wall = time.monotonic() - t0
    print("threads: child %-11s %s: exit %d, wall %.1f s (limit %.0f s)" % (scenario, " ".join(args), r.returncode, wall, limit))
    if r.returncode < 0 or r.returncode in (3, 124, 134, 137, 139):
        _DEAD["why"] = "%s ended with status %d" % (scenario, r.returncode)
        pytest.fail("%s\n%s" % (_DEAD["why"], r.stderr[-6000:]))
    if r.returncode != 0 or "THREADS-WORKER-DONE" not in r.stdout:
        pytest.fail("child %s failed (exit %d)\n%s\n%s" % (scenario, r.returncode, r.stdout[-2000:], r.stderr[-6000:]))
    return np.load(out, allow_pickle=False), wall, r.stderr


@pytest.fixture(scope="module")
def serial(gpu, tmp_path_factory):
    """(the serial child's file, its wall time, its stderr)"""
    out = str(tmp_path_factory.mktemp("threads") / "serial.npz")
    return _child("serial", out)


def _limit(serial_wall, walks):
    return max(120.0, 5.0 * serial_wall * walks)


def _fields(npz, prefix):
    """field names (without the digest mark) stored under prefix/"""
    return sorted(k[len(prefix) + 1:].replace("#sha256", "") for k in npz.files if k.startswith(prefix + "/"))


def _diffs(got, runs, ref):
    """Every array stored for the runs [(tag, pass, job)] against ref(job, field) -> list of differences (empty = bit for bit).
    A run that stored nothing, or not the fields the reference has, is a difference too."""
    out = []
    for tag, r, name in runs:
        prefix = "%s/%d/%s" % (tag, r, name)
        keys = [k for k in got.files if k.startswith(prefix + "/")]
        if not keys:
            out.append("%s: no result" % prefix)
            continue
        for k in keys:
            field = k[len(prefix) + 1:]
            hashed = field.endswith("#sha256")
            want = ref(name, field[:-7] if hashed else field)
            if want is None:
                out.append("%s: the serial run has no such field" % k)
                continue
            a = got[k]
            if hashed:
                same = np.array_equal(a, tw.digest(want))
            else:
                same = a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes()
            if not same:
                note = ""
                if not hashed and a.shape == want.shape and a.dtype.kind in "fiu":
                    note = " (%d of %d elements differ)" % (int(np.sum(~((a == want) | ((a != a) & (want != want))))), a.size)
                out.append("%s differs from the serial run%s" % (k, note))
        want_fields = ref(name, None)
        if _fields(got, prefix) != want_fields:
            out.append("%s: fields %s, the serial run has %s" % (prefix, _fields(got, prefix), want_fields))
    return out


def _serial_ref(npz, tag=None):
    """ref(job, field) over the serial file (tag None) or over the runs `tag`/0/ of another file; field None -> the field names"""
    def ref(name, field):
        prefix = name if tag is None else "%s/0/%s" % (tag, name)
        if field is None:
            return _fields(npz, prefix)
        key = "%s/%s" % (prefix, field)
        return npz[key] if key in npz.files else None
    return ref


def _no_thread_errors(got):
    errs = [str(e) for e in got["errors"]]
    assert not errs, "\n".join(errs)


def _walk_runs(tags, passes, jobs):
    return [(t, r, j.name) for t in tags for r in range(passes) for j in jobs]


# ---- the oracle side ----------------------------------------------------------------------------------------------------------
def _oracle_check(ob, j, res):
    """One small job's result (field -> array, all in full) against the CPU oracle: maps bit for bit, f64 palettes to 1e-9."""
    def pal_close(got, want, what="palette"):
        err = float(np.nanmax(np.abs(got - want)))
        print("threads: %s vs oracle: %s max abs diff %.3g" % (j.name, what, err))
        assert got.shape == want.shape and np.allclose(got, want, rtol=0, atol=1e-9, equal_nan=True), (j.name, what, err)

    def map_same(got, want):
        mism = int(np.sum(np.asarray(got).reshape(-1).astype(np.int64) != np.asarray(want).reshape(-1).astype(np.int64)))
        print("threads: %s vs oracle: %d of %d map entries differ" % (j.name, mism, np.asarray(want).size))
        assert mism == 0, (j.name, mism)

    if j.entry in ("host", "device", "u8"):
        if j.entry == "u8":
            h, w = j.img.shape[:2]
            flat = ob.planar(j.img.reshape(-1, 3).astype(np.float64) / 255.0)
        else:
            h, w = j.h, j.w
            flat = ob.planar(j.img)
        k = j.kw
        ec, pal_o, map_o = ob.patolette(w, h, flat, j.wts, j.K, dither=k["dither"], color_space=k["color_space"],
                                        kmeans_niter=k["kmeans_niter"], kmeans_max_samples=k["kmeans_max_samples"])
        assert ec == 0
        pal_close(res["pal"], pal_o)
        map_same(res["map"], map_o)
        if j.entry == "u8":
            pal8 = np.clip(res["pal"] * 255, 0, 255).astype(np.uint8) * (res["pal"][:, :1] != -1)
            assert np.array_equal(res["pal8"], pal8) and np.array_equal(res["quant"], pal8[res["map"].astype(np.int64)])
    elif j.entry == "rgba":
        h, w = j.img.shape[:2]
        tr = j.transparent.reshape(-1)
        rows = j.img[..., :3].reshape(-1, 3).astype(np.float64) / 255.0
        ec, pal_o, _ = ob.patolette(int((~tr).sum()), 1, ob.planar(rows[~tr]), None, j.K - 1, dither=True, color_space=2, kmeans_niter=0)
        assert ec == 0
        pal_close(res["pal"][1:], pal_o)
        assert np.all(res["pal"][0] == 0) and tuple(res["pal8"][0]) == (0, 0, 0, 0) and int(res["tidx"][0]) == 0
        rec = ob.convert("ictcp_to_rec2020", ob.convert("srgb_to_ictcp", ob.planar(rows))).reshape(3, h * w).T.copy()
        walk = rgba_ref.masked_dither(ob, rec, w, h, res["map_palette"], ~tr)      # the walk with the palette the device stage used
        map_same(res["map"], np.where(tr, 0, walk + 1))
        assert np.array_equal(res["quant"], res["pal8"][res["map"].astype(np.int64)])
    elif j.entry == "frames":
        k = {n: v for n, v in j.kw.items() if n != "tile_size"}
        pal_o, maps_o = frames_ref.quantize_frames(ob, j.img, j.K, **k)
        pal_close(res["pal"], pal_o)
        map_same(res["map"], maps_o)
        assert np.array_equal(res["quant"], res["pal8"][res["map"].astype(np.int64)])
    else:
        assert j.entry == "remap"
        m_ref, q_ref = remap_ref.remap(ob, j.img, j.palette, dither=j.dither)
        map_same(res["map"], m_ref)
        assert np.array_equal(res["quant"], q_ref)


# ---- the scenarios ------------------------------------------------------------------------------------------------------------
def test_serial_run_is_complete(gpu, serial):
    """the expected values exist for every job, and the dithered 8-bit job is at a size where one lane walks each run"""
    npz, wall, _ = serial
    for j in tw.table():
        assert _fields(npz, j.name), j.name
    assert int(npz["late_growths"]) == 0
    j = tw.job("u8_k64_dither_lanes")
    try:
        tw.setup_process(gpu)                                    # the knob as every child sets it
        assert gpu.patolette_amd_dither_layout_in_use(j.img.shape[1], j.img.shape[0], j.K) == 1
    finally:
        gpu.patolette_amd_dither_layout(-1)


def test_cold_start_mixed_jobs(gpu, ob, serial, tmp_path):
    """Six threads, first library call of the process at the same moment, each on another job; then the rest of the table.
    Every result is the serial one; the small jobs' results are the oracle's."""
    npz, wall, _ = serial
    jobs = tw.table()
    got, _, err = _child("cold_mixed", str(tmp_path / "cold_mixed.npz"), limit=_limit(wall, tw.THREADS))
    _no_thread_errors(got)
    tags = ["t%d" % t for t in range(tw.THREADS)]
    d = _diffs(got, _walk_runs(tags, 1, jobs), _serial_ref(npz))
    assert not d, "\n".join(d)
    # the oracle on what the concurrent threads returned: job i from thread i mod 6
    for i, j in enumerate(jobs):
        if j.oracle:
            prefix = "t%d/0/%s" % (i % tw.THREADS, j.name)
            res = {k[len(prefix) + 1:]: got[k] for k in got.files if k.startswith(prefix + "/")}
            assert not [k for k in res if k.endswith("#sha256")], (j.name, sorted(res))
            _oracle_check(ob, j, res)


@pytest.mark.parametrize("name", ["remap_nearest_fused", "host_k256_kmfull"])
def test_cold_start_same_job(gpu, serial, tmp_path, name):
    """Six threads, first call together on the SAME job: all of them at the same once-per-device steps and size-only tables."""
    npz, wall, _ = serial
    got, _, err = _child("cold_same", str(tmp_path / "cold_same.npz"), [name], limit=_limit(wall, 1))
    _no_thread_errors(got)
    d = _diffs(got, _walk_runs(["t%d" % t for t in range(tw.THREADS)], 2, [tw.job(name)]), _serial_ref(npz))
    assert not d, "\n".join(d)


def test_warm_soak_with_poison(gpu, serial, tmp_path):
    """Six threads, three passes each from their own offsets, fresh memory poisoned: serial results, no late growth.

    The walks meet the sizes in different orders, so an engine grows buffers in the middle of a call that
    tests/test_gpu_workspace_state.py (larger image first) never grows there: the pinned staging of the KMeans subsample list
    when the 65 536-entry list (host_k64_...) comes before the 262 144-entry one (host_k128_chunked), the index map when a small
    image comes before a large one.  Both happen right after the chunked upload has been waited for, and the count must stay 0."""
    npz, wall, _ = serial
    passes = 3
    got, _, err = _child("soak", str(tmp_path / "soak.npz"), [str(passes)], limit=_limit(wall, tw.THREADS * passes))
    _no_thread_errors(got)
    d = _diffs(got, _walk_runs(["t%d" % t for t in range(tw.THREADS)], passes, tw.table()), _serial_ref(npz))
    assert not d, "\n".join(d)
    assert int(got["late_growths"]) == 0, "workspace buffers replaced while work was queued:\n" + err[-4000:]


def test_thread_churn_and_release(gpu, serial, tmp_path):
    """Short-lived threads run one job and exit beside two long-lived ones while the main thread calls
    patolette_amd_release_workspace() again and again; every result, the calls made after a release included, is the serial one
    (an engine in use is not idle: the long-lived threads never lose theirs).  Then the header's contract in device memory, on
    two threads that ran the 2.2 Mpixel job and exited.  The header puts an engine at ~170 bytes per pixel of the largest image
    it has seen; half of that is asked for, twice:
      * a thread's engine is handed back when the thread exits, not freed: with both threads gone that memory is still held;
      * the release frees the calling thread's engine and every idle pooled one: one release gives it back.
    Both are differences of free memory over a short stretch, so what the runtime keeps for itself does not enter."""
    npz, wall, _ = serial
    got, _, err = _child("churn", str(tmp_path / "churn.npz"), limit=_limit(wall, 8))
    _no_thread_errors(got)
    jobs = tw.table()
    small = [j for j in jobs if j.oracle]
    rounds = int(got["release_rounds"])
    assert rounds >= 4
    runs = _walk_runs(["long0", "long1"], 2, jobs)
    runs += [("short%d" % s, 0, small[s % len(small)].name) for s in range(2 * rounds)]
    runs += [("main%d" % r, 0, small[r % len(small)].name) for r in range(rounds)]
    runs += [("after", 0, small[0].name)]
    d = _diffs(got, runs, _serial_ref(npz))
    assert not d, "\n".join(d)
    d = _diffs(got, [("tail0", 0, "host_k128_chunked"), ("tail1", 0, "host_k128_chunked")], _serial_ref(npz))
    assert not d, "\n".join(d)
    before, idle, end = int(got["free_before_tail"]), int(got["free_idle"]), int(got["free_end"])
    print("threads: churn: %d releases; device memory free %.0f MiB before the two last threads, %.0f MiB after they exited, %.0f MiB "
          "after the release" % (rounds, before / 2 ** 20, idle / 2 ** 20, end / 2 ** 20))
    two_engines = 2 * 170 * int(got["tail_pixels"])
    assert before - idle >= two_engines // 2, "the engines of exited threads were not kept: %d bytes held" % (before - idle)
    assert end - idle >= two_engines // 2, "the release gave back %d bytes of about %d" % (end - idle, two_engines)


def test_per_thread_state(gpu, serial, tmp_path):
    """A fails on its arguments while B succeeds; A runs with invariant sums, B without.  Neither sees the other's state."""
    npz, wall, _ = serial
    got, _, err = _child("state", str(tmp_path / "state.npz"), limit=_limit(wall, 3))
    _no_thread_errors(got)
    assert int(got["A/bad_exit_code"]) == -1
    assert str(got["A/last_error_after_step1"]).startswith(tw.REMAP_BOTH_MISSING), str(got["A/last_error_after_step1"])
    assert str(got["B/last_error_after_step1"]) == "", str(got["B/last_error_after_step1"])
    # the setting is the thread's own: it is still there at the thread's end, whatever the other thread set meanwhile
    assert int(got["A/invariant_after"]) == 1 and int(got["B/invariant_after"]) == 0
    names = tw.STATE_JOBS
    # B (setting off): the serial file's results, stats and trace of ITS calls, read after A's different call had finished
    runs_b = [("B", 0, names[1])] + [("B", r + 1, names[i]) for r, i in enumerate((1, 0, 3, 2))]
    d = _diffs(got, runs_b, _serial_ref(npz))
    assert not d, "\n".join(d)
    # A (setting on; its engine has just failed a call): the one-thread run with the setting on
    runs_a = [("A", r + 1, names[i]) for r, i in enumerate((0, 1, 2, 3))]
    d = _diffs(got, runs_a, _serial_ref(got, "serial_invariant"))
    assert not d, "\n".join(d)


def test_two_devices(gpu, serial, tmp_path):
    """three threads on device 0, three on device 1"""
    if gpu.patolette_amd_device_count() < 2:
        pytest.skip("one GPU visible")
    npz, wall, _ = serial
    got, _, err = _child("two_devices", str(tmp_path / "two_devices.npz"), limit=_limit(wall, tw.THREADS))
    _no_thread_errors(got)
    d = _diffs(got, _walk_runs(["t%d" % t for t in range(tw.THREADS)], 1, tw.table()), _serial_ref(npz))
    assert not d, "\n".join(d)
