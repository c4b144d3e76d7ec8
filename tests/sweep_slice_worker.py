"""Worker of tests/test_gpu_sweep_edges.py::test_sliced_image_at_an_odd_boundary_beyond_the_infinity_cache: ONE image dealt
out over two ranks (patolette_amd_slice, gloo, the ranks may share a GPU) at an odd pixel boundary, each slice large enough that
the partition kernel takes its last-use loads in the tiling-invariant form (launch_partition).  Each rank then quantises the WHOLE
image alone with the invariant sums switched on and demands the same bits: the same palette, and its slice of the same index map
(as tests/slice_worker.py does for its smaller images)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before patolette_amd: both link a HIP runtime)
import torch.distributed as dist  # noqa: E402

N0, N1 = 5600001, 5600002                           # pixels of the two slices: an odd boundary, an odd total


def main():
    out_path, weighted = sys.argv[1], sys.argv[2] == "weighted"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    import patolette_amd as p
    from patolette_amd import _native
    from patolette_amd import dist as pdist
    L = _native.lib()
    assert L.patolette_amd_set_device(dev) == 0
    n = N0 + N1
    planes = 4 if weighted else 3
    assert 2 * planes * min(N0, N1) * 8 > 256 << 20   # every slice beyond the threshold of launch_partition
    rng = np.random.default_rng(20261020)           # the same image on every rank
    colors = rng.random((n, 3))
    weights = (1.0 + 3.0 * rng.random(n)) if weighted else None
    b, c = ((0, N0), (N0, N1))[rank]
    kw = dict(color_space=2, kmeans_niter=0)
    res = pdist.quantize_image_sharded(n, b, colors[b:b + c], 16, dist, weights=None if weights is None else weights[b:b + c], **kw)
    L.patolette_amd_set_invariant_sums(1)
    try:
        one = p.quantize(n, 1, colors, 16, dither=False, tile_size=0, weights=weights, **kw)
    finally:
        L.patolette_amd_set_invariant_sums(0)
    notes = []
    ok = bool(res[0]) and bool(one[0])
    if ok:
        same_pal = np.array_equal(res[1], one[1])
        same_map = np.array_equal(res[2], one[2][b:b + c])
        notes.append("slice %d+%d of %d: palette %s, map %s" % (b, c, n, "same" if same_pal else "DIFFERS", "same" if same_map else "DIFFERS"))
        ok = same_pal and same_map
    else:
        notes.append("sliced call: %s; whole image: %s" % (res[3] if len(res) > 3 else res[0], one[3]))
    with open("%s.%d" % (out_path, rank), "w") as f:
        f.write(("OK\n" if ok else "MISMATCH\n") + "\n".join(notes) + "\n")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
