"""Call every entry a host driver serves on a fixed set of small images and dump palettes, maps, quantized images and the calls'
counters to an .npz -- the A/B of two builds, or of a library switch, across two processes:

    python tools/dump_results.py a.npz            (once per build or environment)
    python tools/dump_results.py --compare a.npz b.npz      -> ALL EQUAL, or the names that differ

Entries: quantize (planar, row-major; given and derived weights), quantize_u8, quantize_frames, quantize_rgba (none, some and all
pixels transparent; a tensor view that is not 4-byte aligned), remap and remap_rgba in all three modes, quantize_rgba_frames,
quantize_u8_batch -- the 8-bit ones from a numpy array and from a torch device tensor -- then the other routes through the knobs
the tests use: the chunked upload (PAMD_UPLOAD_CHUNK_MIN), patolette_amd_debug_remap_two_pass, patolette_amd_dither_layout,
patolette_amd_debug_nn_route.  Those images (96 x 80) are below the 65 536 pixels from which patolette_amd_dither_layout(1) selects
the lane layout, so the `route_` calls follow: quantize with dither in the three colour spaces on 256 x 256, quantize_frames on
4 x 128 x 128, quantize_rgba and remap_rgba on 256 x 288 with 5 % of the pixels transparent, remap fused and two-pass -- each under
the lane layout, the wavefront layout, the single chain (patolette_amd_dither_config(1, -1)) and the lane walk that gives up at its
first stalled pass (warm-up 1, patolette_amd_debug_dither_stall_passes(0), patolette_amd_debug_dither_solo_cap(0)) -- and K = 300 on
96 x 80, the wavefront layout's generic loop.  `--large` adds the f64 images of up to 2048 x 2048 this tool began with.

A k_fill_weights launch goes ahead of every call, so a `rocprofv3 --kernel-trace --memory-copy-trace --output-format rocpd` of this
script can be cut into calls:

    python tools/dump_results.py --enqueued TRACE_DIR [--names a.npz] > list.txt

prints per call the kernels with their grids and the copies with direction and bytes in order of start, runs of one line folded;
sorted instead for the calls whose work runs on more than one stream at once (the batch; the chunked uploads, whose conversions
run beside the copies; route_lanes_* and route_gives_up_*, whose lane walks build their record grids on two side streams)."""
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTERS = ("split_evals", "lq_rounds", "n_base_clusters", "n_clusters", "kmeans_samples", "dither_segments", "dither_repairs",
            "dither_rounds", "dither_through", "dither_jumps", "dither_solo")


def smooth(w, h):
    y, x = np.mgrid[0:h, 0:w]
    r = 0.5 + 0.5 * np.sin(x / 37.0) * np.cos(y / 53.0)
    g = (x + y) / float(w + h)
    b = 0.5 + 0.5 * np.cos((x - y) / 71.0)
    return np.stack([r, g, b], axis=-1).reshape(-1, 3)


def large_cases():
    rng = np.random.default_rng(11)
    yield "noise2048_K256", 2048, 2048, rng.random((2048 * 2048, 3)), None, 256, dict(color_space=2, kmeans_niter=0)
    yield "noise512_K256_km", 512, 512, rng.random((512 * 512, 3)), None, 256, dict(color_space=2, kmeans_niter=8)
    yield "smooth_K256", 1000, 800, smooth(1000, 800), None, 256, dict(color_space=2, kmeans_niter=0)
    yield "smooth_K37_luv_w", 640, 480, smooth(640, 480) * 0.8 + 0.2 * rng.random((640 * 480, 3)), 0.5 + 3 * rng.random(640 * 480), 37, dict(color_space=1, kmeans_niter=0)
    yield "srgb_K1000", 700, 700, rng.random((490000, 3)) ** 2.0, None, 1000, dict(color_space=0, kmeans_niter=0)
    blobs = np.concatenate([0.05 * rng.standard_normal((20000, 3)) + c for c in rng.random((12, 3))]).clip(0, 1)
    yield "blobs_K64", 240000, 1, blobs, None, 64, dict(color_space=2, kmeans_niter=0)
    yield "blobs_K7", 240000, 1, blobs, None, 7, dict(color_space=1, kmeans_niter=0)
    yield "tiny_K16", 9, 7, rng.random((63, 3)), None, 16, dict(color_space=2, kmeans_niter=0)


W, H, FW, FH, F, K = 96, 80, 40, 24, 3, 20
RW, RH = 256, 288                                                # the dither-route cases: RW x RW, 4 frames of RW/2 x RW/2, RW x RH with alpha


def image_u8(w, h, seed, frames=None):
    rng = np.random.default_rng(seed)
    one = lambda: ((smooth(w, h) * 0.8 + 0.2 * rng.random((w * h, 3))) * 255.0).astype(np.uint8).reshape(h, w, 3)   # noqa: E731
    return one() if frames is None else np.stack([one() for _ in range(frames)])


def with_alpha(rgb, kind):
    """RGB + an alpha channel: 'none' transparent, 'some' (outside a disc, per frame) or 'all'."""
    h, w = rgb.shape[-3:-1]
    y, x = np.mgrid[0:h, 0:w]
    disc = ((x - w / 2.0) ** 2 + (y - h / 2.0) ** 2 <= (0.45 * min(w, h)) ** 2)
    alpha = {"none": np.full((h, w), 255), "some": np.where(disc, 255, 0), "all": np.zeros((h, w))}[kind].astype(np.uint8)
    return np.concatenate([rgb, np.broadcast_to(alpha, rgb.shape[:-1])[..., None]], axis=-1)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def calls(large):
    """(name, function returning the arrays to keep) per call, in a fixed order."""
    import torch
    import patolette_amd as p
    from patolette_amd import _native
    L = _native.lib()
    rng = np.random.default_rng(5)
    colors = smooth(W, H) * 0.8 + 0.2 * rng.random((W * H, 3))
    wts = 0.5 + 3 * rng.random(W * H)
    img, frames = image_u8(W, H, 1), image_u8(FW, FH, 2, F)
    fwts = 0.5 + 3 * rng.random(F * FW * FH)
    kw = dict(kmeans_niter=2)
    # every input, and the remaps' palettes, before the first call: what making them enqueues belongs to no call
    arrays = {"img": img, "frames": frames}
    # the route cases' images: 65 536 pixels and more, the RGBA one with 65 536 opaque pixels and transparent ones scattered inside it
    rcolors = smooth(RW, RW) * 0.8 + 0.2 * rng.random((RW * RW, 3))
    alpha = np.where(rng.random((RH, RW)) < 0.05, 0, 255).astype(np.uint8)
    arrays.update(rimg=image_u8(RW, RW, 4), rframes=image_u8(RW // 2, RW // 2, 5, 4), rrgba=np.concatenate([image_u8(RW, RH, 6), alpha[..., None]], axis=-1))
    assert int((alpha == 255).sum()) >= 65536
    for kind in ("none", "some", "all"):
        arrays["img_" + kind], arrays["frames_" + kind] = with_alpha(img, kind), with_alpha(frames, kind)
    tensors = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}
    flat = torch.zeros(1 + W * H * 4, dtype=torch.uint8, device="cuda")
    flat[1:] = tensors["img_some"].reshape(-1)
    odd = flat[1:].view(H, W, 4)                                   # a tensor view one byte into its allocation: the RGBA entries stage such pixels
    assert odd.data_ptr() % 4 == 1
    pal8 = p.quantize_u8(img, K, dither=False, tile_size=0, **kw)[1]
    palrgba = p.quantize_rgba(arrays["img_some"], K, dither=False, tile_size=0, **kw)[1]
    torch.cuda.synchronize()

    def quantize(src, **k):
        def run():
            r = p.quantize(W, H, src, K, **k)
            assert r[0], r[-1]
            return dict(pal=r[1], map=r[2])
        return run

    def u8(fn, *a, **k):                                           # quantize_u8 / quantize_frames / quantize_rgba* / remap / remap_rgba
        def run():
            r = fn(*a, **k)
            assert r[0], r[-1]
            return {"out%d" % i: host(v) for i, v in enumerate(r[1:-1])}
        return run

    for name, src in (("planar", np.asfortranarray(colors)), ("rows", np.ascontiguousarray(colors))):
        yield "quantize_%s" % name, quantize(src, dither=False, tile_size=0, **kw)
        yield "quantize_%s_dither_luv" % name, quantize(src, dither=True, tile_size=0, color_space=p.ColorSpace_CIELuv, **kw)
        yield "quantize_%s_weights" % name, quantize(src, dither=True, tile_size=0, weights=wts, **kw)
        yield "quantize_%s_derived" % name, quantize(src, dither=False, tile_size=512, **kw)
    yield "quantize_planar_palette_only", quantize(np.asfortranarray(colors), palette_only=True, tile_size=0, **kw)
    for where, at in (("np", arrays), ("torch", tensors)):
        for dither in (False, True):
            d = "_dither" if dither else ""
            yield "u8_%s%s" % (where, d), u8(p.quantize_u8, at["img"], K, dither=dither, tile_size=0, **kw)
            yield "u8_%s%s_weights" % (where, d), u8(p.quantize_u8, at["img"], K, dither=dither, tile_size=0, weights=wts, **kw)
            yield "u8_%s%s_derived" % (where, d), u8(p.quantize_u8, at["img"], K, dither=dither, tile_size=512, **kw)
            yield "frames_%s%s" % (where, d), u8(p.quantize_frames, at["frames"], K, dither=dither, tile_size=0, **kw)
            yield "frames_%s%s_weights" % (where, d), u8(p.quantize_frames, at["frames"], K, dither=dither, tile_size=0, weights=fwts, **kw)
            yield "frames_%s%s_derived" % (where, d), u8(p.quantize_frames, at["frames"], K, dither=dither, tile_size=512, **kw)
            for kind in ("none", "some", "all"):
                yield "rgba_%s_%s%s" % (kind, where, d), u8(p.quantize_rgba, at["img_" + kind], K, dither=dither, tile_size=0, **kw)
            yield "rgba_some_%s%s_weights" % (where, d), u8(p.quantize_rgba, at["img_some"], K, dither=dither, tile_size=0,
                                                            weights=wts, **kw)
            yield "rgba_some_%s%s_derived" % (where, d), u8(p.quantize_rgba, at["img_some"], K, dither=dither, tile_size=512, **kw)
            yield "rgba_frames_%s%s" % (where, d), u8(p.quantize_rgba_frames, at["frames_some"], K, dither=dither, tile_size=0, **kw)
        yield "u8_%s_luv" % where, u8(p.quantize_u8, at["img"], K, dither=False, tile_size=0, color_space=p.ColorSpace_CIELuv, **kw)
        yield "u8_%s_K300" % where, u8(p.quantize_u8, at["img"], 300, dither=False, tile_size=0, **kw)
        yield "rgba_some_%s_luv" % where, u8(p.quantize_rgba, at["img_some"], K, dither=False, tile_size=0,
                                             color_space=p.ColorSpace_CIELuv, **kw)
        yield "rgba_frames_%s_ordered" % where, u8(p.quantize_rgba_frames, at["frames_some"], K, dither="ordered", tile_size=0, **kw)
    yield "rgba_some_unaligned", u8(p.quantize_rgba, odd, K, dither=True, tile_size=0, **kw)
    # the remaps, each mode under the knobs that steer it
    nearest, riemersma, ordered = ("nearest", False), ("riemersma", True), ("ordered", "ordered")
    knobs = (("", lambda: None, (nearest, riemersma, ordered)),
             ("_two_pass", lambda: L.patolette_amd_debug_remap_two_pass(1), (nearest, riemersma)),
             ("_lanes", lambda: L.patolette_amd_dither_layout(1), (riemersma,)),
             ("_wavefronts", lambda: L.patolette_amd_dither_layout(0), (riemersma,)),
             ("_nn1", lambda: L.patolette_amd_debug_nn_route(1), (nearest,)), ("_nn2", lambda: L.patolette_amd_debug_nn_route(2), (nearest,)),
             ("_nn3", lambda: L.patolette_amd_debug_nn_route(3), (nearest,)))

    def reset():
        L.patolette_amd_debug_remap_two_pass(0)
        L.patolette_amd_dither_layout(-1)
        L.patolette_amd_dither_config(0, -1)
        L.patolette_amd_debug_dither_stall_passes(-1)
        L.patolette_amd_debug_dither_solo_cap(-1)
        L.patolette_amd_debug_nn_route(0)

    def knobbed(set_knob, fn):
        def run():
            set_knob()
            try:
                return fn()
            finally:
                reset()
        return run

    for knob, set_knob, modes in knobs:
        for where, at in (("np", arrays), ("torch", tensors)):
            for mode, dither in modes:
                tag = "%s_%s%s" % (mode, where, knob)
                yield "remap_" + tag, knobbed(set_knob, u8(p.remap, at["img"], pal8, dither=dither))
                yield "remap_frames_" + tag, knobbed(set_knob, u8(p.remap, at["frames"], pal8, dither=dither))
                for kind in ("none", "some", "all"):
                    yield "remap_rgba_%s_%s" % (kind, tag), knobbed(set_knob, u8(p.remap_rgba, at["frames_" + kind], palrgba, dither=dither))
        if riemersma in modes and knob:
            yield "remap_rgba_unaligned" + knob, knobbed(set_knob, u8(p.remap_rgba, odd, palrgba, dither=True))
            yield "u8_np_dither" + knob, knobbed(set_knob, u8(p.quantize_u8, img, K, dither=True, tile_size=0, **kw))
            yield "rgba_some_np_dither" + knob, knobbed(set_knob, u8(p.quantize_rgba, arrays["img_some"], K, dither=True, tile_size=0, **kw))

    # the dither's routes at the size from which patolette_amd_dither_layout(1) selects the lane layout (65 536 pixels; the images
    # above are far below it, so their _lanes cases walk wavefronts): every driver of a Riemersma walk under each layout, the single
    # chain, and the lane walk that gives up at its first stalled pass and hands the image to the wavefront layout
    def route_knobs(layout, segments, warm, stall, cap):
        def set_knob():
            L.patolette_amd_dither_layout(layout)
            L.patolette_amd_dither_config(segments, warm)
            L.patolette_amd_debug_dither_stall_passes(stall)
            L.patolette_amd_debug_dither_solo_cap(cap)
        return set_knob

    def two_pass(fn):
        def run():
            L.patolette_amd_debug_remap_two_pass(1)
            return fn()                                            # (knobbed's reset puts it back)
        return run

    def quantize_at(w, h, src, **k):
        def run():
            r = p.quantize(w, h, src, K, **k)
            assert r[0], r[-1]
            return dict(pal=r[1], map=r[2])
        return run

    for knob, set_knob in (("lanes", route_knobs(1, 0, -1, -1, -1)), ("wavefronts", route_knobs(0, 0, -1, -1, -1)),
                           ("chain", route_knobs(-1, 1, -1, -1, -1)), ("gives_up", route_knobs(1, 0, 1, 0, 0))):
        for cs in ("sRGB", "CIELuv", "ICtCp"):
            yield "route_%s_quantize_%s" % (knob, cs), knobbed(set_knob, quantize_at(RW, RW, rcolors, dither=True, tile_size=0,
                                                                                     color_space=getattr(p, "ColorSpace_" + cs), **kw))
        for where, at in (("np", arrays), ("torch", tensors)):
            yield "route_%s_frames_%s" % (knob, where), knobbed(set_knob, u8(p.quantize_frames, at["rframes"], K, dither=True, tile_size=0, **kw))
            yield "route_%s_rgba_%s" % (knob, where), knobbed(set_knob, u8(p.quantize_rgba, at["rrgba"], K, dither=True, tile_size=0, **kw))
            yield "route_%s_remap_rgba_%s" % (knob, where), knobbed(set_knob, u8(p.remap_rgba, at["rrgba"], palrgba, dither=True))
            yield "route_%s_remap_%s" % (knob, where), knobbed(set_knob, u8(p.remap, at["rimg"], pal8, dither=True))
            yield "route_%s_remap_two_pass_%s" % (knob, where), knobbed(set_knob, two_pass(u8(p.remap, at["rimg"], pal8, dither=True)))
    # more than 256 palette rows: the generic loop of the wavefront layout
    yield "route_K300_u8_np", u8(p.quantize_u8, img, 300, dither=True, tile_size=0, **kw)

    # the chunked upload: the conversion behind the pieces
    def chunked(fn):
        def run():
            os.environ["PAMD_UPLOAD_CHUNK_MIN"] = "1000"
            try:
                return fn()
            finally:
                del os.environ["PAMD_UPLOAD_CHUNK_MIN"]
        return run

    yield "chunked_quantize_planar", chunked(quantize(np.asfortranarray(colors), dither=False, tile_size=0, weights=wts, **kw))
    yield "chunked_quantize_rows", chunked(quantize(np.ascontiguousarray(colors), dither=True, tile_size=512, **kw))
    yield "chunked_u8", chunked(u8(p.quantize_u8, img, K, dither=True, tile_size=512, **kw))
    yield "chunked_frames", chunked(u8(p.quantize_frames, frames, K, dither=True, tile_size=0, weights=fwts, **kw))
    yield "remap_rgba_unaligned", u8(p.remap_rgba, odd, palrgba, dither=True)
    for kind in ("none", "some", "all"):
        yield "chunked_rgba_" + kind, chunked(u8(p.quantize_rgba, arrays["img_" + kind], K, dither=True, tile_size=0, weights=wts, **kw))
    if large:
        for name, w, h, col, weights, k, kwl in large_cases():
            yield name, (lambda w=w, h=h, col=col, weights=weights, k=k, kwl=kwl:
                         dict(zip(("pal", "map"), p.quantize(w, h, col, k, dither=False, tile_size=0, weights=weights, **kwl)[1:3])))

    # two images on two engines at once (--enqueued sorts this call's list, as it sorts the chunked calls')
    def batch():
        res = p.quantize_u8_batch([img, image_u8(W, H, 3)], K, dither=True, tile_size=0, **kw)
        return {"img%d_out%d" % (i, j): v for i, r in enumerate(res) for j, v in enumerate(r[1:-1])}
    yield "batch_u8", batch


def dump(path, large):
    import torch   # noqa: F401  (before patolette_amd: patolette_amd/__init__.py says why)
    from patolette_amd import _native
    L = _native.lib()
    d_sep = L.patolette_amd_malloc(8 * 64)
    out, names = {}, []
    for name, fn in calls(large):
        assert L.patolette_amd_fill_weights(d_sep, 64, 1) == 0      # the separator --enqueued cuts at
        res = fn()
        st = _native.last_stats()
        names.append(name)
        for k, v in res.items():
            if v is not None:
                out["%s_%s" % (name, k)] = np.asarray(v)
        out[name + "_stats"] = np.array([int(st[c]) for c in COUNTERS], dtype=np.int64)
    L.patolette_amd_free(d_sep)
    out["call_names"] = np.array(names)
    np.savez(path, **out)
    print("%d calls, %d arrays -> %s" % (len(names), len(out) - 1, path))


def compare(a, b):
    a, b = np.load(a), np.load(b)
    ok = sorted(a.files) == sorted(b.files)
    if not ok:
        print("DIFFERS the set of arrays", sorted(set(a.files) ^ set(b.files)))
    for k in a.files:
        if k in b.files and not (a[k].shape == b[k].shape and np.array_equal(a[k], b[k])):
            ok = False
            print("DIFFERS", k, a[k].tolist() if k.endswith("_stats") else "", b[k].tolist() if k.endswith("_stats") else "")
    print("%d arrays of %d calls" % (len(a.files) - 1, len(a["call_names"])))
    print("ALL EQUAL" if ok else "MISMATCH")
    return ok


def enqueued(trace_dir, names):
    """The trace's kernels and copies (rocprofv3 --output-format rocpd: the csv has no copy sizes) in order of start, cut at the
    k_fill_weights launches."""
    import sqlite3
    events = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        db = sqlite3.connect(f)
        for start, name, gx, gy, gz in db.execute("select start, name, grid_x, grid_y, grid_z from kernels"):
            m = re.search(r"pamd::(\w+)", name)
            events.append((start, "%s grid %d,%d,%d" % (m.group(1) if m else name.split("(")[0], gx, gy, gz)))
        for start, name, size in db.execute("select start, name, size from memory_copies"):
            events.append((start, "copy %s %d bytes" % (name.replace("MEMORY_COPY_", ""), size)))
    events.sort()
    cut, cur = [], None
    for _, e in events:
        if e.startswith("k_fill_weights "):
            cur = []
            cut.append(cur)
        elif cur is not None:
            cur.append(e)
    names = list(np.load(names)["call_names"]) if names else ["call %d" % i for i in range(len(cut))]
    assert len(names) == len(cut), "the trace holds %d calls, the names are %d" % (len(cut), len(names))
    total = 0
    for name, ev in zip(names, cut):
        total += len(ev)
        # no order of start between streams: these lists are sorted (the lane layout builds its record grids on two side streams)
        two_streams = name.startswith(("batch", "chunked", "route_lanes_", "route_gives_up_"))
        if two_streams:
            ev = sorted(ev)
        print("== %s%s" % (name, " (sorted: its work runs on more than one stream)" if two_streams else ""))
        i = 0
        while i < len(ev):
            j = i
            while j < len(ev) and ev[j] == ev[i]:
                j += 1
            print("  %s%s" % (ev[i], " x %d" % (j - i) if j - i > 1 else ""))
            i = j
    print("== %d calls, %d events" % (len(cut), total))


def main():
    args = sys.argv[1:]
    if args[0] == "--compare":
        sys.exit(0 if compare(args[1], args[2]) else 1)
    if args[0] == "--enqueued":
        return enqueued(args[1], args[args.index("--names") + 1] if "--names" in args else None)
    dump(args[0], "--large" in args)


if __name__ == "__main__":
    main()
