"""tests/dither_ref.py without a GPU: the vectorised replay of the chain against the CPU oracle and against the step-by-step model of
tests/independent_ref.py, and the conditions the GPU suite (tests/test_gpu_dither_edges.py) rests on, which the reference alone must
satisfy: every reset between two probes holds, hardly a probe is dropped for lack of an anchor, and the images together meet every
class of query the dither's three searches tell apart.  Prints the counts."""
import numpy as np
import pytest

from tests import dither_ref as dr
from tests import independent_ref, nn_ref, util

FLOOR = 64                                                          # steps every class must hold
ALL = list(dict.fromkeys(dr.wave_cases() + dr.lane_cases() + dr.big_cases()))


@pytest.fixture(scope="module")
def cases(ob):
    return {name: dr.evaluated(ob, name) for name in ALL}


def test_replay_is_the_oracle_on_every_case(cases):
    for name, ev in cases.items():
        assert np.array_equal(ev.idx, ev.chain), name


def test_replay_is_the_step_by_step_model(ob):
    """one small image (40 x 24: not a power of two) of tie probes on the 64 lattice rows, through the serial model of independent_ref"""
    w, h = 40, 24
    order = ob.hilbert_order(w, h).astype(np.int64)
    probes, pal = dr.lattice_ties(64, (w * h - dr.RESET) // dr.STRIDE)
    lay = dr.layout(probes, pal, order, w, h)
    img = np.stack([lay.image[c * w * h:(c + 1) * w * h] for c in range(3)], axis=1)
    serial = independent_ref.dither(img, w, h, pal)
    assert np.array_equal(serial, ob.dither(lay.image, w, h, pal).astype(np.int64))
    q, idx, gap, ties = dr.replay(lay.seq, pal, serial[order])
    assert np.array_equal(idx, serial[order])
    assert int(np.sum(ties[lay.ranks] > 1)) >= 8


def test_resets_hold(cases):
    """every step that is no probe pushes exactly zero, and every probe's choice is the brute arg-min of the query meant for it"""
    for name, ev in cases.items():
        lay = ev.lay
        err = lay.seq - lay.pal[ev.chain]
        assert not np.any(err[~ev.probe] != 0), name
        meant = dr.KW * lay.seq[lay.ranks]
        assert np.array_equal(ev.q[lay.ranks], meant), name
        assert np.array_equal(nn_ref.brute(meant, lay.pal * dr.FW)[0], ev.chain[lay.ranks]), name


def test_hardly_a_probe_is_dropped(cases):
    for name, ev in cases.items():
        kept, dropped = ev.lay.ranks.shape[0], ev.lay.dropped.shape[0]
        print("%-20s probes %5d, without an anchor %4d (%.2f %%)" % (name, kept, dropped, 100.0 * dropped / (kept + dropped)))
        assert dropped <= 0.02 * (kept + dropped), name
        assert kept >= 1000, name


def test_every_class_of_query_is_met(cases):
    lane, wave = {}, {}
    f32_other = 0
    for name, ev in cases.items():
        k = ev.lay.pal.shape[0]
        palw = ev.lay.pal * dr.FW
        big = name.startswith("big-")
        sel = slice(None) if not big else np.concatenate([np.arange(70000 + dr.STRIDE), ev.lay.ranks[ev.lay.ranks > 70000]])
        q, gap, idx = ev.q[sel], ev.gap[sel], ev.idx[sel]
        if name in dr.lane_cases() or big:
            geo = dr.lane_geometry(ev.lay.pal, ev.order.shape[0])
            dr.level_classes(q, geo, lane)
            dr.gap_classes(gap, dr.query_margin(q, geo), lane)
            f32_other += dr.f32_names_another(q, palw, geo, idx)
        if name in dr.wave_cases():
            dr.tie_classes(q, palw, dr.per_of(k), wave)
            dr.low_word_classes(q, palw, wave)
    for group, counts in (("lane layout", lane), ("wavefront layout", wave)):
        for key in sorted(counts):
            print("%-18s %-32s %8d" % (group, key, counts[key]))
    print("f32 first pass names another row than f64 at %d steps" % f32_other)
    need = ["first-grid", "second-grid", "third-grid", "outside"] + ["on-%s-%d" % (s, g) for s in ("lo", "hi") for g in range(3)]
    need += ["gap-0-M/32", "gap-M/32-M", "gap-M-2M", "gap-2M-8M"]
    for key in need:
        assert lane.get(key, 0) >= FLOOR, (key, lane.get(key, 0))
    need = ["tie-2", "tie-4", "tie-8", "tie-50+", "per2-same-lane-01", "per2-same-row", "per2-other-row", "per4-same-row", "per4-other-row"]
    need += ["per4-same-lane-%d%d" % p for p in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))]
    need += ["low-word-higher-index-nearer", "low-word-lower-index-nearer"]
    for key in need:
        assert wave.get(key, 0) >= FLOOR, (key, wave.get(key, 0))
    assert f32_other >= 1


@pytest.mark.parametrize("variant", [v[0] for v in dr.NONFINITE])
def test_non_finite_pixels_in_the_oracle(ob, native, cases, variant):
    """what the GPU tests hold the kernels to: the replay (a NaN is never '<': index 0) is the oracle with such a pixel too; a pixel
    that is not finite takes index 0, and so do the sixteen steps behind it; seventeen steps of anchors later the chain is the clean one"""
    ev = cases["margin-64"]
    lay, order = ev.lay, ev.order
    places = dr.nonfinite_places(lay, util.dither_locate(native, lay.width, lay.height))
    image = dr.with_nonfinite(lay, order, variant, places)
    got = ob.dither(image, lay.width, lay.height, lay.pal).astype(np.int64)[order]
    seq = dr.to_sequence(image, order)
    assert np.array_equal(dr.replay(seq, lay.pal, got)[1], got)
    value = [v[2] for v in dr.NONFINITE if v[0] == variant][0]
    differs = np.nonzero(got != ev.chain)[0]
    print("%s: %d steps differ from the clean chain" % (variant, differs.size))
    if variant == "1e308-pair":                                     # both errors at the queue's heavy end (weights 0.83 and 1): the sum is +Inf
        qs = dr.queries(seq, lay.pal, got)
        assert np.isinf(qs[places[0] + 2, 0]) and np.all(np.isfinite(qs[places[0] + 18:places[0] + 30]))
    if not np.isfinite(value) or variant in ("1e200", "1e308-pair"):
        for p in places:
            assert np.all(got[p:p + 17] == 0)
    for d in differs:                                               # nothing beyond the next reset
        assert np.any((places <= d) & (d < places + 3 * dr.STRIDE)), (variant, d)
