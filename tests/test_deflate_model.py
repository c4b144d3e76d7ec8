"""The two oracles of tests/test_gpu_png_tokens.py, tested without a GPU.

  * tests/deflate_trace.py against zlib: streams zlib writes at levels 1, 6 and 9, with the fixed code and with dynamic blocks, trace to
    tokens that expand to the input, in blocks that lie end to end; what the tracer must reject, it rejects.
  * tests/deflate_model.py against itself: its tokens expand to the filtered stream, no match leaves its segment or its frame, the
    trace's counters equal a recount from the tokens.
  * the inputs (tests/deflate_cases.py): the MODEL ALONE reaches every edge they were built for -- conditions, not measurements --
    and every single-rule mutation of the model changes the tokens of at least one of them.
  * the host's blocks for the model's tokens (patolette_amd_debug_deflate_block: host code, no device) pass every check that the GPU
    test makes on the device's blocks, and hold the table edges."""
import zlib

import numpy as np
import pytest

from tests import deflate_cases as cases
from tests import deflate_checks as checks
from tests import deflate_model as model
from tests import deflate_trace as dt

RUNS = cases.runs()


def _text(n, seed=0):
    """compressible bytes: words of a small vocabulary, some noise between them"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9))).astype(np.uint8)) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 200))] + b" "
        if rng.random() < 0.05:
            out += bytes(rng.integers(0, 256, size=5).astype(np.uint8))
    return bytes(out[:n])


# ---------------------------------------------------------------- the tracer against zlib
@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("strategy", ["fixed", "dynamic"])
def test_the_tracer_reads_what_zlib_writes(level, strategy):
    for data in (_text(70000, level), _text(300, 7), b"a", b"abcabcabcabc" * 40, bytes(1000)):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_FIXED if strategy == "fixed" else zlib.Z_DEFAULT_STRATEGY)
        half = len(data) // 2
        stream = c.compress(data[:half]) + c.flush(zlib.Z_BLOCK) + c.compress(data[half:]) + c.flush()   # Z_BLOCK: a block ends, nothing stored
        blocks = dt.trace(stream)
        assert blocks[0]["start"] == 0 and all(a["end"] == b["start"] for a, b in zip(blocks, blocks[1:]))
        assert 8 * len(stream) - 8 < blocks[-1]["end"] <= 8 * len(stream)
        assert [b["bfinal"] for b in blocks] == [0] * (len(blocks) - 1) + [1]
        kinds = {b["btype"] for b in blocks}
        assert kinds == {1} if strategy == "fixed" else kinds <= {1, 2}
        if strategy == "dynamic" and len(data) == 70000:
            assert 2 in kinds
        out = bytearray()
        for b in blocks:
            dt.expand(b["tokens"], out)
            for t in b["tokens"]:
                assert 0 <= t <= 255 if not isinstance(t, tuple) else 3 <= t[0] <= 258 and 1 <= t[1] <= 32768
            if b["btype"] == 2:
                assert len(b["lit_lens"]) == b["hlit"] and len(b["dist_lens"]) == b["hdist"] and len(b["cl_sent"]) == b["hclen"]
                lens = []
                for s, e in b["rle"]:                                   # the run-length symbols give the two tables back
                    lens += [s] if s < 16 else [lens[-1]] * (3 + e) if s == 16 else [0] * ((3 if s == 17 else 11) + e)
                assert lens == b["lit_lens"] + b["dist_lens"]
        assert bytes(out) == data
        if len(data) == 70000:
            assert len(blocks) >= 2


def test_the_tracer_rejects_what_zlib_rejects_and_what_the_coder_never_writes():
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    good = c.compress(_text(2000)) + c.flush()
    blocks = dt.trace(good)
    assert blocks[-1]["end"] & 7, "the case needs padding bits"
    for bad, what in ((good[:-1], "stops"), (good + b"\0", "behind"), (good[:-1] + bytes([good[-1] | 0x80]), "padding"),
                      (bytes([0b111]), "reserved"), (bytes([0b011]), "stops")):
        with pytest.raises(dt.DeflateError, match=what):
            dt.trace(bad)
        d = zlib.decompressobj(-15)
        try:
            d.decompress(bad)
            assert not d.eof or d.unused_data or what == "padding"      # (zlib ignores the padding bits: the coder's contract does not)
        except zlib.error:
            pass
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    with pytest.raises(dt.DeflateError, match="stored"):
        dt.trace(c.compress(b"stored") + c.flush())
    # a dynamic header, bit by bit: HLIT 257, HDIST 1, HCLEN 4, then code-length codes that cannot be
    def header(cl4, rest=()):
        bits = [1, 0, 1] + [0] * 5 + [0] * 5 + [0] * 4
        for l in cl4:
            bits += [(l >> i) & 1 for i in range(3)]
        bits += list(rest)
        bits += [0] * (-len(bits) % 8 + 64)
        return bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))
    with pytest.raises(dt.DeflateError, match="over-subscribed"):
        dt.trace(header((1, 1, 1, 0)))
    with pytest.raises(dt.DeflateError, match="incomplete"):
        dt.trace(header((1, 0, 0, 0)))
    with pytest.raises(dt.DeflateError, match="no length before"):
        dt.trace(header((1, 0, 1, 0), (0,)))                            # symbols 16 and 18 with one bit each; the first one sent is a 16
    for bad in (header((1, 1, 1, 0)), header((1, 0, 0, 0)), header((1, 0, 1, 0), (0,))):
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(bad)


# ---------------------------------------------------------------- the model against itself
def _segments(name, segment):
    """(frame, segment index, q0, the segment's bytes, tokens, trace) of a run"""
    seg = cases.DEFAULT_SEGMENT if segment is None else segment
    for f, ((tokens, traces), (stream, R)) in enumerate(zip(cases.model(name, segment), cases.frames_of(name))):
        assert len(tokens) == len(traces) == -(-len(stream) // seg)
        for k, (toks, tr) in enumerate(zip(tokens, traces)):
            yield f, k, k * seg, stream[k * seg:(k + 1) * seg], toks, tr


@pytest.mark.parametrize("name,segment", RUNS)
def test_the_model_is_consistent_with_itself(name, segment):
    for (stream, R), (tokens, _) in zip(cases.frames_of(name), cases.model(name, segment)):
        out = bytearray()
        for toks in tokens:
            dt.expand(toks, out)
        assert bytes(out) == stream
        assert len(stream) <= 72000, "a frame of the GPU cases stays small"
    for f, k, q0, part, toks, tr in _segments(name, segment):
        at, matches, prev = 0, [], None
        for t in toks:
            if isinstance(t, tuple):
                assert 3 <= t[0] <= 258 and 1 <= t[1] <= min(q0 + at, 32768), "a match starts before its frame or window"
                assert not (t[0] == 3 and t[1] > 4096)
                matches.append((at, t[0], t[1], isinstance(prev, tuple) and prev[0] == 258))
            at += t[0] if isinstance(t, tuple) else 1
            assert at <= len(part), "a match crosses the end of its segment"
            prev = t
        assert at == len(part)
        assert tr["longest_match"] == max([m[1] for m in matches], default=0)
        assert tr["longest_distance"] == max([m[2] for m in matches], default=0)
        assert tr["before_segment"] == sum(1 for p, l, d, _ in matches if d > p)
        assert tr["distance_32768"] == sum(1 for p, l, d, _ in matches if d == 32768)
        assert tr["ends_at_last_byte"] == sum(1 for p, l, d, _ in matches if p + l == len(part))
        assert tr["three_at_4096"] == sum(1 for p, l, d, _ in matches if (l, d) == (3, 4096))
        assert tr["match_258_then_match"] == sum(1 for m in matches if m[3])
        assert sum(tr["winners"].values()) == len(matches) and tr["hash_won"] == tr["winners"]["hash"]
        assert tr["skipped_steps"] == sum(1 for b0 in range(0, len(part), 64)          # steps with no token start
                                          if not any(b0 <= p < b0 + 64 for p in _starts(toks)))
        assert tr["explored"] == sum(tr["rotation"].values()) <= tr["explorations"] == len(tr["explore_log"])
        assert tr["longest_wait"] == max(tr["waits_served"], default=0)


def _starts(tokens):
    at = 0
    for t in tokens:
        yield at
        at += t[0] if isinstance(t, tuple) else 1


# ---------------------------------------------------------------- the edges, reached by the model alone
def _traces(name, segments=None):
    maps, rects, segs = cases.cases()[name]
    return [tr for s in (segs if segments is None else segments) for _, _, _, _, _, tr in _segments(name, s)]


def _sum(name, key, segments=None):
    return sum(tr[key] for tr in _traces(name, segments))


def _runs_of(waits, value):
    best = run = 0
    for w in waits:
        run = run + 1 if w == value else 0
        best = max(best, run)
    return best


def test_edges_lengths():
    assert _sum("flat", "match_258_then_match") > 0
    assert _sum("equal_rows", "ends_at_last_byte") > 0
    segs = {k: (part, toks) for f, k, q0, part, toks, tr in _segments("equal_rows", 100)}
    part, toks = segs[10]                                               # a three-byte match on the segment's last three bytes: the last keyed position
    assert toks[-1] == (3, 301) and not isinstance(toks[-2], tuple)
    part, toks = segs[12]                                               # the last two bytes repeat the row above and are literals all the same
    stream = cases.frames_of("equal_rows")[0][0]
    assert toks[-2:] == [part[-2], part[-1]] and stream[1298:1300] == stream[1298 - 301:1300 - 301] and not isinstance(toks[-3], tuple)
    assert cases.cases()["lengths"][2] == (1, 2, 3, 63, 64, 65) and len(cases.frames_of("lengths")[0][0]) == 65
    last = [part for f, k, q0, part, toks, tr in _segments("lengths", 64)][-1]
    assert len(last) == 1                                               # a one-byte last segment


def test_edges_window():
    for segment in (32768, None):
        assert _sum("window32768", "distance_32768", (segment,)) > 0
        assert max(tr["longest_distance"] for tr in _traces("window32769", (segment,))) <= 32768
    stream = cases.frames_of("window32769")[0][0]
    assert stream[32769:] == stream[:len(stream) - 32769] and stream[32768:33768] != stream[:1000]
    stream = cases.frames_of("window32768")[0][0]
    assert stream[32768:] == stream[:len(stream) - 32768]


def test_edges_before_the_segment_never_before_the_frame():
    for f, k, q0, part, toks, tr in _segments("equal_rows", 100):
        if q0 >= 400:                                                   # from the second row's second segment on
            assert isinstance(toks[0], tuple) and toks[0][1] in (301, 602)         # position 0: any distance lies before the segment
    assert cases.cases()["equal_rows"][2] == (100,) and cases.frames_of("equal_rows")[0][1] == 301
    alone = cases.model("equal_rows", 100)[0][0]
    for segment in (100, None):
        frames = cases.model("three_frames", segment)
        assert len(frames) == 3 and frames[0][0] == frames[1][0] == frames[2][0]
    assert cases.model("three_frames", 100)[1][0] == alone
    assert not isinstance(alone[0][0], tuple) and not isinstance(alone[0][1], tuple)


def test_edges_candidates():
    assert [r[2] for r in cases.cases()["widths"][1].tolist()] == [1, 2, 3, 6, 7, 8, 9]
    for name in ("R-1", "R+1", "2R", "4R", "8R"):
        assert sum(tr["sole"][name] for tr in _traces("candidates")) > 0, name
    for name in model.FIXED:
        assert sum(tr["sole"][name] for tr in _traces("widths") + _traces("two_valued")) > 0, name
    assert _sum("two_valued", "tie_far") > 0 and _sum("widths", "tie_far") > 0


def test_edges_hash():
    for key in ("slot_collisions", "unseen_same_step", "key_in_skipped_step", "hash_won"):
        assert _sum("words", key) > 0, key


def test_edges_walk():
    assert _sum("two_valued", "lazy") > 0 and _sum("two_valued", "no_look_across_steps") > 0
    covers = [t[0] for f, k, q0, part, toks, tr in _segments("flat", None) for t in toks if isinstance(t, tuple)]
    assert max(covers) > 128 and _sum("flat", "skipped_steps") > 0
    covers = [t[0] for f, k, q0, part, toks, tr in _segments("equal_rows", 100) for t in toks if isinstance(t, tuple)]
    assert any(64 < c <= 128 for c in covers)
    assert _sum("far3_at_4096", "three_at_4096") > 0 and _sum("far3_beyond", "far_dropped") > 0
    assert cases.frames_of("far3_beyond")[0][1] * 8 > 4096 and _sum("far3_beyond", "three_at_4096") == 0


def test_edges_explorations():
    rotation = {k: sum(tr["rotation"][k] for tr in _traces("bayer") + _traces("words")) for k in ("rep0", "rep1", "rep2", "new")}
    assert all(rotation.values()), rotation
    assert max(_runs_of(tr["waits_served"], 15) for tr in _traces("explore")) >= 2
    logs = [tr["explore_log"] for tr in _traces("words")]
    assert max(tr["success_after_failures"] for tr in _traces("words")) >= 2
    # a success after two and more failures, and the next failure is the schedule's first again: it waits 1
    assert any(log[i][1] >= 8 and log[i][3] >= 2 and any(e[1] < 8 and e[3] == 0 for e in log[i + 1:]) for log in logs for i in range(len(log)))
    assert _sum("endings", "short_anchor") > 0
    far = [tr["longest_distance"] for tr in _traces("bayer")]
    assert max(far) > 8 * cases.frames_of("bayer")[0][1], "the dither's far distances, beyond 8 rows"
    assert sum(tr["winners"][r] for tr in _traces("bayer") for r in ("rep0", "rep1", "rep2", "rep3")) > 0


# ---------------------------------------------------------------- the mutations
# where to look first (any input may tell a mutation apart; these are the ones built for it)
FIRST = {"tie_nearest": "two_valued", "hash_after_insert": "words", "hash_first_wins": "words", "hash_skipped_steps": "words",
         "lazy_off": "two_valued", "lazy_across_steps": "two_valued", "far_4095": "far3_at_4096", "reach_in_segment": "equal_rows",
         "reach_32767": "window32768", "max_257": "flat", "explore_tokens_1": "bayer", "explore_tokens_3": "bayer", "explore_min_7": "bayer",
         "wait_1_2_4_8": "explore", "rotate_push_only": "bayer", "no_R-1": "candidates", "no_R+1": "candidates", "no_2R": "candidates",
         "no_4R": "candidates", "no_8R": "candidates", "no_R": "equal_rows"}


@pytest.mark.parametrize("mutation", list(model.MUTATIONS))
def test_every_mutation_changes_some_tokens(mutation):
    first = FIRST.get(mutation, "widths")
    for name, segment in sorted(RUNS, key=lambda r: r[0] != first):
        true = [t for t, _ in cases.model(name, segment)]
        if [t for t, _ in cases.model(name, segment, mutation)] != true:
            return
    raise AssertionError("no input tells '%s' (%s) from the true rules" % (mutation, model.MUTATIONS[mutation]))


# ---------------------------------------------------------------- the host's blocks for the model's tokens
def test_the_hosts_blocks_pass_the_checks_and_hold_the_table_edges(native):
    kinds, no_distance, one_distance, one_literal, starts = set(), 0, 0, 0, set()
    for name, segment in RUNS:
        for f, (tokens, _) in enumerate(cases.model(name, segment)):
            at = 0
            for k, toks in enumerate(tokens):
                bits, data = checks.host_block(native, toks, True)
                if name == "endings":
                    starts.add(at & 7)
                at += bits
                blocks = dt.trace(data, 32768)
                assert len(blocks) == 1 and blocks[0]["tokens"] == toks and blocks[0]["end"] == bits
                kind = checks.check_block(blocks[0])
                kinds.add(kind)
                lit, dist, _ = checks.histograms(toks)
                if kind == "dynamic":
                    no_distance += not any(dist)
                    one_distance += sum(1 for d in dist if d) == 1
                one_literal += sum(1 for v in lit[:256] if v) == 1 and not any(lit[257:])
    assert kinds == {"fixed", "dynamic"}
    assert no_distance and one_distance and one_literal
    assert starts == set(range(8)), "the blocks of `endings` start at every bit of a byte"
    kinds = {checks.check_block(dt.trace(checks.host_block(native, toks, True)[1], 32768)[0]) for toks in cases.model("noise8", None)[0][0]}
    assert kinds == {"dynamic"}                                         # noise at 8 bits
    kinds = {checks.check_block(dt.trace(checks.host_block(native, toks, True)[1], 32768)[0]) for toks in cases.model("lengths", 3)[0][0]}
    assert kinds == {"fixed"}                                           # tiny segments


def test_a_fibonacci_histogram_meets_the_length_limit(native):
    """The second segment of `fibonacci`: Huffman's tree for its literal/length histogram is 16 deep, so the code the host writes is the
    limited one -- 15 bits at the most, complete, and dearer than Huffman's."""
    R = cases.frames_of("fibonacci")[0][1]
    assert cases.cases()["fibonacci"][2] == (R,)
    toks = cases.model("fibonacci", R)[0][0][1]
    lit, dist, _ = checks.histograms(toks)
    assert sorted(v for v in lit if v) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 2581]
    cost, depth = checks.huffman(lit)
    assert depth == 16
    blk = dt.trace(checks.host_block(native, toks, True)[1], 32768)[0]
    assert checks.check_block(blk) == "dynamic" and max(blk["lit_lens"]) == 15
    assert sum(f * l for f, l in zip(lit, blk["lit_lens"])) > cost


def test_the_export_checks_its_arguments(native):
    import ctypes as C
    L = native.lib()
    bits = C.c_uint64(7)
    out = np.zeros(16, dtype=np.uint8)
    one = np.array([65], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))              # noqa: E731
    assert L.patolette_amd_debug_deflate_block(p(one), 1, 1, out.ctypes.data_as(C.c_void_p), 16, None) == -1
    assert L.patolette_amd_debug_deflate_block(None, 1, 1, out.ctypes.data_as(C.c_void_p), 16, C.byref(bits)) == -1
    for bad in (256, 0x80008000, 0x81000000):
        assert L.patolette_amd_debug_deflate_block(p(np.array([bad], dtype=np.uint32)), 1, 1, out.ctypes.data_as(C.c_void_p), 16, C.byref(bits)) == -1
    assert L.patolette_amd_debug_deflate_block(p(one), 1, 1, out.ctypes.data_as(C.c_void_p), 2, C.byref(bits)) == -1 and bits.value == 18
    assert L.patolette_amd_debug_deflate_block(p(one), 1, 1, out.ctypes.data_as(C.c_void_p), 3, C.byref(bits)) == 0 and bits.value == 18
    assert dt.trace(out[:3].tobytes())[0]["tokens"] == [65]
    assert L.patolette_amd_debug_deflate_block(None, 0, 0, out.ctypes.data_as(C.c_void_p), 16, C.byref(bits)) == 0 and bits.value == 10
