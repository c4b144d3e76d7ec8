"""k_deflate_segments token for token: the device's parse against tests/deflate_model.py, its tables against the host's and against
what follows from the stream alone.

Everything is read from the bytes `png_deflate` returns, by tests/deflate_trace.py: one segment is one block, so block i of frame f is
segment i of that frame.  For every block of every case of tests/deflate_cases.py:
  * its tokens equal the model's for that segment;
  * (a) its bits, from its first to its last, equal the block the HOST writes for these tokens through the routines the kernel shares
    with it (patolette_amd_debug_deflate_block): the 64-lane tables, the emitter, the carry between emit steps, the join of blocks
    at every bit offset;
  * (b) the checks of tests/deflate_checks.py, made from the trace alone: lengths within 15 and 7, Kraft sums of exactly 1, the
    Huffman cost wherever Huffman's tree fits, HLIT, HDIST and HCLEN trimmed, the run-length coding deflate_codes.h specifies, the
    cheaper block type with ties to the fixed one;
  * (c) BFINAL on the frame's last block and on no other.
tests/test_deflate_model.py proves without a GPU that the model reaches every edge on these inputs and that each single-rule
mutation of it changes some tokens here, so a pass cannot come from never getting there.  tests/test_gpu_png.py stays the decoder's
oracle; check_streams is run here too."""
import numpy as np
import pytest

import patolette_amd
from tests import deflate_cases as cases
from tests import deflate_checks as checks
from tests import deflate_trace as dt
from tests import png_ref

pytestmark = pytest.mark.gpu


def _frames(name, segment):
    """[(the frame's stream bytes, its traced blocks)] of one png_deflate call"""
    maps, rects, _ = cases.cases()[name]
    ok, data, offsets, adler, msg = patolette_amd.png_deflate(maps, rects, segment)
    assert ok, msg
    png_ref.check_streams(maps, rects, data, offsets, adler)
    out = []
    for f in range(maps.shape[0]):
        stream = data[int(offsets[f]):int(offsets[f + 1])].tobytes()
        out.append((stream, dt.trace(stream)))
    return out


def _first_difference(got, want):
    at = 0
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "token %d at byte %d: the device %r, the model %r" % (i, at, g, w)
        at += g[0] if isinstance(g, tuple) else 1
    return "%d tokens, the model %d" % (len(got), len(want))


@pytest.mark.parametrize("name,segment", cases.runs())
def test_tokens_tables_and_flags(gpu, native, name, segment):
    kinds, starts = set(), set()
    for f, ((stream, blocks), (tokens, _)) in enumerate(zip(_frames(name, segment), cases.model(name, segment))):
        assert len(blocks) == len(tokens), "frame %d: %d blocks for %d segments" % (f, len(blocks), len(tokens))
        for k, (blk, want) in enumerate(zip(blocks, tokens)):
            where = "%s, segment %s, frame %d, block %d" % (name, segment, f, k)
            assert blk["tokens"] == want, "%s: %s" % (where, _first_difference(blk["tokens"], want))
            last = k == len(blocks) - 1
            assert blk["bfinal"] == (1 if last else 0), where                                          # (c)
            bits, host = checks.host_block(native, blk["tokens"], last)                                # (a)
            assert blk["end"] - blk["start"] == bits, where
            assert dt.bit_slice(stream, blk["start"], blk["end"]) == int.from_bytes(host, "little"), where
            kinds.add(checks.check_block(blk))                                                         # (b)
            starts.add(blk["start"] & 7)
    if name == "noise8" and segment is None:
        assert kinds == {"dynamic"}
    if name == "lengths" and segment == 3:
        assert kinds == {"fixed"}
    if name == "endings":
        assert starts == set(range(8)), "blocks start at every bit of a byte"


def test_a_frame_of_three_equal_ones_is_coded_as_alone(gpu):
    """Three identical frames in one call: every frame's bytes are those of the frame coded alone -- frame 1's first positions find
    nothing in frame 0, which lies right before it in the workspace."""
    maps, _, segments = cases.cases()["three_frames"]
    for segment in segments:
        ok, data, offsets, adler, msg = patolette_amd.png_deflate(maps, None, segment)
        assert ok, msg
        ok, one, _, adler1, msg = patolette_amd.png_deflate(maps[:1], None, segment)
        assert ok, msg
        for f in range(3):
            assert data[int(offsets[f]):int(offsets[f + 1])].tobytes() == one.tobytes() and adler[f] == adler1[0], (segment, f)
        blocks = dt.trace(one.tobytes())
        assert not isinstance(blocks[0]["tokens"][0], tuple) and not isinstance(blocks[0]["tokens"][1], tuple)
