"""What can be said about a deflate block from its trace alone (tests/deflate_trace.py), with no model of the coder: the checks of
tests/test_deflate_model.py (on the host's blocks) and tests/test_gpu_png_tokens.py (on the device's).  Python from RFC 1951 and the
comments of csrc/deflate_codes.h; a textbook heap Huffman for the costs."""
import ctypes as C
import heapq

import numpy as np

from tests import deflate_trace as dt


def pack(tokens):
    """the library's token words (include/patolette_amd.h, patolette_amd_debug_deflate_block) of a tracer's token list"""
    return np.array([0x80000000 | (t[0] - 3) << 16 | (t[1] - 1) if isinstance(t, tuple) else t for t in tokens], dtype=np.uint32)


def host_block(native, tokens, final):
    """(bits, bytes) of the block the HOST writes for the tokens: csrc/deflate_codes.h's write_block behind the library's export"""
    words = pack(tokens)
    bits = C.c_uint64(0)
    out = np.zeros(6 * (len(tokens) + 1) + 64, dtype=np.uint8)         # at most 48 bits a token, and a header
    rc = native.lib().patolette_amd_debug_deflate_block(words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size, 1 if final else 0,
                                                        out.ctypes.data_as(C.c_void_p), out.size, C.byref(bits))
    assert rc == 0, "patolette_amd_debug_deflate_block: %d, %d bits" % (rc, bits.value)
    return bits.value, out[:(bits.value + 7) // 8].tobytes()


def length_symbol(length):
    s = max(i for i, b in enumerate(dt.LENGTH_BASE) if b <= length)
    return 257 + s, dt.LENGTH_EXTRA[s]


def distance_symbol(distance):
    s = max(i for i, b in enumerate(dt.DIST_BASE) if b <= distance)
    return s, dt.DIST_EXTRA[s]


def histograms(tokens):
    """(literal/length counts [286] with the end of block, distance counts [30], extra bits in all)"""
    lit, dist, extra = [0] * 286, [0] * 30, 0
    for t in tokens:
        if isinstance(t, tuple):
            s, e = length_symbol(t[0])
            d, f = distance_symbol(t[1])
            lit[s] += 1
            dist[d] += 1
            extra += e + f
        else:
            lit[t] += 1
    lit[256] += 1
    return lit, dist, extra


def huffman(freq):
    """(cost in bits, depth) of a Huffman code for the used symbols of freq (two at least): the textbook heap, ties to the shallower
    subtree, which gives the least depth among the optimal trees."""
    heap = [(f, 0) for f in freq if f]
    assert len(heap) >= 2
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def kraft(lens, limit):
    return sum(1 << (limit - l) for l in lens if l)


def rle_of(lens):
    """csrc/deflate_codes.h's run-length coding: zeros -- an 18 for every 11 .. 138 of a run, then a 17 for 3 .. 10, else zeros; another
    length -- the length once, a 16 for every 3 .. 6 repeats, else the length again."""
    out, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, None))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
        out += [(v, None)] * run
    return out


def check_code(freq, lens, limit, what):
    """lengths within the limit, used exactly where counted; two and more used symbols: Kraft sum 1, the cost Huffman's wherever
    its tree fits the limit and never below; one: a single bit"""
    used = [s for s, f in enumerate(freq) if f]
    lens = list(lens) + [0] * (len(freq) - len(lens))
    assert all(0 <= l <= limit for l in lens), what
    assert all(lens[s] for s in used), "%s: a used symbol without a code" % what
    coded = [s for s, l in enumerate(lens) if l]
    if len(used) >= 2:
        assert coded == used, "%s: codes for unused symbols" % what
        assert kraft(lens, limit) == 1 << limit, "%s: Kraft sum" % what
        cost, depth = huffman(freq)
        mine = sum(freq[s] * lens[s] for s in used)
        assert mine >= cost, what
        if depth <= limit:
            assert mine == cost, "%s: %d bits, Huffman %d (depth %d)" % (what, mine, cost, depth)
    elif len(used) == 1:
        assert [lens[s] for s in used] == [1], what
    return lens


def fixed_bits(tokens):
    lit, dist, extra = histograms(tokens)
    return 3 + sum(f * dt.FIXED_LIT_LENS[s] for s, f in enumerate(lit)) + 5 * sum(dist) + extra


def check_block(blk):
    """the checks of a traced block that need no model of the parse; returns the block's kind, "fixed" or "dynamic" """
    lit, dist, extra = histograms(blk["tokens"])
    fix = fixed_bits(blk["tokens"])
    if blk["btype"] == 1:
        assert blk["end"] - blk["start"] == fix
        return "fixed"                                                  # (the dynamic block it was preferred to is not in the stream: check (a))
    hlit, hdist, hclen = blk["hlit"], blk["hdist"], blk["hclen"]
    assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and 4 <= hclen <= 19
    assert hlit == 257 or blk["lit_lens"][-1], "HLIT is not trimmed"
    assert hdist == 1 or blk["dist_lens"][-1], "HDIST is not trimmed"
    assert hclen == 4 or blk["cl_sent"][-1], "HCLEN is not minimal"
    lit_lens = check_code(lit, blk["lit_lens"], 15, "literal/length code")
    dist_lens = check_code(dist, blk["dist_lens"], 15, "distance code")
    if not any(dist):
        assert hdist == 1 and blk["dist_lens"] == [0]
    assert blk["rle"] == rle_of(blk["lit_lens"] + blk["dist_lens"]), "the run-length coding of the lengths"
    cl_freq = [0] * 19
    for s, _ in blk["rle"]:
        cl_freq[s] += 1
    cl_lens = [0] * 19
    for i, l in enumerate(blk["cl_sent"]):
        assert 0 <= l <= 7
        cl_lens[dt.CL_ORDER[i]] = l
    if sum(1 for f in cl_freq if f) >= 2:
        check_code(cl_freq, cl_lens, 7, "code-length code")
    else:                                                               # one symbol sent: a second is counted in, so the code is complete
        assert kraft(cl_lens, 7) == 1 << 7 and sorted(l for l in cl_lens if l) == [1, 1]
    header = 3 + 14 + 3 * hclen + sum(cl_lens[s] + (0 if e is None else {16: 2, 17: 3, 18: 7}[s]) for s, e in blk["rle"])
    body = sum(f * lit_lens[s] for s, f in enumerate(lit)) + sum(f * dist_lens[s] for s, f in enumerate(dist)) + extra
    assert blk["end"] - blk["start"] == header + body, "the block's bits against its header and lengths"
    assert header + body < fix, "a dynamic block of %d bits where the fixed one takes %d (ties go to fixed)" % (header + body, fix)
    return "dynamic"
