"""A tracing inflater for raw deflate streams, written from RFC 1951.  It shares no code with csrc/deflate_codes.h.

`trace(data)` decodes one complete stream and returns what every block said, not only what it expands to: where it starts and ends
(in bits), BFINAL and BTYPE, a dynamic block's header field by field -- HLIT, HDIST, HCLEN, the code-length code's lengths as sent,
the run-length symbols with their extra values, the two tables of code lengths -- and the tokens: an int for a literal, a
(length, distance) pair for a match.  It raises DeflateError on everything zlib's inflate rejects (the reserved block type, counts
beyond 286 / 30, a repeat without a previous length or beyond the tables, no end-of-block code, over-subscribed and incomplete codes
other than a single code of one bit, unused symbols in the stream, a distance beyond the output or the window, a stream that stops
early, bytes behind the stream), and also on what png_deflate never writes: a stored block, and padding bits behind the final block
that are not zero."""

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)                 # RFC 1951, 3.2.7
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                                   # 3.2.6; 286 and 287 never occur in data
FIXED_DIST_LENS = [5] * 32
WINDOW = 32768


class DeflateError(ValueError):
    pass


class _Bits:
    """The stream's bits, least significant bit of every byte first (3.1.1)."""

    def __init__(self, data):
        self.data, self.pos = bytes(data), 0

    def bit(self):
        byte = self.pos >> 3
        if byte >= len(self.data):
            raise DeflateError("the stream stops at bit %d" % self.pos)
        b = (self.data[byte] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def bits(self, n):                                                  # a value of n bits, its least significant bit first
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v


def _code(lens, what, allow_single):
    """{(length, code): symbol} of the canonical code of `lens` (3.2.2); the completeness rules are zlib's."""
    count = [0] * 16
    for l in lens:
        if not 0 <= l <= 15:
            raise DeflateError("%s: a code length of %d" % (what, l))
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise DeflateError("%s: over-subscribed code" % what)
    used = sum(count)
    if left > 0 and used > 0 and not (allow_single and used == 1 and count[1] == 1):
        raise DeflateError("%s: incomplete code" % what)
    next_code, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        next_code[l] = code
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(l, next_code[l])] = s
            next_code[l] += 1
    return table


def _symbol(rd, table, what):
    code = 0
    for l in range(1, 16):
        code = code << 1 | rd.bit()                                     # Huffman codes arrive most significant bit first
        s = table.get((l, code))
        if s is not None:
            return s
    raise DeflateError("%s: bits at %d are no code" % (what, rd.pos))


_FIXED = None


def trace(data, history=0):
    """The blocks of one raw deflate stream, in order: dicts with start, bfinal, btype, tokens, end and, for btype 2, hlit, hdist,
    hclen, cl_sent (the hclen lengths in the header's order), rle [(symbol, extra value or None)], lit_lens [hlit], dist_lens [hdist].
    `history`: bytes that lie before the stream's first, as behind a preset dictionary (a block traced on its own)."""
    global _FIXED
    rd = _Bits(data)
    blocks, produced = [], history
    while True:
        blk = dict(start=rd.pos, bfinal=rd.bit(), btype=rd.bits(2))
        if blk["btype"] == 0:
            raise DeflateError("a stored block at bit %d" % blk["start"])
        if blk["btype"] == 3:
            raise DeflateError("the reserved block type at bit %d" % blk["start"])
        if blk["btype"] == 1:
            if _FIXED is None:
                _FIXED = (_code(FIXED_LIT_LENS, "fixed literal/length", False), _code(FIXED_DIST_LENS, "fixed distance", False))
            lit, dist = _FIXED
        else:
            hlit, hdist, hclen = rd.bits(5) + 257, rd.bits(5) + 1, rd.bits(4) + 4
            if hlit > 286 or hdist > 30:
                raise DeflateError("HLIT %d, HDIST %d" % (hlit, hdist))
            sent = [rd.bits(3) for _ in range(hclen)]
            cl_lens = [0] * 19
            for i, l in enumerate(sent):
                cl_lens[CL_ORDER[i]] = l
            cl = _code(cl_lens, "code-length code", False)
            lens, rle = [], []
            while len(lens) < hlit + hdist:
                s = _symbol(rd, cl, "code-length code")
                if s < 16:
                    rle.append((s, None))
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise DeflateError("a repeat with no length before it")
                    extra = rd.bits(2)
                    value, n = lens[-1], 3 + extra
                elif s == 17:
                    extra = rd.bits(3)
                    value, n = 0, 3 + extra
                else:
                    extra = rd.bits(7)
                    value, n = 0, 11 + extra
                rle.append((s, extra))
                if len(lens) + n > hlit + hdist:
                    raise DeflateError("a repeat runs beyond the tables")
                lens += [value] * n
            if lens[256] == 0:
                raise DeflateError("no end-of-block code")
            blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_sent=sent, rle=rle, lit_lens=lens[:hlit], dist_lens=lens[hlit:])
            lit = _code(blk["lit_lens"], "literal/length code", True)
            dist = _code(blk["dist_lens"], "distance code", True)
        tokens = []
        while True:
            s = _symbol(rd, lit, "literal/length code")
            if s < 256:
                tokens.append(s)
                produced += 1
            elif s == 256:
                break
            else:
                if s > 285:
                    raise DeflateError("length symbol %d" % s)
                length = LENGTH_BASE[s - 257] + rd.bits(LENGTH_EXTRA[s - 257])
                d = _symbol(rd, dist, "distance code")
                if d > 29:
                    raise DeflateError("distance symbol %d" % d)
                distance = DIST_BASE[d] + rd.bits(DIST_EXTRA[d])
                if distance > produced or distance > WINDOW:
                    raise DeflateError("distance %d after %d bytes" % (distance, produced - history))
                tokens.append((length, distance))
                produced += length
        blk["tokens"], blk["end"] = tokens, rd.pos
        blocks.append(blk)
        if blk["bfinal"]:
            break
    while rd.pos & 7:
        if rd.bit():
            raise DeflateError("a padding bit behind the final block is set")
    if rd.pos >> 3 != len(rd.data):
        raise DeflateError("%d bytes behind the stream" % (len(rd.data) - (rd.pos >> 3)))
    return blocks


def expand(tokens, out=None):
    """The bytes a token list stands for, appended to the bytearray `out` (the bytes before it: what distances may reach into)."""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, tuple):
            length, distance = t
            assert 1 <= distance <= len(out)
            for _ in range(length):                                     # byte by byte: a match may overlap itself
                out.append(out[-distance])
        else:
            out.append(t)
    return out


def bit_slice(data, start, end):
    """Bits [start, end) of a byte string as an int, the first bit its least significant."""
    whole = int.from_bytes(bytes(data[start >> 3:(end + 7) >> 3]), "little")
    return (whole >> (start & 7)) & ((1 << (end - start)) - 1)
