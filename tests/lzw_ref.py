"""Reference of gif_lzw / patolette_amd_gif_lzw and of write_gif, in plain Python / numpy (test infrastructure).

`encode` is the normative statement of the contract in include/patolette_amd.h: the GIF flavour of LZW over a frame's symbols cut
into segments that are compressed independently, each ending in a Clear code, the bit strings put end to end.

`decode` is NOT derived from it: it is a GIF decoder written from the GIF89a specification (appendix F) the way decoders are -- it
builds its table one code behind the encoder (an entry is made when the NEXT code arrives: the previous string plus the first symbol
of the current one), so its width rule reads the other way round: after an entry is made and the next free code reaches 2^width,
the width grows, up to 12.  It knows nothing of segments: a Clear resets it, wherever it comes from.

`parse_gif` reads a GIF89a container: per frame the rectangle, the graphic control fields and the raw LZW stream (sub-blocks joined).
`composite` replays parsed and decoded frames on a canvas the way a viewer does with disposal 1."""
import numpy as np

DEFAULT_SEGMENT = 8192


class BitWriter:
    """Codes packed least-significant bit first."""

    def __init__(self):
        self.acc, self.nbits, self.out = 0, 0, bytearray()

    def put(self, code, width):
        assert 0 <= code < (1 << width)
        self.acc |= code << self.nbits
        self.nbits += width
        while self.nbits >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.nbits -= 8

    def bits(self):
        return 8 * len(self.out) + self.nbits

    def done(self):
        """The bytes, the last one padded with zero bits."""
        if self.nbits:
            self.out.append(self.acc & 255)
            self.acc, self.nbits = 0, 0
        return bytes(self.out)


def encode_segment(bw, symbols, m, closing, codes=None):
    """One segment of the contract into `bw`: an empty dictionary, greedy LZW, the pending prefix, the width step the decoder's entry
    on that code implies, then `closing` ("clear" or "eoi").  codes: a list that receives (code, width) of everything emitted."""
    clear, eoi = 1 << m, (1 << m) + 1

    def put(code, width):
        bw.put(code, width)
        if codes is not None:
            codes.append((code, width))

    table, free, width = {}, eoi + 1, m + 1
    prefix = int(symbols[0])
    assert 0 <= prefix < clear
    for byte in symbols[1:]:
        byte = int(byte)
        assert 0 <= byte < clear
        hit = table.get((prefix, byte))
        if hit is not None:
            prefix = hit
            continue
        put(prefix, width)
        if free < 4096:
            table[(prefix, byte)] = free
            if free == (1 << width) and width < 12:
                width += 1
            free += 1
        else:
            put(clear, width)
            table, free, width = {}, eoi + 1, m + 1
        prefix = byte
    put(prefix, width)
    if free < 4096 and free == (1 << width) and width < 12:
        width += 1
    put(clear if closing == "clear" else eoi, width)


def encode(symbols, m, segment=DEFAULT_SEGMENT, codes=None):
    """The stream of one frame: `symbols` (a 1-D sequence of integers below 2^m, at least one) -> bytes."""
    symbols = np.asarray(symbols).reshape(-1)
    assert symbols.size >= 1 and 2 <= m <= 8 and segment >= 1
    bw = BitWriter()
    bw.put(1 << m, m + 1)
    if codes is not None:
        codes.append((1 << m, m + 1))
    nseg = -(-symbols.size // segment)
    for k in range(nseg):
        encode_segment(bw, symbols[k * segment:(k + 1) * segment], m, "eoi" if k == nseg - 1 else "clear", codes)
    return bw.done()


def encode_frames(maps, rects=None, m=8, segment=DEFAULT_SEGMENT):
    """What gif_lzw returns for (F, H, W) maps: (data uint8, offsets (F + 1,) int64).  rects: None or (F, 4) rows (x0, y0, w, h), an
    empty one standing for (0, 0, 1, 1)."""
    maps = np.asarray(maps)
    if maps.ndim == 2:
        maps = maps[None]
    streams = []
    for f in range(maps.shape[0]):
        x0, y0, w, h = (0, 0, maps.shape[2], maps.shape[1]) if rects is None else (int(v) for v in rects[f])
        if w == 0 and h == 0:
            x0, y0, w, h = 0, 0, 1, 1
        streams.append(encode(maps[f, y0:y0 + h, x0:x0 + w].reshape(-1), m, segment))
    offsets = np.zeros(len(streams) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in streams])
    return np.frombuffer(b"".join(streams), dtype=np.uint8), offsets


def bound(area, segment=DEFAULT_SEGMENT):
    """The header's capacity bound for one frame, in bytes."""
    nseg = -(-area // segment)
    return (12 * (area + 2 * nseg + area // 3000 + 2) + 7) // 8


def decode(stream, m, count=None):
    """A GIF LZW decoder from the specification.  stream: the raw bytes (sub-blocks already joined); returns the symbols as a list.
    count: when given, the decoder must deliver exactly that many symbols and then meet the end code."""
    clear, eoi = 1 << m, (1 << m) + 1
    acc, nbits, pos = 0, 0, 0
    out = []
    table = {}                      # code -> tuple of symbols, for codes above eoi
    width, nxt, prev = m + 1, eoi + 1, None

    def string(code):
        return (code,) if code < clear else table[code]

    while True:
        while nbits < width:
            assert pos < len(stream), "the stream ends without an end code"
            acc |= stream[pos] << nbits
            nbits += 8
            pos += 1
        code = acc & ((1 << width) - 1)
        acc >>= width
        nbits -= width
        if code == clear:
            table, width, nxt, prev = {}, m + 1, eoi + 1, None
            continue
        if code == eoi:
            break
        if prev is None:                                   # the first code after a Clear: a plain symbol, no entry
            assert code < clear, "the first code after a Clear must be a symbol"
            out.extend(string(code))
            prev = code
            continue
        if code < clear or code in table:
            s = string(code)
            entry = string(prev) + (s[0],)
        else:                                              # the code the encoder has just made: previous string + its own first symbol
            assert code == nxt and nxt < 4096, "a code beyond the table"
            entry = string(prev) + (string(prev)[0],)
            s = entry
        if nxt < 4096:
            table[nxt] = entry
            nxt += 1
            if nxt == (1 << width) and width < 12:
                width += 1
        out.extend(s)
        prev = code
    assert pos == len(stream) and acc == 0, "bytes or set bits after the end code"
    if count is not None:
        assert len(out) == count, (len(out), count)
    return out


def wrap_gif(streams, rects, size, palette, m, transparent_index=None, delay_cs=4, loop=0, disposal=1):
    """The tests' own container around raw streams (not write_gif's code): GIF89a bytes.  size: (H, W); palette: (2^k, 3) uint8."""
    h, w = size
    palette = np.asarray(palette, dtype=np.uint8)
    k = int(palette.shape[0]).bit_length() - 1
    assert palette.shape == (1 << k, 3) and k >= 1
    u16 = lambda v: bytes([v & 255, v >> 8])
    out = bytearray(b"GIF89a" + u16(w) + u16(h) + bytes([0xF0 | (k - 1), 0, 0]) + palette.tobytes())
    if loop is not None:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + u16(loop) + b"\x00"
    for stream, (x0, y0, rw, rh) in zip(streams, rects):
        flag = 0 if transparent_index is None else 1
        out += b"\x21\xf9\x04" + bytes([disposal << 2 | flag]) + u16(delay_cs) + bytes([transparent_index or 0, 0])
        out += b"\x2c" + u16(int(x0)) + u16(int(y0)) + u16(int(rw)) + u16(int(rh)) + b"\x00" + bytes([m])
        stream = bytes(stream)
        for i in range(0, len(stream), 255):
            out += bytes([len(stream[i:i + 255])]) + stream[i:i + 255]
        out += b"\x00"
    out += b"\x3b"
    return bytes(out)


def parse_gif(blob):
    """A minimal GIF89a parser.  Returns (header dict: width, height, table (n, 3) uint8, loop or None;
    frames: list of dicts rect (x0, y0, w, h), disposal, transparent (index or None), delay_cs, m, stream bytes)."""
    assert blob[:6] == b"GIF89a"
    u16 = lambda p: blob[p] | blob[p + 1] << 8
    head = dict(width=u16(6), height=u16(8), loop=None, table=None)
    packed = blob[10]
    p = 13
    if packed & 0x80:
        n = 2 << (packed & 7)
        head["table"] = np.frombuffer(blob[p:p + 3 * n], dtype=np.uint8).reshape(n, 3).copy()
        p += 3 * n
    frames, gce = [], None

    def blocks(p):
        data = bytearray()
        while blob[p]:
            data += blob[p + 1:p + 1 + blob[p]]
            p += 1 + blob[p]
        return bytes(data), p + 1

    while True:
        kind = blob[p]
        if kind == 0x3B:
            assert p == len(blob) - 1, "bytes after the trailer"
            break
        if kind == 0x21:
            label = blob[p + 1]
            data, p = blocks(p + 2)
            if label == 0xF9:
                assert len(data) == 4
                gce = dict(disposal=(data[0] >> 2) & 7, transparent=data[3] if data[0] & 1 else None, delay_cs=data[1] | data[2] << 8)
            elif label == 0xFF and data[:11] == b"NETSCAPE2.0":
                assert data[11] == 1
                head["loop"] = data[12] | data[13] << 8
            continue
        assert kind == 0x2C, "neither an extension, an image nor the trailer"
        rect = (u16(p + 1), u16(p + 3), u16(p + 5), u16(p + 7))
        assert blob[p + 9] == 0, "local colour tables and interlace are out of scope"
        m = blob[p + 10]
        stream, p = blocks(p + 11)
        frame = dict(rect=rect, m=m, stream=stream)
        frame.update(gce or dict(disposal=0, transparent=None, delay_cs=0))
        frames.append(frame)
        gce = None
    return head, frames


def composite(head, frames):
    """Every frame's canvas of indices, (F, H, W) int64, as a viewer builds it with disposal 0 / 1 (leave in place): inside the
    rectangle every decoded index but the transparent one overwrites the canvas.  The canvas starts as -1 (nothing drawn)."""
    canvas = np.full((head["height"], head["width"]), -1, dtype=np.int64)
    out = []
    for fr in frames:
        assert fr["disposal"] in (0, 1)
        x0, y0, w, h = fr["rect"]
        idx = np.array(decode(fr["stream"], fr["m"], w * h), dtype=np.int64).reshape(h, w)
        part = canvas[y0:y0 + h, x0:x0 + w]
        keep = idx == fr["transparent"] if fr["transparent"] is not None else np.zeros_like(idx, dtype=bool)
        canvas[y0:y0 + h, x0:x0 + w] = np.where(keep, part, idx)
        out.append(canvas.copy())
    return np.stack(out)


def contents(kind, n, m, seed=0):
    """The tests' symbol sequences of length n below 2^m: "noise", "one" (a single value: one match runs on and on), "ramp" (period 7)."""
    top = 1 << m
    if kind == "noise":
        return np.random.default_rng(seed + 1000 * m + n).integers(0, top, size=n).astype(np.uint8)
    if kind == "one":
        return np.full(n, top - 1, dtype=np.uint8)
    assert kind == "ramp"
    return ((np.arange(n) % 7) % top).astype(np.uint8)
