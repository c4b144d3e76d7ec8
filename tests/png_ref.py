"""A reader of indexed PNG and APNG files, written from the PNG (ISO/IEC 15948) and APNG 1.0 specifications, and a zlib-backed stand-in
for `png_deflate`.  It shares no code with the writer: chunks with every CRC verified, inflate by zlib, filter type 0 undone, and the
APNG compositor (dispose_op, blend_op, regions)."""
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
DISPOSE_NONE, DISPOSE_BACKGROUND, DISPOSE_PREVIOUS = 0, 1, 2
BLEND_SOURCE, BLEND_OVER = 0, 1


def chunks(blob):
    """[(type bytes, body bytes)] of a PNG datastream; every length, CRC and the signature are checked, IEND must end the file."""
    assert blob[:8] == SIGNATURE, "no PNG signature"
    out, p = [], 8
    while p < len(blob):
        n = int.from_bytes(blob[p:p + 4], "big")
        kind, body = blob[p + 4:p + 8], blob[p + 8:p + 8 + n]
        assert len(body) == n, "a chunk runs beyond the file"
        assert int.from_bytes(blob[p + 8 + n:p + 12 + n], "big") == zlib.crc32(kind + body), "CRC of %r" % kind
        out.append((kind, body))
        p += 12 + n
    assert out and out[0][0] == b"IHDR" and out[-1][0] == b"IEND" and out[-1][1] == b"", "IHDR first, an empty IEND last"
    assert [k for k, _ in out].count(b"IEND") == 1
    return out


def filtered(rows):
    """The filtered stream of (h, w) uint8 rows at depth 8 with filter type 0: every row behind a zero byte."""
    rows = np.asarray(rows, dtype=np.uint8)
    return np.concatenate([np.zeros((rows.shape[0], 1), dtype=np.uint8), rows], axis=1).tobytes()


def unfilter(stream, w, h):
    """(h, w) uint8 indices of a filtered stream whose every row has filter type 0."""
    assert len(stream) == h * (w + 1), "%d filtered bytes for %d x %d" % (len(stream), w, h)
    a = np.frombuffer(stream, dtype=np.uint8).reshape(h, w + 1)
    assert not a[:, 0].any(), "a filter type other than 0"
    return a[:, 1:].copy()


def inflate_zlib(data):
    """A zlib stream's bytes; header, Adler-32 and the end of the stream are checked (nothing may follow)."""
    assert data[:2] == b"\x78\x9c"
    d = zlib.decompressobj()
    out = d.decompress(data) + d.flush()
    assert d.eof and not d.unused_data, "the zlib stream does not end with its data"
    return out


def parse(blob):
    """An indexed PNG or APNG -> (head, frames).  head: width, height, palette (K, 3) uint8, alpha (K,) uint8 (255 where tRNS is
    silent), num_frames, num_plays (None for a plain PNG).  frames: dicts with rect (x0, y0, w, h), delay_num, delay_den, dispose_op,
    blend_op, sequence (the fcTL's), data_sequences (the fdATs'), indices (h, w) uint8; a plain PNG has one frame without the fcTL's fields."""
    cs = chunks(blob)
    ihdr = cs[0][1]
    assert len(ihdr) == 13
    width, height = int.from_bytes(ihdr[:4], "big"), int.from_bytes(ihdr[4:8], "big")
    assert tuple(ihdr[8:]) == (8, 3, 0, 0, 0), "depth 8, colour type 3, deflate, filter method 0, no interlace"
    head = dict(width=width, height=height, palette=None, alpha=None, num_frames=1, num_plays=None)
    frames, current, seen_idat, order = [], None, False, []
    for kind, body in cs[1:-1]:
        order.append(kind)
        if kind == b"PLTE":
            assert not seen_idat and len(body) % 3 == 0 and 1 <= len(body) // 3 <= 256
            head["palette"] = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3).copy()
            head["alpha"] = np.full(len(body) // 3, 255, dtype=np.uint8)
        elif kind == b"tRNS":
            assert head["palette"] is not None and not seen_idat and 1 <= len(body) <= head["palette"].shape[0]
            head["alpha"][:len(body)] = np.frombuffer(body, dtype=np.uint8)
        elif kind == b"acTL":
            assert not seen_idat and len(body) == 8
            head["num_frames"], head["num_plays"] = int.from_bytes(body[:4], "big"), int.from_bytes(body[4:], "big")
            assert head["num_frames"] >= 1
        elif kind == b"fcTL":
            assert len(body) == 26
            u32 = lambda p: int.from_bytes(body[p:p + 4], "big")
            current = dict(sequence=u32(0), rect=(u32(12), u32(16), u32(4), u32(8)), delay_num=int.from_bytes(body[20:22], "big"),
                           delay_den=int.from_bytes(body[22:24], "big"), dispose_op=body[24], blend_op=body[25], data=b"", data_sequences=[],
                           idat=False)
            x0, y0, w, h = current["rect"]
            assert w >= 1 and h >= 1 and x0 + w <= width and y0 + h <= height and current["dispose_op"] <= 2 and current["blend_op"] <= 1
            frames.append(current)
        elif kind == b"IDAT":
            assert head["palette"] is not None
            if not seen_idat:
                if current is None:                                     # a plain PNG, or an APNG whose default image is no frame
                    current = dict(rect=(0, 0, width, height), data=b"", data_sequences=[], idat=True)
                    frames.append(current)
                assert current["rect"] == (0, 0, width, height), "the default image's frame must cover the canvas"
                current["idat"] = True
            assert current["idat"], "IDAT chunks must be consecutive"
            seen_idat = True
            current["data"] += body
        elif kind == b"fdAT":
            assert seen_idat and current is not None and not current["idat"] and len(body) >= 4
            current["data_sequences"].append(int.from_bytes(body[:4], "big"))
            current["data"] += body[4:]
        else:
            raise AssertionError("unexpected chunk %r" % kind)
    assert seen_idat
    if head["num_plays"] is not None:
        assert len(frames) == head["num_frames"], "acTL's num_frames"
        numbers = []
        for fr in frames:
            numbers += [fr["sequence"]] + fr["data_sequences"]
        assert numbers == list(range(len(numbers))), "sequence numbers must count from 0 without gaps: %r" % numbers
        assert order.index(b"acTL") < order.index(b"IDAT") and order.index(b"fcTL") < order.index(b"IDAT")
    for fr in frames:
        x0, y0, w, h = fr["rect"]
        fr["stream"] = fr.pop("data")
        fr["indices"] = unfilter(inflate_zlib(fr["stream"]), w, h)
        assert int(fr["indices"].max()) < head["palette"].shape[0], "an index beyond PLTE"
    return head, frames


def composite(head, frames):
    """Every frame's output buffer as the APNG specification builds it, (F, H, W, 4) uint8 RGBA: the buffer starts fully transparent
    black; blend_op SOURCE replaces the region, OVER composites onto it; dispose_op then leaves the region, clears it to transparent
    black or puts back what it held before the frame (PREVIOUS on the first frame counts as BACKGROUND)."""
    table = np.concatenate([head["palette"], head["alpha"][:, None]], axis=1)
    canvas = np.zeros((head["height"], head["width"], 4), dtype=np.uint8)
    out = []
    for i, fr in enumerate(frames):
        x0, y0, w, h = fr["rect"]
        region = canvas[y0:y0 + h, x0:x0 + w]
        before = region.copy()
        src = table[fr["indices"]]
        if fr.get("blend_op", BLEND_SOURCE) == BLEND_SOURCE:
            region[...] = src
        else:
            a = src[..., 3:].astype(np.float64) / 255.0
            b = before[..., 3:].astype(np.float64) / 255.0
            oa = a + b * (1.0 - a)
            with np.errstate(divide="ignore", invalid="ignore"):
                rgb = np.where(oa > 0, (src[..., :3] * a + before[..., :3] * b * (1.0 - a)) / oa, 0.0)
            mixed = np.concatenate([np.round(rgb), np.round(oa * 255.0)], axis=2).astype(np.uint8)
            region[...] = np.where(src[..., 3:] == 255, src, np.where(src[..., 3:] == 0, before, mixed))
        out.append(canvas.copy())
        dispose = fr.get("dispose_op", DISPOSE_NONE)
        if dispose == DISPOSE_PREVIOUS and i == 0:
            dispose = DISPOSE_BACKGROUND
        if dispose == DISPOSE_BACKGROUND:
            region[...] = 0
        elif dispose == DISPOSE_PREVIOUS:
            region[...] = before
    return np.stack(out)


def composite_indices(head, frames):
    """The same buffers as palette indices, (F, H, W) int64, -1 where nothing opaque has been drawn: defined for palettes whose alpha is
    0 or 255 only -- what a GIF viewer's canvas of indices is (tests/lzw_ref.py, composite) with APNG's disposal on top."""
    assert np.all((head["alpha"] == 0) | (head["alpha"] == 255))
    canvas = np.full((head["height"], head["width"]), -1, dtype=np.int64)
    out = []
    for i, fr in enumerate(frames):
        x0, y0, w, h = fr["rect"]
        region = canvas[y0:y0 + h, x0:x0 + w]
        before = region.copy()
        idx = fr["indices"].astype(np.int64)
        clear = head["alpha"][idx] == 0
        if fr.get("blend_op", BLEND_SOURCE) == BLEND_SOURCE:
            region[...] = np.where(clear, -1, idx)
        else:
            region[...] = np.where(clear, before, idx)
        out.append(canvas.copy())
        dispose = fr.get("dispose_op", DISPOSE_NONE)
        if dispose == DISPOSE_PREVIOUS and i == 0:
            dispose = DISPOSE_BACKGROUND
        if dispose == DISPOSE_BACKGROUND:
            region[...] = -1
        elif dispose == DISPOSE_PREVIOUS:
            region[...] = before
    return np.stack(out)


def rect_rows(maps, rects, f):
    """Frame f's rectangle of (F, H, W) maps; None: the full frame; an empty rectangle stands for (0, 0, 1, 1)."""
    if rects is None:
        return maps[f]
    x0, y0, w, h = (int(v) for v in rects[f])
    if w == 0 and h == 0:
        x0, y0, w, h = 0, 0, 1, 1
    return maps[f, y0:y0 + h, x0:x0 + w]


def zlib_png_deflate(maps, rects=None, segment=None, level=6):
    """A stand-in for `patolette_amd.png_deflate` with its return shape: raw deflate streams by zlib, no device."""
    maps = np.asarray(maps)
    if maps.ndim == 2:
        maps = maps[None]
    parts, offsets, adler = [], [0], []
    for f in range(maps.shape[0]):
        stream = filtered(rect_rows(maps, rects, f))
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        parts.append(c.compress(stream) + c.flush())
        offsets.append(offsets[-1] + len(parts[-1]))
        adler.append(zlib.adler32(stream))
    data = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return (True, data, np.array(offsets, dtype=np.int64), np.array(adler, dtype=np.uint32), "Success")


def check_streams(maps, rects, data, offsets, adler):
    """What every `png_deflate` result must satisfy: frame f's stream inflates (raw, window 15, nothing left over) to its filtered
    stream byte for byte, and adler[f] is that stream's Adler-32."""
    maps = np.asarray(maps)
    if maps.ndim == 2:
        maps = maps[None]
    assert offsets[0] == 0 and offsets[-1] == data.size and len(offsets) == maps.shape[0] + 1 and len(adler) == maps.shape[0]
    for f in range(maps.shape[0]):
        want = filtered(rect_rows(maps, rects, f))
        d = zlib.decompressobj(-15)
        got = d.decompress(data[int(offsets[f]):int(offsets[f + 1])].tobytes()) + d.flush()
        assert d.eof and not d.unused_data, "frame %d: the stream does not end where its bytes end" % f
        assert got == want, "frame %d: %d bytes inflate to %d, first difference at %d" % (
            f, len(want), len(got), next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want))))
        assert int(adler[f]) == zlib.adler32(want), "frame %d: adler" % f
