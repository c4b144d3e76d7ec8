"""Reference of the RGBA entry's dither, restated in Python (test infrastructure).

The reference's Riemersma walk (dither/riemersma.c:124-257) visits the positions of a 2^L square along the Hilbert curve and
skips those outside the image: no dithering, the error queue unchanged (riemersma.c:151-156, move()).  The RGBA entry treats a
transparent pixel exactly like such a position.  So its chain is the reference's chain over the visit order of the image
(`oracle.hilbert_order`) with the transparent pixels dropped.  `masked_dither` is that chain, step for step as
tests/independent_ref.dither computes it (riemersma.c:275-341 + :360-426)."""
import numpy as np

RW, GW, BW = 0.51254268114958, 0.8234075540095561, 0.2435159132377184


def dither_weights():
    m = np.exp(np.log(16.0) / (16.0 - 1))
    wts = np.zeros(16)
    v = 1.0
    for i in range(16):
        wts[i] = v / 16.0
        v *= m
    return wts


def chain(img, visit, pal):
    """The chain over the pixel numbers `visit` in order: img (N,3) linear Rec2020, pal (k,3).  Returns {pixel: choice}."""
    fw = np.array([np.float64(np.float32(RW)), np.float64(np.float32(GW)), np.float64(np.float32(BW))])
    palw = pal * fw
    wts = dither_weights()
    q = np.zeros((16, 3))
    out = {}
    for p in visit:
        p = int(p)
        err = np.zeros(3)
        for i in range(16):
            err = err + q[i] * wts[i]
        px = img[p]
        cor = px + err
        qq = np.array([RW * cor[0], GW * cor[1], BW * cor[2]])
        d = ((qq[0] - palw[:, 0]) ** 2 + (qq[1] - palw[:, 1]) ** 2) + (qq[2] - palw[:, 2]) ** 2
        idx = int(np.argmin(d))
        out[p] = idx
        q[:-1] = q[1:]
        q[15] = px - pal[idx]
    return out


def masked_dither(ob, img, width, height, pal, opaque):
    """The reference's walk over the width x height image with the pixels where `opaque` is False skipped like out-of-image
    positions.  Returns an int64 map of width*height entries: the choice on visited pixels, -1 elsewhere."""
    opaque = np.asarray(opaque, dtype=bool).reshape(-1)
    order = ob.hilbert_order(width, height) if max(width, height) > 1 else np.zeros(0, dtype=np.uint64)
    visit = order[opaque[order.astype(np.int64)]] if order.size else order
    out = np.full(width * height, -1, dtype=np.int64)
    for p, c in chain(np.asarray(img, dtype=np.float64).reshape(-1, 3), visit, pal).items():
        out[p] = c
    return out


def hilbert_level(width, height):
    """L of the reference's 2^L square (riemersma.c:437-451): ceil(log2(max(width, height)))."""
    mx, L = max(width, height), 0
    while (1 << L) < mx:
        L += 1
    return L
