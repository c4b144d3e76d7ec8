"""The colour conversions in high precision, the inputs at which they can go wrong, and the oracle's own rounding noise.

Three things, shared by tests/test_color_reference.py (CPU) and tests/test_gpu_color_edges.py (GPU):

* `mp_convert(name, planar)`: the six conversions and the fused Luv -> ICtCp chain with mpmath at 40 digits, written from the
  reference's C sources as oracle/patolette_oracle.c cites them (eotf.c, sRGB.c, xyz.c, rec2020.c, ICtCp.c, CIELuv.c).  Constants
  are the decimal literals of the C code, taken exactly (0.4124564 is 4124564 / 10^7, `1.0 / 2.4` is 5/12), and every branch is
  taken on the exact value.  pow / fmax / fmin follow C for negative, infinite and NaN operands.
* `edge_sets()` / `random_sets()`: the inputs.  Plain numpy and the oracle, no mpmath.
* `dref_table()`: per conversion, input set and output plane the largest |oracle - exact| in units of that plane's max |want|:
  the f64 rounding noise of the reference arithmetic itself, the yardstick for what a last-ulp pow neighbour may move.

A branch decided within 2^-40 (relative) of its threshold is "near": the f64 chain may land on the other side there, and the
distance between the two then measures the curve's jump (sRGB's companding is not continuous at its knee; a zero denominator
that f64 hits exactly is 1e-17 away from zero in exact arithmetic), not rounding noise.  Such pixels are left out of D_ref.
"""
import functools
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DREF_PATH = os.path.join(GOLDEN, "color_dref.json")

CONVERSIONS = ("srgb_to_ictcp", "srgb_to_cieluv", "ictcp_to_rec2020", "cieluv_to_rec2020", "srgb_to_rec2020", "rec2020_to_srgb",
               "cieluv_to_ictcp")
CONV_ID = {name: i for i, name in enumerate(CONVERSIONS)}          # the ids of patolette_amd_convert
FUSED = ("cieluv_to_rec2020", "rec2020_to_srgb", "srgb_to_ictcp")  # patolette.c:305-314: what cieluv_to_ictcp stands for
SOURCE = {"srgb_to_ictcp": "srgb", "srgb_to_cieluv": "srgb", "srgb_to_rec2020": "srgb", "ictcp_to_rec2020": "ictcp",
          "cieluv_to_rec2020": "cieluv", "cieluv_to_ictcp": "cieluv", "rec2020_to_srgb": "rec2020"}
RANDOM_N = 20000
NEAR = 2.0 ** -40


# ----------------------------------------------------------------------------------------------------------------------
# the conversions, exactly
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ctx():
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.dps = 40
    return ctx


class _Exact:
    """One pixel through the reference's expressions; `near` is set when a branch was decided within NEAR of its threshold."""

    def __init__(self):
        c = self.c = _ctx()
        m = self.m = c.mpf
        self.near = False
        self._literals = {}
        k = self.k
        self.zero, self.one = m(0), m(1)
        # eotf.c:13-18
        self.Lp, self.m1, self.m2 = m(10000), k("0.1593017578125"), k("78.84375")
        self.c1, self.c2, self.c3 = k("0.8359375"), k("18.8515625"), k("18.6875")
        # CIELuv.c:19-25
        self.rwx, self.rwy, self.rwz = k("0.95047"), m(1), k("1.08883")
        self.kE, self.kK, self.kKE = m(216) / 24389, m(24389) / 27, m(8)

    def k(self, literal):
        """A decimal literal of the C code, exactly."""
        v = self._literals.get(literal)
        if v is None:
            v = self._literals[literal] = self.m(literal)
        return v

    # -- C semantics on top of mpf ------------------------------------------------------------------------------------
    def mark(self, x, t, scale=0):
        c = self.c
        if not (c.isfinite(x) and c.isfinite(t)):
            return
        d = abs(x - t)
        if d != 0 and d <= NEAR * max(abs(x), abs(t), scale):
            self.near = True

    def div(self, a, b):
        c = self.c
        if b == 0 and not c.isnan(a):
            return c.nan if a == 0 else (c.inf if a > 0 else -c.inf)       # the sign of a zero is not kept: no caller depends on it
        return a / b

    def pow(self, x, y):
        """C's pow for y > 0 finite: NaN for NaN or a negative x with a non-integer y."""
        c = self.c
        if c.isnan(x):
            return c.nan
        if x == 0:
            return self.zero
        if x < 0:
            return c.power(x, y) if y == int(y) else c.nan
        if c.isinf(x):
            return c.inf
        return c.power(x, y)

    def fmax(self, a, b):
        c = self.c
        if c.isnan(a):
            return b
        if c.isnan(b):
            return a
        return a if a > b else b

    def fmin(self, a, b):
        c = self.c
        if c.isnan(a):
            return b
        if c.isnan(b):
            return a
        return a if a < b else b

    # -- eotf.c ---------------------------------------------------------------------------------------------------------
    def eotf(self, v):                                           # eotf.c:29-42
        V_p = self.pow(v, 1 / self.m2)
        n = self.fmax(self.zero, V_p - self.c1)
        return self.Lp * self.pow(self.div(n, self.c2 - self.c3 * V_p), 1 / self.m1)

    def eotf_inv(self, v):                                       # eotf.c:44-57
        y_ = self.pow(v / self.Lp, self.m1)
        return self.pow((self.c1 + self.c2 * y_) / (1 + self.c3 * y_), self.m2)

    # -- sRGB.c ---------------------------------------------------------------------------------------------------------
    def gamma_decode(self, v):                                   # sRGB.c:70-89
        k = self.k
        t = k("0.0404500")
        self.mark(v, t)
        r = v / k("12.92") if v <= t else self.pow((v + k("0.055")) / k("1.055"), k("2.4"))
        return self.fmin(self.fmax(r, self.zero), self.one)

    def gamma_encode(self, v):                                   # sRGB.c:91-110
        k = self.k
        t = k("0.0031308")
        self.mark(v, t)
        r = v * k("12.92") if v <= t else k("1.055") * self.pow(v, 1 / k("2.4")) - k("0.055")
        return self.fmin(self.fmax(r, self.zero), self.one)

    # -- xyz.c, rec2020.c -----------------------------------------------------------------------------------------------
    def linear_to_xyz(self, R, G, B):                            # xyz.c:27-39
        k = self.k
        return (R * k("0.4124564") + G * k("0.3575761") + B * k("0.1804375"),
                R * k("0.2126729") + G * k("0.7151522") + B * k("0.0721750"),
                R * k("0.0193339") + G * k("0.1191920") + B * k("0.9503041"))

    def xyz_to_rec2020(self, x, y, z):                           # rec2020.c:80-102
        k = self.k
        return (x * k("1.71666343") + y * k("-0.35567332") + z * k("-0.25336809"),
                x * k("-0.66667384") + y * k("1.61645574") + z * k("0.0157683"),
                x * k("0.01764248") + y * k("-0.04277698") + z * k("0.94224328"))

    def srgb_to_rec2020(self, p):                                # rec2020.c:104-126
        return self.xyz_to_rec2020(*self.linear_to_xyz(*(self.gamma_decode(v) for v in p)))

    def rec2020_to_srgb(self, p):                                # sRGB.c:32-59 + xyz.c:42-64
        k = self.k
        r2, g2, b2 = p
        x = r2 * k("0.63695351") + g2 * k("0.14461919") + b2 * k("0.16885585")
        y = r2 * k("0.26269834") + g2 * k("0.67800877") + b2 * k("0.0592929")
        z = g2 * k("0.02807314") + b2 * k("1.06082723")
        r = x * k("3.2404542") - y * k("1.5371385") - z * k("0.4985314")
        g = -x * k("0.9692660") + y * k("1.8760108") + z * k("0.0415560")
        b = x * k("0.0556434") - y * k("0.2040259") + z * k("1.0572252")
        return self.gamma_encode(r), self.gamma_encode(g), self.gamma_encode(b)

    # -- ICtCp.c ----------------------------------------------------------------------------------------------------------
    def rec2020_to_ictcp(self, p):                               # ICtCp.c:41-79 (Ct halved)
        r, g, b = p
        L = (r * 1688 + g * 2146 + b * 262) / 4096
        M = (r * 683 + g * 2951 + b * 462) / 4096
        S = (r * 99 + g * 309 + b * 3688) / 4096
        L_, M_, S_ = self.eotf_inv(L), self.eotf_inv(M), self.eotf_inv(S)
        return (L_ / 2 + M_ / 2, (L_ * 6610 - M_ * 13613 + S_ * 7003) / 4096 / 2, (L_ * 17933 - M_ * 17390 - S_ * 543) / 4096)

    def ictcp_to_rec2020(self, p):                               # rec2020.c:32-69 (Ct doubled)
        k = self.k
        I, Ct, Cp = p[0], p[1] * 2, p[2]
        L_ = I + k("0.00860904") * Ct + k("0.11102963") * Cp
        M_ = I - k("0.00860904") * Ct - k("0.11102963") * Cp
        S_ = I + k("0.56003134") * Ct - k("0.32062717") * Cp
        L, M, S = self.eotf(L_), self.eotf(M_), self.eotf(S_)
        return (L * k("3.43660669") - M * k("2.50645212") + S * k("0.06984542"),
                -L * k("0.79132956") + M * k("1.98360045") - S * k("0.1922709"),
                -L * k("0.0259499") - M * k("0.09891371") + S * k("1.12486361"))

    # -- CIELuv.c ---------------------------------------------------------------------------------------------------------
    def srgb_to_cieluv(self, p):                                 # CIELuv.c:166-197 + :54-89
        x, y, z = self.linear_to_xyz(*(self.gamma_decode(v) for v in p))
        den = x + 15 * y + 3 * z
        self.mark(den, self.zero, abs(x) + 15 * abs(y) + 3 * abs(z))
        up = 4 * x / den if den > 0 else self.zero
        vp = 9 * y / den if den > 0 else self.zero
        wden = self.rwx + 15 * self.rwy + 3 * self.rwz
        urp, vrp = 4 * self.rwx / wden, 9 * self.rwy / wden
        yr = y / self.rwy
        self.mark(yr, self.kE)
        L_ = 116 * self.pow(yr, self.one / 3) - 16 if yr > self.kE else self.kK * yr
        return L_, 13 * L_ * (up - urp), 13 * L_ * (vp - vrp)

    def cieluv_to_rec2020(self, p):                              # CIELuv.c:100-164 + rec2020.c:150-173
        L, u, v = p
        self.mark(L, self.kKE)
        y_ = self.pow((L + 16) / 116, self.m(3)) if L > self.kKE else L / self.kK
        wden = self.rwx + 15 * self.rwy + 3 * self.rwz
        u0, v0 = 4 * self.rwx / wden, 9 * self.rwy / wden
        a_den = u + 13 * L * u0
        self.mark(a_den, self.zero, abs(u) + abs(13 * L * u0))
        a = self.zero if a_den == 0 else (52 * L / a_den - 1) / 3
        b = -5 * y_
        cc = -self.one / 3
        d_den = v + 13 * L * v0
        self.mark(d_den, self.zero, abs(v) + abs(13 * L * v0))
        d = self.zero if d_den == 0 else y_ * (39 * L / d_den - 5)
        x_den = a - cc
        self.mark(x_den, self.zero, abs(a) + abs(cc))
        x_ = self.zero if x_den == 0 else (d - b) / x_den
        return self.xyz_to_rec2020(x_, y_, x_ * a + b)

    def srgb_to_ictcp(self, p):                                  # ICtCp.c:120-146
        return self.rec2020_to_ictcp(self.srgb_to_rec2020(p))

    def cieluv_to_ictcp(self, p):                                # patolette.c:305-314, nothing rounded in between
        return self.srgb_to_ictcp(self.rec2020_to_srgb(self.cieluv_to_rec2020(p)))


def mp_convert(name, planar):
    """planar f64 (3n) -> (want, near): want[p][i] the exact value of plane p at pixel i as an mpf, near[i] whether a branch was close."""
    planar = np.asarray(planar, dtype=np.float64)
    n = planar.size // 3
    px = planar.reshape(3, n)
    ex = _Exact()
    fn = getattr(ex, name)
    want = ([None] * n, [None] * n, [None] * n)
    near = np.zeros(n, dtype=bool)
    seen = {}
    for i in range(n):
        key = px[:, i].tobytes()
        if key not in seen:
            ex.near = False
            out = fn(tuple(ex.m(float(v)) for v in px[:, i]))
            seen[key] = (out, ex.near)
        out, near[i] = seen[key]
        want[0][i], want[1][i], want[2][i] = out
    return want, near


def distance(got, want):
    """|got - want| per pixel in f64 for one plane (want: mpf list); NaN where either side is not finite."""
    c = _ctx()
    out = np.full(len(want), np.nan)
    for i, (g, w) in enumerate(zip(got, want)):
        if math.isfinite(g) and c.isfinite(w):
            out[i] = float(abs(c.mpf(float(g)) - w))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
def neighbours(x, k):
    """x with k doubles on each side, ascending."""
    lo, hi, out = x, x, [x]
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out = [float(lo)] + out + [float(hi)]
    return out


def srgb_edge_values():
    v = [-0.0, 0.0, 5e-324, 1e-310]
    v += neighbours(1e-200, 2)                                   # div_const's guard
    v += [1e-9, 0.0404, 0.0405] + neighbours(0.04045, 2)
    v += [k / 255.0 for k in range(256)]
    v += [1 - 2.0 ** -53, 1.0, 1 + 2.0 ** -52, 1.5, -0.25]
    v += [1e300, -1e300, np.inf, -np.inf, np.nan]                # the companding clamps all of these to 0 or 1
    return v


def _pixels(values):
    """Every value in each channel in turn, the other two channels at the same value, at 0.5 and at 0: planar (3n)."""
    rows = []
    for v in values:
        for ch in range(3):
            for other in (v, 0.5, 0.0):
                p = [other] * 3
                p[ch] = v
                rows.append(p)
    return _planar(rows)


def _planar(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 3).T).reshape(-1)


def _cat(*planars):
    return np.concatenate([np.asarray(p).reshape(3, -1) for p in planars], axis=1).reshape(-1)


def _bisect(pred, lo, hi):
    """Largest double x in [lo, hi) with pred(x) false, pred monotone, pred(lo) false, pred(hi) true; lo, hi > 0."""
    a, b = (int(np.float64(v).view(np.int64)) for v in (lo, hi))
    assert not pred(lo) and pred(hi)
    while b - a > 1:
        mid = (a + b) // 2
        if pred(float(np.int64(mid).view(np.float64))):
            b = mid
        else:
            a = mid
    return float(np.int64(a).view(np.float64))


def _around(x, k=64):
    """k consecutive doubles up to and including x and k above it."""
    return neighbours(x, k)[1:] if k else [x]


@functools.lru_cache(maxsize=None)
def knees():
    """The three knees that lie behind arithmetic, located with the oracle: the grey whose yr crosses 216/24389 (L crosses 8 there),
    per output channel the Rec2020 grey whose linear sRGB crosses 0.0031308 (the output crosses 12.92 * 0.0031308), and L = 8."""
    from oracle import binding as ob
    grey_luv = _bisect(lambda g: ob.convert("srgb_to_cieluv", np.array([g, g, g]))[0] > 8.0, 0.01, 0.5)
    grey_enc = [_bisect(lambda g, ch=ch: ob.convert("rec2020_to_srgb", np.array([g, g, g]))[ch] > 0.0031308 * 12.92, 1e-4, 0.1)
                for ch in range(3)]
    return dict(srgb_grey=_around(grey_luv), rec2020_grey=[_around(g) for g in grey_enc], L=_around(8.0))


def _freeze(d):
    for sets in d.values():
        for a in sets.values():
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def edge_sets():
    """conversion -> {set name -> planar f64 input}.  Built once and read-only."""
    from oracle import binding as ob
    k = knees()
    srgb = _cat(_pixels(srgb_edge_values()), _planar([[g, g, g] for g in k["srgb_grey"]]))
    finite = np.all(np.isfinite(srgb.reshape(3, -1)), axis=0)
    srgb_finite = srgb.reshape(3, -1)[:, finite].reshape(-1)

    rec2020 = _cat(ob.convert("srgb_to_rec2020", srgb_finite), *[_planar([[g, g, g] for g in gs]) for gs in k["rec2020_grey"]])

    # CIELuv.c:100-164 evaluates u0 and v0 in f64; a_den and d_den are exactly zero for the u and v built the same way
    u0 = (4.0 * 0.95047) / (0.95047 + 15.0 * 1.0 + 3.0 * 1.08883)
    v0 = (9.0 * 1.0) / (0.95047 + 15.0 * 1.0 + 3.0 * 1.08883)
    luv = [[0.0, 0.0, 0.0]]
    luv += [[0.0, u, 0.0] for u in (1.0, -2.5, 1e-300)] + [[0.0, 0.0, v] for v in (1.0, -2.5, 1e-300)]
    for L in (1.0, 8.0, 50.0, 100.0):
        luv += [[L, -(13.0 * L * u0), w] for w in (0.0, 7.0)]                   # a_den == 0
        luv += [[L, w, -(13.0 * L * v0)] for w in (0.0, 7.0)]                   # d_den == 0
        luv += [[L, -(13.0 * L * u0), -(13.0 * L * v0)]]
    luv += [[L, u, v] for L in k["L"] for (u, v) in ((0.0, 0.0), (3.0, -2.0))]
    cieluv = _cat(ob.convert("srgb_to_cieluv", srgb_finite), _planar(luv))

    # eotf.c:29-42: n = fmax(0, V_p - c1) is 0 for I' <= c1^m2
    i0 = 0.8359375 ** 78.84375
    clamp = [[I, 0.0, 0.0] for I in neighbours(i0, 3) + [i0 / 2, 1e-9, 1e-300, 0.0]]
    clamp += [[i0, 1e-7, -1e-7], [2 * i0, 0.0, 0.0]]
    ictcp = _cat(ob.convert("srgb_to_ictcp", srgb_finite), _planar(clamp))
    extreme = [[I, ct, cp] for I in (1.0, 1.5, 1.99, 2.1) for (ct, cp) in ((0.0, 0.0), (0.01, -0.02))]
    extreme += [[0.001, 0.0, 0.1], [0.5, 0.0, 5.0]]                              # M' < 0: pow of a negative number
    return _freeze({
        "srgb_to_ictcp": {"edges": srgb}, "srgb_to_cieluv": {"edges": srgb}, "srgb_to_rec2020": {"edges": srgb},
        "rec2020_to_srgb": {"edges": rec2020},
        "cieluv_to_rec2020": {"edges": cieluv}, "cieluv_to_ictcp": {"edges": cieluv},
        "ictcp_to_rec2020": {"edges": ictcp, "extreme": _planar(extreme)},
    })


def random_input(name, n, seed):
    """n uniform sRGB pixels taken by the oracle into the space the conversion starts from."""
    from oracle import binding as ob
    src = ob.image(n, seed)
    space = SOURCE[name]
    return src if space == "srgb" else ob.convert("srgb_to_" + space, src)


@functools.lru_cache(maxsize=None)
def random_sets():
    return _freeze({name: {"random": random_input(name, RANDOM_N, 40 + i)} for i, name in enumerate(CONVERSIONS)})


@functools.lru_cache(maxsize=None)
def oracle_convert(name, key, n=None):
    """The oracle's answer for a named input set (or, key == seed, for random_input(name, n, seed)); computed once, read-only."""
    if n is not None:
        src = random_input(name, n, key)
    else:
        src = (random_sets() if key == "random" else edge_sets())[name][key]
    out = convert_f64(name, src)
    out.setflags(write=False)
    return out


def convert_f64(name, planar):
    from oracle import binding as ob
    if name != "cieluv_to_ictcp":
        return ob.convert(name, planar)
    out = planar
    for hop in FUSED:
        out = ob.convert(hop, out)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the oracle's own distance
# ----------------------------------------------------------------------------------------------------------------------
def plane_scale(want_plane):
    """max |want| over the finite entries of one plane (0 if there is none)."""
    a = np.abs(np.asarray(want_plane, dtype=np.float64))
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def measure_dref(name, key):
    """(D_ref per plane, nan_mismatch) of one input set: max |oracle - exact| / max |oracle|, near-branch pixels left out."""
    src = (random_sets() if key == "random" else edge_sets())[name][key]
    f64 = oracle_convert(name, key).reshape(3, -1)
    want, near = mp_convert(name, src)
    c = _ctx()
    out, mismatch = [], 0
    for p in range(3):
        d = distance(f64[p], want[p])
        exact_nan = np.array([bool(c.isnan(w)) for w in want[p]])
        mismatch += int(np.sum((np.isnan(f64[p]) != exact_nan) & ~near))
        d = d[~near & np.isfinite(d)]
        scale = plane_scale(f64[p])
        out.append(float(d.max()) / scale if d.size and scale > 0 else 0.0)
    return out, mismatch


def round_up(x, digits=2):
    """x rounded up to `digits` significant digits: the committed table has to stay above a table regenerated with a libm whose
    pow rounds a last place differently."""
    if x == 0:
        return 0.0
    e = math.floor(math.log10(x)) - (digits - 1)
    return float("%.*e" % (digits - 1, math.ceil(x / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e))


def dref_table(rounded=True):
    table = {}
    for name in CONVERSIONS:
        table[name] = {}
        for key in list(edge_sets()[name]) + ["random"]:
            d, _ = measure_dref(name, key)
            table[name][key] = [round_up(v) if rounded else v for v in d]
    return table


def write_dref(path=DREF_PATH):
    with open(path, "w") as f:
        json.dump(dref_table(), f, indent=1, sort_keys=True)
        f.write("\n")


@functools.lru_cache(maxsize=None)
def load_dref():
    with open(DREF_PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    write_dref()
    print(json.dumps(load_dref(), indent=1, sort_keys=True))


# ----------------------------------------------------------------------------------------------------------------------
# pamd_pow: the exponents, where each is called from, and the inputs by class
# ----------------------------------------------------------------------------------------------------------------------
# exponent -> the argument range of its call site in color_device.h.  A range that starts at 0 has no lowest binade: it is taken
# down to 2^-40, the floor of the log-uniform class.
POW_FLOOR_E, POW_TOP_E = -40, 14
POW_SITES = {
    "2.4": (2.4, (0.04045 + 0.055) / 1.055, 1.0),                 # gamma_decode: (c + 0.055) / 1.055, 0.04045 < c <= 1
    "1/2.4": (1.0 / 2.4, 0.0031308, 1.0),                         # gamma_encode: 0.0031308 < c <= 1
    "m1": (0.1593017578125, 0.0, 1e-4),                           # eotf_inv: v / 10000, 0 <= v <= 1
    "m2": (78.84375, 0.8359375, 1.0),                             # eotf_inv: (c1 + c2 y) / (1 + c3 y), 0 <= y <= 1
    "1/m1": (1.0 / 0.1593017578125, 0.0, 1.0),                    # eotf: n / (c2 - c3 V_p), c1 <= V_p <= 1
    "1/m2": (1.0 / 78.84375, 0.0, 1.0),                           # eotf: 0 <= I' <= 1
    "1/3": (1.0 / 3.0, 216.0 / 24389.0, 1.0),                     # linear_to_cieluv: 216/24389 < yr <= 1
    "3": (3.0, 24.0 / 116.0, 1.0),                                # cieluv_to_rec2020: (L + 16) / 116, 8 < L <= 100
}
POW_STRUCTURED = ("edges", "near1", "ties")
POW_RANDOM = ("site", "loguniform")


def _with_neighbours(x, k=3):
    """x (array) and k doubles on each side of every element."""
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def pow_binades(name):
    _, lo, hi = POW_SITES[name]
    e_lo = POW_FLOOR_E if lo == 0.0 else math.frexp(lo)[1] - 1
    e_hi = math.frexp(hi)[1] - 1
    return sorted(set(range(e_lo, e_hi + 1)) | {POW_FLOOR_E, POW_TOP_E})


@functools.lru_cache(maxsize=None)
def pow_inputs(name):
    """class name -> x (read-only f64) for one exponent."""
    y, lo, hi = POW_SITES[name]
    rng = np.random.default_rng(sorted(POW_SITES).index(name) + 100)
    out = {}
    i = np.arange(129) / 128.0
    out["edges"] = _with_neighbours(np.concatenate([np.ldexp(1.0 + i, e) for e in pow_binades(name)]))
    k = np.arange(1, 53)
    out["near1"] = np.concatenate([1 + 2.0 ** -k, 1 - 2.0 ** -k, 1 + 3 * 2.0 ** -(k + 1.0), 1 - 3 * 2.0 ** -(k + 1.0)])
    # rint(Ph * 64) flips where y log2(x) = (k + 1/2) / 64: every k with x in [2^-40, 2^15) and a normal, finite result
    t_lo = max(POW_FLOOR_E, -1022.0 / y) * 64 * y
    t_hi = min(POW_TOP_E + 1, 1023.0 / y) * 64 * y
    kk = np.arange(math.ceil(t_lo), math.floor(t_hi) - 1, dtype=np.float64)
    out["ties"] = _with_neighbours(np.exp2((kk + 0.5) / (64 * y)))
    out["site"] = lo + (hi - lo) * (1.0 - rng.random(200000))                              # (lo, hi]
    out["loguniform"] = np.exp2(POW_FLOOR_E + (POW_TOP_E + 1 - POW_FLOOR_E) * rng.random(200000))
    out["tiny"] = np.array([5e-324, 4e-320, 1e-310, 2.2250738585072014e-308, np.nextafter(2.2250738585072014e-308, 0.0)])
    if name in ("3", "2.4"):                                                                # results in [2^-1074, 2^-1022)
        out["subnormal"] = np.exp2((-1074 + 52 * rng.random(20000)) / y)
    for a in out.values():
        a.setflags(write=False)
    return out


def pow_reference(x, y):
    """pow(x, y) in long double (64-bit significand): within 0.002 ulp of the f64 result (tests/test_color_reference.py)."""
    with np.errstate(all="ignore"):
        return np.power(np.asarray(x, dtype=np.float64).astype(np.longdouble), np.longdouble(y))


def f64_spacing(ref):
    """The spacing of the doubles at |ref| (long double in, long double out); 2^-1074 throughout the subnormals and below."""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(np.longdouble(1.0), np.maximum(e.astype(np.int64) - 53, -1074).astype(np.int32))


def ulp_error(got, ref):
    """|got - ref| in units of the f64 spacing at ref."""
    return (np.abs(np.asarray(got, dtype=np.float64).astype(np.longdouble) - ref) / f64_spacing(ref)).astype(np.float64)


def correctly_rounded(x, y, ref):
    """The double nearest the exact pow(x, y).  The long-double reference decides it wherever it lies more than 0.002 ulp (its own
    error bound) from the midpoint of two doubles; the rest -- next to 1, (1 +- 2^-k)^y comes within 1e-9 ulp of a midpoint -- is
    settled by mpmath at 60 digits."""
    with np.errstate(over="ignore"):
        rn = ref.astype(np.float64)
    spacing = f64_spacing(ref)
    to_mid = np.abs(np.abs(rn.astype(np.longdouble) - ref) / spacing - np.longdouble(0.5))
    doubt = np.flatnonzero(np.isfinite(rn) & (to_mid < 0.002))
    if doubt.size:
        import mpmath
        ctx = mpmath.mp.clone()
        ctx.dps = 60
        rn = rn.copy()
        for i in doubt:
            exact = ctx.power(ctx.mpf(float(x[i])), ctx.mpf(y))
            cands = (float(np.nextafter(rn[i], -np.inf)), float(rn[i]), float(np.nextafter(rn[i], np.inf)))
            rn[i] = min(cands, key=lambda c: abs(ctx.mpf(c) - exact))
    return rn
