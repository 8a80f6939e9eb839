"""The encode stage (include/kajo_hip.h "The encode") restated in numpy, independent of the library: the transfer tables from the analytic
formulas in binary64 (the C library's pow through math.pow, one entry at a time, so that the table is the one any IEEE host forms), the
curves, the lookup, the hash, the quantisation and the half rounding in float32 and integer operations, one rounding per operation.
Nothing here calls kajo_hip_encode_table or kajo_hip_encode_pixels."""
import functools
import math

import numpy as np

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64

ARGB8, RGB10A2, RGBA16, RGBA16F = 0, 1, 2, 3
GAMMA22, SRGB, PQ, LINEAR = 0, 1, 2, 3
DITHER, SCENE = 1, 2
CLAMP, REINHARD, ACES = 0, 1, 2
LOG2E = 7  # the library's E = 128 knots per binade (the sweep)
BINADES = 32
LOW = 2.0 ** -32
MAXCODE = {ARGB8: 255, RGB10A2: 1023, RGBA16: 65535}
BYTES = {ARGB8: 4, RGB10A2: 4, RGBA16: 8, RGBA16F: 8}
DTYPE = {ARGB8: np.uint32, RGB10A2: np.uint32, RGBA16: np.uint64, RGBA16F: np.uint64}

_PQ = dict(m1=2610.0 / 16384.0, m2=2523.0 / 4096.0 * 128.0, c1=3424.0 / 4096.0, c2=2413.0 / 4096.0 * 32.0, c3=2392.0 / 4096.0 * 32.0)


def t64(transfer, peak, y, pow=np.power):
    """the analytic transfer in binary64; y a float64 array (pow = np.power) or a float (pow = math.pow)"""
    if transfer == GAMMA22:
        return pow(y, 1.0 / 2.2)
    if transfer == SRGB:
        hi = 1.055 * pow(y, 1.0 / 2.4) - 0.055
        if isinstance(y, float):
            return 12.92 * y if y <= 0.0031308 else hi
        return np.where(y <= 0.0031308, 12.92 * y, hi)
    if transfer == PQ:
        lp = pow(y * float(peak) / 10000.0, _PQ["m1"])
        return pow((_PQ["c1"] + _PQ["c2"] * lp) / (1.0 + _PQ["c3"] * lp), _PQ["m2"])
    return y


def knots(log2e=LOG2E):
    """the float32 knots y_0 .. y_{32 E}: the last one is 1.0"""
    n = BINADES << log2e
    bits = (np.arange(n + 1, dtype=np.uint64) + np.uint64((127 - BINADES) << log2e)) << np.uint64(23 - log2e)
    return bits.astype(U32).view(F32)


def table(transfer, peak, log2e=LOG2E):
    """(T_i, S_i) interleaved, i = 0 .. 32 E; the last entry is (T64(1), the slope below 2^-32). Formed once per transfer; read-only."""
    return _table(int(transfer), float(F32(peak)) if transfer == PQ else 0.0, int(log2e))


@functools.lru_cache(maxsize=None)
def _table(transfer, peak, log2e):
    y = [float(v) for v in knots(log2e)]
    t = [t64(transfer, peak, v, math.pow) for v in y]
    out = np.zeros(2 * len(y), F32)
    out[0::2] = np.array(t, F64).astype(F32)
    out[1:-1:2] = np.array([(t[i + 1] - t[i]) / (y[i + 1] - y[i]) for i in range(len(y) - 1)], F64).astype(F32)
    out[-1] = F32(t64(transfer, peak, LOW, math.pow) / LOW)
    out.setflags(write=False)
    return out


def lookup(tab, y, log2e=LOG2E):
    """v of the definition for float32 y >= 0 (an array)"""
    y = np.asarray(y, F32)
    n = BINADES << log2e
    idx = (y.view(U32).astype(np.int64) >> (23 - log2e)) - ((127 - BINADES) << log2e)
    i = np.clip(idx, 0, n - 1)
    yk = ((i + ((127 - BINADES) << log2e)) << (23 - log2e)).astype(U32).view(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        inner = np.minimum(tab[2 * i] + (y - yk) * tab[2 * i + 1], tab[2 * i + 2])
        below = y * tab[-1]
    return np.where(y >= F32(1.0), tab[-2], np.where(y < F32(LOW), below, inner)).astype(F32)


def _max0(t):
    with np.errstate(invalid="ignore"):
        return np.where(t > F32(0), t, F32(0)).astype(F32)


def _min1(t):
    with np.errstate(invalid="ignore"):
        return np.where(t < F32(1), t, F32(1)).astype(F32)


def scale_of(exposure):
    return F32(2.0 ** float(F32(exposure)))


def curve(mean, curve_id, s, white):
    """m (n, 3) float32 -> (x, y): the exposed colour and the curve's value"""
    m = np.asarray(mean, F32).reshape(-1, 3)
    s, white = F32(s), F32(white)
    with np.errstate(all="ignore"):
        x = (m * s).astype(F32)
        counts = np.isfinite(m).all(1)
        y = _min1(_max0(x))
        if curve_id == REINHARD:
            L = ((F32(0.2126) * x[:, 0] + F32(0.7152) * x[:, 1]) + F32(0.0722) * x[:, 2]).astype(F32)
            one = F32(1.0)
            ratio = ((one + L / (white * white)) / (one + L)) if white > 0 else (one / (one + L))
            r = _min1(_max0((x * ratio.astype(F32)[:, None]).astype(F32)))
            r = np.where((L > 0)[:, None], r, F32(0))
            y = np.where(counts[:, None], r, y)
        elif curve_id == ACES:
            v = np.where(x < F32(1e4), x, F32(1e4)).astype(F32)
            num = (v * (F32(2.51) * v + F32(0.03))).astype(F32)
            den = (v * (F32(2.43) * v + F32(0.59)) + F32(0.14)).astype(F32)
            y = np.where(counts[:, None], _min1(_max0((num / den).astype(F32))), y)
    return x, y.astype(F32)


def hash32(px, py, channel, seed):
    """the header's hash, operation by operation, modulo 2^32"""
    M = np.uint64(0xFFFFFFFF)
    px, py = np.asarray(px).astype(np.uint64) & M, np.asarray(py).astype(np.uint64) & M
    h = (py * np.uint64(0x85EBCA6B)) & M
    h = h ^ ((np.uint64(channel) * np.uint64(0xC2B2AE35)) & M)
    h = h ^ np.uint64(seed)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & M
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & M
    h = h ^ (h >> np.uint64(16))
    return ((h + px * np.uint64(0x9E3779B9)) & M).astype(U32)


def dither_offset(px, py, channel, seed):
    return ((hash32(px, py, channel, seed) >> U32(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)


def quantise(v, maxcode, d):
    q = np.floor((v * F32(maxcode)).astype(F32) + d).astype(np.int64)
    return np.clip(q, 0, maxcode).astype(np.uint64)


def half_bits(f):
    """float32 -> binary16 bits, round to nearest even, by integer operations (finite input below 65520)"""
    b = np.asarray(f, F32).view(U32).astype(np.int64)
    sign = (b >> 16) & 0x8000
    a = b & 0x7FFFFFFF
    # normal halves
    r = a - 0x38000000
    h = r >> 13
    rem = r & 0x1FFF
    normal = h + ((rem > 0x1000) | ((rem == 0x1000) & ((h & 1) == 1)))
    # subnormal halves: the significand with its hidden bit, shifted down to units of 2^-24
    e = a >> 23
    s = np.clip(126 - e, 14, 24)
    m = (a & 0x7FFFFF) | 0x800000
    hs = m >> s
    rs = m & ((1 << s) - 1)
    halfway = 1 << (s - 1)
    sub = hs + ((rs > halfway) | ((rs == halfway) & ((hs & 1) == 1)))
    out = np.where(a < 0x33000000, 0, np.where(a < 0x38800000, sub, normal))
    return (sign | out).astype(np.uint64)


def encode_pixels(fmt, transfer, flags, peak, seed, curve_id, exposure, white, mean, x0=0, y0=0, row_width=None, log2e=LOG2E, scale=None):
    """the words of n pixels of MEANS (n, 3), row-major in a rectangle row_width wide whose first pixel is (x0, y0)"""
    m = np.asarray(mean, F32).reshape(-1, 3)
    n = len(m)
    row_width = row_width or max(n, 1)
    i = np.arange(n, dtype=np.int64)
    px, py = x0 + i % row_width, y0 + i // row_width
    s = scale_of(exposure) if scale is None else F32(scale)
    x, y = curve(m, curve_id, s, white)
    if fmt == RGBA16F:
        if flags & SCENE:
            with np.errstate(invalid="ignore"):
                v = np.where(x > F32(0), x, F32(0)).astype(F32)
                v = np.where(v < F32(65504), v, F32(65504)).astype(F32)
        else:
            v = y
        c = half_bits(v)
        return (c[:, 0] | (c[:, 1] << np.uint64(16)) | (c[:, 2] << np.uint64(32)) | (np.uint64(0x3C00) << np.uint64(48))).astype(np.uint64)
    v = y if transfer == LINEAR else lookup(table(transfer, peak, log2e), y.reshape(-1), log2e).reshape(-1, 3)
    M = MAXCODE[fmt]
    c = np.zeros((n, 3), np.uint64)
    for ch in range(3):
        d = dither_offset(px, py, ch, seed) if flags & DITHER else F32(0.5)
        c[:, ch] = quantise(v[:, ch], M, d)
    if fmt == ARGB8:
        return (np.uint64(0xFF000000) | (c[:, 0] << np.uint64(16)) | (c[:, 1] << np.uint64(8)) | c[:, 2]).astype(np.uint32)
    if fmt == RGB10A2:
        return (np.uint64(0xC0000000) | (c[:, 0] << np.uint64(20)) | (c[:, 1] << np.uint64(10)) | c[:, 2]).astype(np.uint32)
    return (c[:, 0] | (c[:, 1] << np.uint64(16)) | (c[:, 2] << np.uint64(32)) | (np.uint64(0xFFFF) << np.uint64(48))).astype(np.uint64)


def sweep(log2e, transfer, peak, stride=61):
    """the accuracy sweep of the definition: float32 y in [2^-32, 1], every `stride`-th value plus every knot and its two neighbours ->
    (the largest |v(y) - T64(y)| * 65535, the sweep's y sorted, its v)"""
    lo, hi = int(F32(LOW).view(U32)), int(F32(1.0).view(U32))
    k = knots(log2e).view(U32).astype(np.int64)
    bits = np.unique(np.concatenate([np.arange(lo, hi + 1, stride, dtype=np.int64), k, k - 1, k + 1]))
    bits = bits[(bits >= lo) & (bits <= hi)]
    y = bits.astype(U32).view(F32)
    v = lookup(table(transfer, peak, log2e), y, log2e)
    dev = np.abs(v.astype(F64) - t64(transfer, float(F32(peak)), y.astype(F64))) * 65535.0
    return float(dev.max()), y, v


def edge_means():
    """the edge inputs of the tests, as (n, 3) means: exact 0, -0, negatives, denormals, NaN, +-Inf, every knot of two binades with one ulp
    either side, 2^-32 and its neighbours, 1.0 and its neighbours, values far above 1, the half format's rounding ties and the 65504
    boundary"""
    def around(bits):
        bits = np.asarray(bits, np.int64)
        return np.concatenate([bits - 1, bits, bits + 1]).astype(U32).view(F32)

    k = knots().view(U32).astype(np.int64)
    per = 1 << LOG2E
    two = np.concatenate([k[(126 - 95) * per:], k[(117 - 95) * per:(118 - 95) * per + 1]])  # the binades [0.5, 1) and [2^-10, 2^-9)
    half_ties = []
    for h in (0x0001, 0x0002, 0x03FF, 0x0400, 0x0401, 0x3BFF, 0x3C00, 0x1234, 0x7BFE, 0x7BFF):  # halfway between h and h + 1
        a, b = np.array([h, h + 1], np.uint16).view(np.float16).astype(F64)
        half_ties.append(F32(0.5 * (a + b)))
    special = np.array([0.0, -0.0, -1.0, -1e-30, -3e38, 1e-45, -1e-45, 1e-40, 1.17549435e-38, np.nan, np.inf, -np.inf, 2.0 ** -25, 2.0 ** -24,
                        2.0 ** -14, 1.5, 2.0, 7.25, 1e4, 1.0001e4, 65503.9, 65504.0, 65505.0, 65519.9, 65520.0, 1e9, 3e38], F32)
    vals = np.concatenate([special, around(two), around([int(F32(LOW).view(U32))]), around([int(F32(1.0).view(U32))]),
                           around([int(F32(65504.0).view(U32))]), around(np.array(half_ties, F32).view(U32)), np.array(half_ties, F32)])
    n = len(vals)
    m = np.stack([vals, np.roll(vals, 7), np.roll(vals[::-1], 3)], 1)
    # NaN / Inf in one channel beside finite ones is covered by the rolls; add rows that are grey, so every value is seen by every channel
    return np.concatenate([m, np.repeat(vals[:, None], 3, 1)]).astype(F32)


def binade_ramp(per=5):
    """a ramp through every binade from 2^-34 to 2^2: `per` values a binade, as grey means with a tint"""
    e = np.arange(-34, 2)
    f = 1.0 + np.arange(per) / per
    v = (2.0 ** e[:, None] * f[None, :]).reshape(-1).astype(F32)
    return np.stack([v, (v * F32(0.75)).astype(F32), (v * F32(1.25)).astype(F32)], 1)
