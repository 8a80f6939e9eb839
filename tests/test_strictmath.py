"""include/kajo_strictmath.h: within 1 ulp of the correctly rounded result on the domains the integrator
uses (CPU, through the oracle library), and bit-identical on the GPU (gpu-marked, through the C ABI).
tools/strictmath_exhaustive.c makes the same check over EVERY binary32 of the domains (minutes of CPU time).

The device side of "identical bits" is checked over EVERY binary32 argument: the sweep kernel (kajo_hip_kat_strictmath_sweep) returns two
checksums per (sign, exponent) binade, and tests/golden/strictmath_binades.npz holds the same words from the host build of the header
(tools/make_strictmath_binades.py). The CPU suite recomputes six binades of every table, so a stale fixture fails here and not on the
GPU. What is binary (kdiv, pow in x AND y) is stratified instead: every exponent pair, the mantissas at the ends and at the selects."""
import ctypes as C
import os

import numpy as np
import pytest

from oraclelib import OracleLib, available

pytestmark = pytest.mark.skipif(not available("oracle"), reason="oracle not built")

RNG = np.random.default_rng(7)
N = 200000
U = RNG.random(N).astype(np.float32)
CASES = [
    (0, (2 * np.pi * U).astype(np.float32), None, np.sin),                 # sin(2 pi s), Light.cpp:43, Random.cpp:84
    (0, (np.pi * (U - .5)).astype(np.float32), None, np.sin),              # sin(pi (s - .5)), Light.cpp:45
    (1, (2 * np.pi * U).astype(np.float32), None, np.cos),
    (2, (2 * U - 1).astype(np.float32), None, np.arcsin),                  # asin(r / dist), Light.cpp:32
    (3, (2 * U - 1).astype(np.float32), None, np.arccos),                  # acos(u^(1/(e+1))), Random.cpp:95
    (4, U, np.full(N, 100, np.float32), np.power),                         # cos^e, BSDF.cpp:66
    (4, U, np.full(N, 1 / 101, np.float32), np.power),                     # u^(1/(e+1))
    (4, U, np.full(N, 1 / 2.2, np.float32), np.power),                     # linearToSRGB, Image.cpp:16
    (4, (16 * U).astype(np.float32), np.full(N, 2.2, np.float32), np.power),  # srgbToLinear, Parser.cpp:72
]


def cpu_eval(fn, x, y):
    L = OracleLib("oracle").lib
    out = np.zeros_like(x)
    yy = x if y is None else y
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.koracle_strictmath(C.c_int(fn), C.c_int(x.size), p(x), p(yy), p(out))
    return out


def ulp_distance(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_within_one_ulp_of_correct_rounding(case):
    fn, x, y, ref = CASES[case]
    got = cpu_eval(fn, x, y)
    want = (ref(x.astype(np.float64)) if y is None else ref(x.astype(np.float64), y.astype(np.float64))).astype(np.float32)
    ok = np.isfinite(want) & (np.abs(want) > 1e-37)  # denormal results: compare absolutely below
    assert ulp_distance(got[ok], want[ok]).max() <= 1
    assert np.abs(got[~ok] - want[~ok]).max(initial=0) <= 1e-37
    # and almost always exactly the correctly rounded value: the binary32 evaluation of sin / cos / asin / acos rounds
    # a value that is itself good to ~0.01 ulp (98.5 % of uniformly drawn arguments; 99.9 % of all binary32 arguments,
    # which crowd towards zero), the binary64 evaluation of pow one that is good to ~1e-4 ulp
    assert np.mean(got[ok] == want[ok]) > (0.999 if fn == 4 else 0.98)


def test_special_values():
    x = np.array([0, 0, 1, 0.5, np.nan, -1, 0, 4], np.float32)
    y = np.array([100, 0, 100, 0, 2, 2, -1, .5], np.float32)
    got = cpu_eval(4, x, y)
    assert got[0] == 0 and got[1] == 1 and got[2] == 1 and got[3] == 1
    assert np.isnan(got[4]) and np.isnan(got[5]) and np.isinf(got[6]) and got[7] == 2
    assert cpu_eval(3, np.array([1, -1], np.float32), None)[0] == 0
    assert np.isnan(cpu_eval(2, np.array([1.0000001], np.float32), None)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
def test_gpu_bits_equal_cpu_bits(case, scenes):
    from kajo_amd import capi
    from kajo_amd.renderer import HipRenderer
    fn, x, y, _ = CASES[case]
    yy = x if y is None else y
    out = np.zeros_like(x)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with HipRenderer(scenes["spheres_a1"], 8, 8, strict=True) as r:
        capi.check(capi.lib().kajo_hip_kat_strictmath(r._h, fn, x.size, p(x), p(yy), p(out)))
    assert np.array_equal(out.view(np.uint32), cpu_eval(fn, x, y).view(np.uint32))


# ---- every binary32: the per-binade checksums -------------------------------------------------------------------------------------

def _load_tables():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strictmath_binades.npz"), allow_pickle=False)
    y = z["ybits"].view(np.float32)
    return {str(n): (int(z["fn"][t]), y[t], z["sums"][t]) for t, n in enumerate(z["names"])}


TABLES = _load_tables()
POW_TABLES = [n for n in TABLES if TABLES[n][0] == 4]
NAN_BITS = np.uint32(0x7fc00000)


def binade_args(b):
    """The 2^23 arguments of binade b = sign * 256 + biased exponent."""
    return ((np.uint32(b) << np.uint32(23)) | np.arange(1 << 23, dtype=np.uint32)).view(np.float32)


def host_eval(fn, x, y):
    """The host's result: the header through the oracle library, the IEEE operations (fn 5, 6) through numpy."""
    with np.errstate(all="ignore"):
        if fn == 5:
            return x / y
        if fn in (6, 7):
            return np.sqrt(x)
    return cpu_eval(fn, x, None if fn < 4 else np.ascontiguousarray(np.broadcast_to(np.asarray(y, np.float32), x.shape)))


def checksums(r):
    """(A, B) of one binade's results r[m], m = 0 .. 2^23 - 1, as the sweep kernel and tools/strictmath_binades.c form them."""
    bits = np.where(np.isnan(r), NAN_BITS, r.view(np.uint32)).astype(np.uint64)
    w = 2 * np.arange(r.size, dtype=np.uint64) + np.uint64(1)
    return np.array([bits.sum(dtype=np.uint64), (bits * w).sum(dtype=np.uint64)], np.uint64)


def same_bits(a, b):
    """Equal bits, a NaN equal to any NaN (sign and payload of a NaN are not part of the contract)."""
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# the subnormal binade, the lowest normal one, the one of 0.5, the one of 1 and pi/2, the top finite one, and the one of -1 and -pi/2
FRESH_BINADES = (0, 1, 126, 127, 254, 256 + 127)


@pytest.mark.parametrize("name", list(TABLES))
def test_fixture_is_what_the_current_header_computes(name):
    fn, y, want = TABLES[name]
    for b in FRESH_BINADES:
        got = checksums(host_eval(fn, binade_args(b), y))
        assert np.array_equal(got, want[b]), \
            "tests/golden/strictmath_binades.npz is stale for %s, binade %d: regenerate it with tools/make_strictmath_binades.py" % (name, b)


# ---- accuracy at the strata the uniform draws above never reach -------------------------------------------------------------------

def _neighbours(v, count=64):
    """The binary32 nearest v and `count` binary32 neighbours on each side of it."""
    c = np.float32(v)
    up, dn = [c], []
    for _ in range(count):
        up.append(np.nextafter(up[-1], np.float32(np.inf)))
        dn.append(np.nextafter(dn[-1] if dn else c, np.float32(-np.inf)))
    return np.array(dn[::-1] + up, np.float32)


def _tiny():
    """The smallest 4096 normal binary32 and subnormals of every exponent (leading bit 0 .. 22, up to 64 mantissas under each)."""
    rng = np.random.default_rng(11)
    normal = np.arange(0x00800000, 0x00800000 + 4096, dtype=np.uint32)
    sub = [np.uint32(1 << p) | rng.integers(0, 1 << p, min(64, 1 << p), dtype=np.uint32) for p in range(23)]
    sub.append(np.array([1, 0x007fffff], np.uint32))
    return np.unique(np.concatenate([normal] + sub)).view(np.float32)


def _strata(fn):
    tiny = _tiny()
    zero = np.array([0.0, -0.0], np.float32)
    if fn in (0, 1):  # documented domain [-2, 6.5]
        parts = [_neighbours(k * np.pi / 2) for k in range(-1, 5)] + [tiny, -tiny, zero]
    elif fn in (2, 3):  # [-1, 1]
        parts = [_neighbours(v) for v in (0.5, -0.5, 1.0, -1.0)] + [tiny, -tiny, zero]
    else:  # pow: x in (0, 1]
        parts = [_neighbours(0.5), _neighbours(1.0), tiny]
    x = np.concatenate(parts)
    lo, hi = {0: (-2, 6.5), 1: (-2, 6.5), 2: (-1, 1), 3: (-1, 1), 4: (0, 1)}[fn]
    x = x[(x >= lo) & (x <= hi)]
    return x[x > 0] if fn == 4 else x


def ulp32_of(v):
    """The binary32 unit in the last place at the binary64 value v (2^-149 in the subnormal range and at zero)."""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


HEADER_POW_Y = [100, 1000, 10, 3, np.float32(2.2), .5, np.float32(1) / np.float32(2.2), np.float32(1) / np.float32(11), np.float32(1) / np.float32(101)]
STRATA_CASES = [(0, None, np.sin), (1, None, np.cos), (2, None, np.arcsin), (3, None, np.arccos)] + [(4, np.float32(y), np.power) for y in HEADER_POW_Y]


@pytest.mark.parametrize("case", range(len(STRATA_CASES)))
def test_within_one_ulp_at_the_reduction_points_the_selects_and_the_tiny_arguments(case):
    """The header's "within 1 ulp of the correctly rounded value", restated against the binary64 value itself -- |got - f64| <= 1.5
    ulp32(f64) -- so that a binary64 near-tie cannot fail a correct result. Arguments: 64 binary32 neighbours on each side of k pi/2,
    k = -1 .. 4 (sin, cos), of +-1/2 and +-1 (asin, acos; 1/2 and 1 for pow), the smallest 4096 normal numbers, subnormals of every
    exponent, and +-0; each on the domain the header documents. (The value only: sin(-0) is +0 here, the reduction's k P2 term being +0.)"""
    fn, y, ref = STRATA_CASES[case]
    x = _strata(fn)
    assert x.size > 4096 + 23 * 32
    got = cpu_eval(fn, x, None if y is None else np.full(x.size, y, np.float32)).astype(np.float64)
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        want = ref(x64) if y is None else ref(x64, np.float64(y))
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got - want) / ulp32_of(want)
    worst = int(np.argmax(err))
    assert err[worst] <= 1.5, (fn, y, float(x[worst]).hex(), got[worst], want[worst], err[worst])


# ---- the device -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def strict_handle(scenes):
    from kajo_amd.renderer import HipRenderer
    with HipRenderer(scenes["spheres_a1"], 8, 8, strict=True) as r:
        yield r


def _name_the_arguments(r, fn, y, binades, limit=4):
    """One mismatching binade, element-wise through kajo_hip_kat_strictmath against the host: the first few arguments that differ."""
    b = int(binades[0])
    x = binade_args(b)
    yy = np.full(x.size, y, np.float32)
    got, want = r.kat_strictmath(fn, x, yy), host_eval(fn, x, yy)
    bad = np.flatnonzero(~same_bits(got, want))[:limit]
    return "%d binades differ (%s ...); in binade %d: " % (len(binades), list(map(int, binades[:8])), b) + "; ".join(
        "x = %s (0x%08x): device %s (0x%08x), host %s (0x%08x)" % (float(x[i]).hex(), x.view(np.uint32)[i], got[i], got.view(np.uint32)[i],
                                                                  want[i], want.view(np.uint32)[i]) for i in bad) + \
        ("" if bad.size else "no element differs through kajo_hip_kat_strictmath: the sweep kernel itself, or the fixture")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in TABLES if n != "sqrt"])
def test_gpu_equals_the_host_at_every_binary32(name, strict_handle):
    """All 2^32 arguments on the device, 512 binades of two checksums against the host build of the same header."""
    fn, y, want = TABLES[name]
    got = strict_handle.kat_strictmath_sweep(fn, y)
    bad = np.flatnonzero((got != want).any(1))
    print("%s: %d binades compared, %d differ" % (name, 512, bad.size))
    assert bad.size == 0, name + ": " + _name_the_arguments(strict_handle, fn, y, bad)


@pytest.mark.gpu
def test_gpu_square_root_is_ieee_at_every_binary32_of_its_domain(strict_handle):
    """ksqrt (integrator.inc.hip) against the IEEE sqrtf: every argument from 2^-96 up (biased exponent >= 31), +inf, the NaNs, every
    negative argument (NaN class; -0 gives -0) and +0. The 31 positive binades below 2^-96 -- 30 normal, one subnormal -- are outside
    its stated domain and are the only ones not asserted; how many of them agree all the same is printed (measured: see the comment
    above ksqrt)."""
    fn, y, want = TABLES["sqrt"]
    got = strict_handle.kat_strictmath_sweep(fn, y)
    differ = (got != want).any(1)
    asserted = np.ones(512, bool)
    asserted[:31] = False
    print("sqrt: %d binades asserted, %d differ; of the 31 binades below 2^-96, %d agree (%s differ)" %
          (asserted.sum(), (differ & asserted).sum(), (~differ[:31]).sum(), np.flatnonzero(differ[:31]).tolist()))
    assert asserted.sum() == 481
    bad = np.flatnonzero(differ & asserted)
    assert bad.size == 0, "sqrt: " + _name_the_arguments(strict_handle, fn, y, bad)
    z = strict_handle.kat_strictmath(6, np.array([0.0, -0.0], np.float32))
    assert z.view(np.uint32).tolist() == [0, 0x80000000]


@pytest.mark.gpu
def test_gpu_square_root_of_the_walk_is_the_same_root_but_for_negative_subnormals(strict_handle):
    """ksqrtWalk (fn 7), the root the sphere tests of the walks form: ksqrt without its select for negative arguments. Every binade
    asserted for ksqrt must agree here too, except the negative subnormal one (binade 256): v_sqrt_f32 flushes such an argument to -0
    and returns -0 where IEEE gives NaN. A discriminant is zero or at least 2^-64 in magnitude under the coordinate range
    kajo_hip_create enforces, so the walks never hold one; -0 itself, in the same binade, gives -0 as IEEE does."""
    _, y, want = TABLES["sqrt"]
    got = strict_handle.kat_strictmath_sweep(7, y)
    differ = (got != want).any(1)
    asserted = np.ones(512, bool)
    asserted[:31] = False
    asserted[256] = False
    print("sqrt of the walk: %d binades asserted, %d differ; the negative subnormal binade %s" %
          (asserted.sum(), (differ & asserted).sum(), "differs" if differ[256] else "agrees"))
    bad = np.flatnonzero(differ & asserted)
    assert bad.size == 0, "sqrt of the walk: " + _name_the_arguments(strict_handle, 7, y, bad)
    z = strict_handle.kat_strictmath(7, np.array([0.0, -0.0, -1e-30, -np.inf], np.float32))
    assert z.view(np.uint32)[:2].tolist() == [0, 0x80000000] and np.isnan(z[2:]).all()


DIV_MANTISSAS = np.array([0, 1, 1 << 22, (1 << 23) - 2, (1 << 23) - 1], np.uint32)
DIV_SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.0, 0.1, 1e-12, 1e12], np.float32)  # (tests/test_hip_exact.py)


def _div_operands(ea, eb, seed):
    """For every (numerator exponent, denominator exponent) pair given: the 5 x 5 mantissa strata and 8 random mantissa pairs, random signs."""
    rng = np.random.default_rng(seed)
    ma, mb = np.meshgrid(DIV_MANTISSAS, DIV_MANTISSAS)
    n = ea.size
    ma = np.concatenate([np.broadcast_to(ma.ravel(), (n, 25)), rng.integers(0, 1 << 23, (n, 8), dtype=np.uint32)], 1)
    mb = np.concatenate([np.broadcast_to(mb.ravel(), (n, 25)), rng.integers(0, 1 << 23, (n, 8), dtype=np.uint32)], 1)
    sa, sb = (rng.integers(0, 2, ma.shape, dtype=np.uint32) << np.uint32(31) for _ in range(2))
    a = (sa | (ea.astype(np.uint32)[:, None] << np.uint32(23)) | ma).ravel().view(np.float32)
    b = (sb | (eb.astype(np.uint32)[:, None] << np.uint32(23)) | mb).ravel().view(np.float32)
    return a, b


def _check_division(r, a, b):
    assert a.size < 4 << 20
    got, want = r.kat_strictmath(5, a, b), host_eval(5, a, b)
    bad = np.flatnonzero(~same_bits(got, want))
    assert bad.size == 0, "%d of %d quotients differ from IEEE; first: " % (bad.size, a.size) + "; ".join(
        "%s / %s: device %s, IEEE %s" % (float(a[i]).hex(), float(b[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:4])


@pytest.mark.gpu
def test_gpu_division_is_ieee_on_every_exponent_pair_of_the_walk(strict_handle):
    """kdiv on every pair of exponents in 2^-47 .. 2^47 -- the operand range the walk relies on (kajo_hip_create's guard keeps scenes
    inside it) -- with the mantissas at the ends and in the middle, random ones, and the special values."""
    e = np.arange(127 - 47, 127 + 48)
    ea, eb = (v.ravel() for v in np.meshgrid(e, e))
    a, b = _div_operands(ea, eb, 21)
    sa, sb = (v.ravel() for v in np.meshgrid(DIV_SPECIAL, DIV_SPECIAL))
    _check_division(strict_handle, np.concatenate([a, sa]), np.concatenate([b, sb]))


@pytest.mark.gpu
def test_gpu_division_is_ieee_on_the_whole_domain_its_comment_states(strict_handle):
    """The domain stated above kdiv, i.e. every operand pair hipcc's v_div_scale would leave alone: a normal denominator of at most
    2^126, exponents fewer than 96 apart, a normal quotient, a numerator of at least 2^-103."""
    ea, eb = (v.ravel() for v in np.meshgrid(np.arange(24, 255), np.arange(1, 253)))
    keep = np.abs(ea - eb) < 96
    a, b = _div_operands(ea[keep], eb[keep], 22)
    # a denominator of exactly 2^126 against the same numerators
    exponent = lambda v: (v.view(np.uint32) >> np.uint32(23) & np.uint32(0xff)).astype(np.int64)
    top = (exponent(b) == 252) & (np.abs(exponent(a) - 253) < 96)
    a, b = np.concatenate([a, a[top]]), np.concatenate([b, np.copysign(np.float32(2.0 ** 126), b[top])])
    q = np.abs(a.astype(np.float64) / b.astype(np.float64))
    normal = (q >= 2.0 ** -126) & (q < 2.0 ** 128 - 2.0 ** 103)  # (the binary64 quotient: below the rounding boundary to infinity)
    _check_division(strict_handle, a[normal], b[normal])


POW_EXTRA_Y = np.array([0.0, -0.0, 1e-30, 1e30, -1e30, 1e-40, np.nan], np.float32)  # (1e-40: a subnormal)
SQRT2_MANTISSA = 0x3504f3  # mantissa of the binary32 below sqrt 2: the m > sqrt 2 select of pow


def _pow_x_grid():
    rng = np.random.default_rng(23)
    m = np.array([0, 1, (1 << 23) - 1] + [SQRT2_MANTISSA + d for d in (-2, -1, 0, 1, 2)], np.uint32)
    e = np.arange(0, 255, dtype=np.uint32)  # 0: subnormals (and, with mantissa 0, zero)
    fixed = ((e[:, None] << np.uint32(23)) | m[None, :]).ravel()
    rand = ((e[:, None] << np.uint32(23)) | rng.integers(0, 1 << 23, (e.size, 16), dtype=np.uint32)).ravel()
    near_one = (0x3f800000 + np.arange(-4, 5)).astype(np.uint32)
    special = np.array([0, 0x80000000, 0x7f800000, 0x7fc00000], np.uint32)  # 0, -0, inf, NaN
    return np.concatenate([fixed, rand, near_one, special]).view(np.float32)


def _check_pow(r, x, y):
    assert x.size < 4 << 20
    got, want = r.kat_strictmath(4, x, y), host_eval(4, x, y)
    bad = np.flatnonzero(~same_bits(got, want))
    assert bad.size == 0, "%d of %d powers differ; first: " % (bad.size, x.size) + "; ".join(
        "pow(%s, %s): device %s (0x%08x), host %s (0x%08x)" % (float(x[i]).hex(), float(y[i]).hex(), got[i], got.view(np.uint32)[i],
                                                             want[i], want.view(np.uint32)[i]) for i in bad[:4])


@pytest.mark.gpu
def test_gpu_pow_equals_the_host_over_exponents_of_x_and_y(strict_handle):
    """pow in both arguments: x at every exponent (subnormals included) with the mantissas at the ends, around the sqrt 2 select and at
    random, 0, inf, NaN and 1 +- 4 ulps; y over the fixture's exponents and +-0, 1e-30, +-1e30, a subnormal and NaN."""
    xs = _pow_x_grid()
    ys = np.concatenate([np.array([TABLES[n][1] for n in POW_TABLES], np.float32), POW_EXTRA_Y])
    x, y = (v.ravel() for v in np.meshgrid(xs, ys))
    _check_pow(strict_handle, np.ascontiguousarray(x), np.ascontiguousarray(y))


def _around(x0, count):
    """`count` consecutive positive binary32 centred on the binary64 value x0 (clipped to the smallest subnormal .. the largest finite)."""
    c = np.float32(min(max(float(x0), 2.0 ** -149), 3.4028234e38)).view(np.uint32).astype(np.int64)
    u = np.clip(c + np.arange(-(count // 2), count - count // 2), 1, 0x7f7fffff)
    return np.unique(u).astype(np.uint32).view(np.float32)


def pow_split_arguments(y, total=4096):
    """x at the floor(t + 0.5) split of pow, t = y log2 x: around every half-integer of t that a positive binary32 x reaches inside the
    +-1100 clamp (at most 2048 of them, evenly picked), the consecutive binary32 that straddle the crossing -- the x NEAREST the
    half-integer on either side. Their t lies within 2^-30 of the half-integer wherever binary32 has such an x at all (a step of x
    moves t by about |y| 2^-24, so for |y| >= 1 a handful of x in all of binary32 come that close and the straddling pair is the
    closest there is); how many do is returned with them."""
    y = float(y)
    lo, hi = sorted((y * -149.0, y * 128.0))
    lo, hi = max(lo, -1100.0), min(hi, 1100.0)
    halves = np.arange(np.ceil(lo - 0.5), np.floor(hi - 0.5) + 1) + 0.5
    if halves.size > total // 2:
        halves = halves[np.linspace(0, halves.size - 1, total // 2).astype(np.int64)]
    per = max(2, total // halves.size)
    with np.errstate(all="ignore"):
        x = np.unique(np.concatenate([_around(np.exp2(h / y), per) for h in halves]))
    t = y * np.log2(x.astype(np.float64))
    return x, int(np.sum(np.abs(t - np.floor(t) - 0.5) <= 2.0 ** -30))


def pow_range_end_arguments(y, total=4096):
    """x whose power falls next to 2^-126 (the smallest normal), 2^-149 (the smallest subnormal) and 2^128 (overflow): at each, consecutive
    binary32 around the x that hits the boundary, and x spread so that the power runs from a quarter to four times the boundary (over
    the gradual underflow to zero, the rounding to the largest finite number and past it)."""
    n = total // 6
    with np.errstate(all="ignore"):
        near = [_around(np.exp2(E / np.float64(y)), n) for E in (-126.0, -149.0, 128.0)]
        wide = [_around(np.exp2((E + d) / np.float64(y)), 1) for E in (-126.0, -149.0, 128.0) for d in np.linspace(-2.0, 2.0, n)]
    return np.unique(np.concatenate(near + wide))


@pytest.mark.gpu
@pytest.mark.parametrize("name", POW_TABLES)
def test_gpu_pow_equals_the_host_at_the_split_and_at_the_ends_of_the_range(name, strict_handle):
    y = TABLES[name][1]
    xs, close = pow_split_arguments(y)
    xe = pow_range_end_arguments(y)
    print("%s: %d arguments at the split (%d within 2^-30 of a half-integer), %d at the ends of the range" % (name, xs.size, close, xe.size))
    x = np.concatenate([xs, xe])
    _check_pow(strict_handle, x, np.full(x.size, y, np.float32))
