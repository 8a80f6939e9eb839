"""Numpy restatements of the grade (include/kajo_hip.h "The grade"; kajo_amd/csrc/grade_math.h, grade.hip), not collected as tests.

spec        the stage's parameters as a plain dict: slope, offset, power (three each), saturation, regions = [dict(objects, amount, and
            the op's keys)]; fill() completes one with the defaults, to_params() makes the KajoGradeParams of it.
masks_of    the regions' masks from read_matte() tables: the selected slots' counts summed in integers and divided ONCE -- in binary64
            for restate64, as float32(sum) / float32(samples) (kajo_hip_matte_mask's words) for restate32.
restate64   the rule in binary64 (numpy's pow) over float32 means, with a running bound of what float32 evaluation may differ by.
restate32   the rule in float32, every step but the power (which numpy cannot restate bit for bit): for specs whose powers are all 1.

The allowance restate64 returns beside its values is DERIVED, step by step, from the rule's own rounding count and the conditioning
of each step, with u = 2^-24 (half an ulp, one float32 rounding):
  v s + o                 E = E_v s + u |v s| + u |v s + o|            a product and a sum
  max(., 0)               E unchanged (1-Lipschitz)
  t^p                     E = the image of [t - E, t + E] under the power (monotone: the exact conditioning, no linearisation)
                              + 2 u t^p                                 kajo_powf is within 1 ulp = 2 u
  l = (a r + b g) + c b   E = a E_r + b E_g + c E_b + u (|a r| + |b g| + |a r + b g| + |c b| + |l|)       five roundings
  l + s (t - l)           E_d = E_t + E_l + u |d|;  E_p = s E_d + u |s d|;  E = E_l + E_p + u |result|
  mask                    E_m = u mask                                  float32(sum) / float32(samples): one rounding (sum < 2^24)
  a = amount mask         E_a = amount E_m + u a
  c + a (op(c) - c)       E_d = E_op + E_c + u |d|;  E_p = a E_d + E_a |d| + u |a d|;  E = E_c + E_p + u |result|
  out = c P, over P       + u |c|
with u |x| read as u |x| + 2^-150 (a rounding among the subnormals), times 1.01 for the second-order terms the lines above leave
out. Nothing in it is tuned."""
import numpy as np

from kajo_amd.renderer import grade_params

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
LUMA = tuple(float(F32(v)) for v in (0.2126, 0.7152, 0.0722))  # the rule's float32 coefficients, as the values they are


def fill(spec=None):
    spec = dict(spec or {})
    three = lambda v, d: [float(F32(x)) for x in np.broadcast_to(np.asarray(d if v is None else v, F64), (3,))]  # (as the struct holds them)
    out = dict(slope=three(spec.get("slope"), 1.0), offset=three(spec.get("offset"), 0.0), power=three(spec.get("power"), 1.0),
               saturation=float(F32(spec.get("saturation", 1.0))))
    out["regions"] = [dict(fill({k: v for k, v in r.items() if k not in ("objects", "amount")}), objects=[int(o) for o in r["objects"]],
                           amount=float(F32(r.get("amount", 1.0)))) for r in spec.get("regions", ())]
    for r in out["regions"]:
        r.pop("regions")
    return out


def to_params(spec):
    """-> capi.KajoGradeParams of a spec"""
    return grade_params(**spec)


def is_identity(spec):
    s = fill(spec)
    return not s["regions"] and s["slope"] == [1.0] * 3 and s["offset"] == [0.0] * 3 and s["power"] == [1.0] * 3 and s["saturation"] == 1.0


def masks_of(ids, counts, samples, regions):
    """ids, counts (..., 8) as read_matte() gives them -> (masks64, masks32), both (..., nRegions)"""
    shape = ids.shape[:-1]
    sums = np.zeros(shape + (len(regions),), np.int64)
    for k, r in enumerate(regions):
        selected = np.isin(ids, np.asarray(r["objects"], np.int64)) & (counts > 0)
        sums[..., k] = np.where(selected, counts.astype(np.int64), 0).sum(-1)
    if samples <= 0:
        return np.zeros(sums.shape, F64), np.zeros(sums.shape, F32)
    assert sums.max(initial=0) < 2 ** 24
    return sums.astype(F64) / F64(samples), (sums.astype(F32) / F32(samples)).astype(F32)


def counting(m):
    return np.isfinite(np.asarray(m, F32)).all(-1)


def R(x):
    """what one float32 rounding of x may move it by: half an ulp, or half the subnormals' spacing"""
    return U * np.abs(x) + 2.0 ** -150


FLT_MAX = float(np.finfo(F32).max)


def _op64(op, v, E, top):
    """-> (value, bound, the largest magnitude any intermediate may have reached)"""
    s, o, p = (np.asarray(op[k], F64) for k in ("slope", "offset", "power"))
    prod = v * s
    t = prod + o
    E = E * s + R(prod) + R(t)
    top = np.maximum(top, (np.maximum(np.abs(prod), np.abs(t)) + E).max(-1))
    t = np.maximum(t, 0.0)
    out, Eout = t.copy(), E.copy()
    for c in range(3):
        if op["power"][c] != 1.0:
            with np.errstate(all="ignore"):
                w = t[..., c] ** p[c]
                hi = (t[..., c] + E[..., c]) ** p[c]
                lo = np.maximum(t[..., c] - E[..., c], 0.0) ** p[c]
            out[..., c] = w
            Eout[..., c] = np.maximum(hi - w, w - lo) + 2 * R(w)
    t, E = out, Eout
    top = np.maximum(top, (np.abs(t) + E).max(-1))
    if op["saturation"] != 1.0:
        a, b, c_ = LUMA
        ab = a * t[..., 0] + b * t[..., 1]
        l = ab + c_ * t[..., 2]
        El = a * E[..., 0] + b * E[..., 1] + c_ * E[..., 2] + (R(a * t[..., 0]) + R(b * t[..., 1]) + R(ab) + R(c_ * t[..., 2]) + R(l))
        sat = op["saturation"]
        d = t - l[..., None]
        Ed = E + El[..., None] + R(d)
        pr = sat * d
        Ep = sat * Ed + R(pr)
        t = l[..., None] + pr
        E = El[..., None] + Ep + R(t)
        top = np.maximum(top, np.maximum((np.abs(d) + Ed).max(-1), np.maximum((np.abs(pr) + Ep).max(-1), (np.abs(t) + E).max(-1))))
    return t, E, top


def restate64(spec, m, masks64=None):
    """m (..., 3) float32 means, masks64 (..., nRegions) -> dict(out64 (..., 3), allowance (..., 3), counts (...)); pixels that do not count
    are left as m (compare their bits apart). ranged (...): the pixel counts and no intermediate can have left float32's range -- where one
    may have, float32 gives +-inf or a NaN that binary64 does not, and only restate32 says what. In the identity case out64 is m and the
    allowance 0."""
    spec = fill(spec)
    m = np.asarray(m, F32)
    cnt = counting(m)
    v = np.where(cnt[..., None], m.astype(F64), 0.0)
    if is_identity(spec):
        return dict(out64=m.astype(F64), allowance=np.zeros(m.shape, F64), counts=cnt, ranged=cnt)
    c, E, top = _op64(spec, v, np.zeros_like(v), np.zeros(v.shape[:-1]))
    for k, r in enumerate(spec["regions"]):
        mask = np.asarray(masks64[..., k], F64)
        Em = R(mask)
        a = r["amount"] * mask
        Ea = r["amount"] * Em + R(a)
        t, Et, top = _op64(r, c, E, top)
        d = t - c
        Ed = Et + E + R(d)
        pr = a[..., None] * d
        Ep = a[..., None] * Ed + Ea[..., None] * np.abs(d) + R(pr)
        c = c + pr
        E = E + Ep + R(c)
        top = np.maximum(top, np.maximum((np.abs(d) + Ed).max(-1), (np.abs(c) + E).max(-1)))
    E = (E + R(c)) * 1.01
    out = np.where(cnt[..., None], c, m.astype(F64))
    with np.errstate(invalid="ignore"):
        ranged = cnt & (top < FLT_MAX)
    return dict(out64=out, allowance=np.where(cnt[..., None], E, 0.0), counts=cnt, ranged=ranged)


def _max0(t):
    return np.where(t > 0, t, F32(0)).astype(F32)


def _op32(op, v):
    assert all(p == 1.0 for p in op["power"]), "the float32 restatement has no power"
    s, o = np.asarray(op["slope"], F32), np.asarray(op["offset"], F32)
    t = _max0((v * s).astype(F32) + o)
    if op["saturation"] != 1.0:
        a, b, c_ = (F32(x) for x in (0.2126, 0.7152, 0.0722))
        l = ((a * t[..., 0]).astype(F32) + (b * t[..., 1]).astype(F32)).astype(F32) + (c_ * t[..., 2]).astype(F32)
        l = l.astype(F32)[..., None]
        t = (l + (F32(op["saturation"]) * (t - l).astype(F32)).astype(F32)).astype(F32)
    return t.astype(F32)


def restate32(spec, m, masks32=None):
    """the rule in float32 over float32 means (every power 1) -> (..., 3) float32, word for word what the stage computes"""
    spec = fill(spec)
    m = np.ascontiguousarray(m, F32)
    if is_identity(spec):
        return m.copy()
    cnt = counting(m)
    with np.errstate(all="ignore"):
        c = _op32(spec, np.where(cnt[..., None], m, F32(0)))
        for k, r in enumerate(spec["regions"]):
            a = (F32(r["amount"]) * np.asarray(masks32[..., k], F32)).astype(F32)[..., None]
            t = _op32(r, c)
            c = (c + (a * (t - c).astype(F32)).astype(F32)).astype(F32)
    out = m.copy()
    out[cnt] = c[cnt]
    return out


def planckian_xy(T):
    """Kim et al. 2002, as the header states it, in binary64"""
    T = float(T)
    if T <= 4000:
        x = -0.2661239e9 / T ** 3 - 0.2343589e6 / T ** 2 + 0.8776956e3 / T + 0.179910
    else:
        x = -3.0258469e9 / T ** 3 + 2.1070379e6 / T ** 2 + 0.2226347e3 / T + 0.240390
    if T <= 2222:
        y = -1.1063814 * x ** 3 - 1.34811020 * x ** 2 + 2.18555832 * x - 0.20219683
    elif T <= 4000:
        y = -0.9549476 * x ** 3 - 1.37418593 * x ** 2 + 2.09137015 * x - 0.16748867
    else:
        y = 3.0817580 * x ** 3 - 5.87338670 * x ** 2 + 3.75112997 * x - 0.37001483
    return x, y


XYZ_TO_SRGB = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]], F64)


def illuminant_rgb(T):
    x, y = planckian_xy(T)
    return XYZ_TO_SRGB @ np.array([x / y, 1.0, (1 - x - y) / y], F64)
