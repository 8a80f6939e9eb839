"""The local tone mapping of include/kajo_hip.h (kajo_hip_local) restated in numpy, for the tests: the input is the float32 frame in
sums over passes and P; m = F.rgb / P is formed in float32 as the kernels form it, everything after that in float64, with the
definition's tap set, tap order (dy outer, dx inner) and pixel rules. Also the meter's binning (kajo_hip_meter), restated from the
header, for the tests that look at the range a frame spans."""
import numpy as np

F32, F64 = np.float32, np.float64
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F64)
DEFAULTS = dict(iterations=5, compression=0.6, detail=1.0, sigma_range=2.0, pivot=float(F32(np.log2(0.18))))
BINS, BASE = 514, (127 - 16) << 4


def _f32(x):
    """a parameter as the C struct holds it"""
    return F64(F32(x))


def _shift(A, ox, oy):
    """S[y, x] = A[y + oy, x + ox], NaN outside the image"""
    h, w = A.shape
    S = np.full((h, w), np.nan, F64)
    x0, x1 = max(0, -ox), min(w, w - ox)
    y0, y1 = max(0, -oy), min(h, h - oy)
    if x0 < x1 and y0 < y1:
        S[y0:y1, x0:x1] = A[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return S


def mean_and_mask(F, passes):
    """m (float32, as the kernels divide) and the mask of the pixels that count"""
    F = np.asarray(F, F32)
    with np.errstate(all="ignore"):
        m = F[..., :3] / F32(passes)
    return m, np.isfinite(m).all(-1)


def log_luminance(m, counts):
    """L of the definition in float64, NaN where the pixel does not count"""
    x = np.maximum(np.where(counts[..., None], m, 0).astype(F64), 0.0)
    l = (0.2126 * x[..., 0] + 0.7152 * x[..., 1]) + 0.0722 * x[..., 2]
    return np.where(counts, np.log2(np.clip(l, 2.0 ** -16, 2.0 ** 16)), np.nan)


def base_layer(L, iterations, sigma_range):
    """B_K: `iterations` edge-avoiding A-trous passes over L (NaN = a pixel that does not count: never a tap, stays NaN)"""
    sigma = _f32(sigma_range)
    B = L
    counts = ~np.isnan(L)
    for i in range(int(iterations)):
        d = 1 << i
        sw = np.zeros(B.shape, F64)
        sb = np.zeros(B.shape, F64)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                Bq = _shift(B, dx * d, dy * d)
                ok = counts & ~np.isnan(Bq)
                with np.errstate(invalid="ignore"):
                    t = (B - Bq) / sigma
                    wr = np.ones(B.shape, F64) if dx == 0 and dy == 0 else np.exp2(-(t * t))
                w = np.where(ok, (H5[dx + 2] * H5[dy + 2]) * wr, 0.0)
                sw += w
                sb += w * np.where(ok, Bq, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            B = np.where(counts, sb / np.where(counts, sw, 1.0), np.nan)
    return B


def restate(F, passes, iterations=5, compression=0.6, detail=1.0, sigma_range=2.0, pivot=DEFAULTS["pivot"]):
    """-> dict(out (H, W, 4) float64: the definition's output, the input's values where the pixel does not count and in .w; L; B (= B_K);
    counts; m). compression == 1 and detail == 1 is the copy case: out is F."""
    F = np.asarray(F, F32)
    m, counts = mean_and_mask(F, passes)
    L = log_luminance(m, counts)
    out = F.astype(F64)
    if _f32(compression) == 1.0 and _f32(detail) == 1.0:
        return dict(out=out, L=L, B=L, counts=counts, m=m)
    B = base_layer(L, iterations, sigma_range)
    p = _f32(pivot)
    with np.errstate(invalid="ignore"):
        mapped = (p + _f32(compression) * (B - p)) + _f32(detail) * (L - B)
        g = np.exp2(mapped - L)
        rgb = (m.astype(F64) * g[..., None]) * F64(passes)
    out[..., :3] = np.where(counts[..., None], rgb, out[..., :3])
    return dict(out=out, L=L, B=B, counts=counts, m=m)


def meter_bins(F, passes):
    """The histogram kajo_hip_meter takes of a frame (include/kajo_hip.h), (514,) int64: by the bit pattern of the float32 luminance."""
    m, counts = mean_and_mask(F, passes)
    x = np.maximum(m[counts], F32(0))
    l = (F32(0.2126) * x[:, 0] + F32(0.7152) * x[:, 1]) + F32(0.0722) * x[:, 2]
    k = ((l.astype(F32).view(np.uint32) & 0x7FFFFFFF) >> 19).astype(np.int64)
    b = np.where(k < BASE, 0, np.minimum(k - BASE + 1, BINS - 1))
    return np.bincount(b, minlength=BINS)


def span(F, passes):
    """maxBin - minBin of the meter's histogram over bins 1..513 (0 with no metered pixel)"""
    filled = np.flatnonzero(meter_bins(F, passes)[1:])
    return int(filled[-1] - filled[0]) if filled.size else 0


def compare(got, want, passes, counts):
    """(mean, max) relative difference over the counting pixels, as test_hip_denoise.compare: relative to the pixel's own value, floored
    at a mean radiance of 1e-2 (values are sums over `passes`)."""
    if not counts.any():
        return 0.0, 0.0
    with np.errstate(invalid="ignore"):  # (the pixels that do not count hold NaN / Inf on both sides)
        d = np.abs(np.asarray(got)[..., :3].astype(F64) - want[..., :3])[counts]
    rel = d / np.maximum(np.abs(want[..., :3][counts]), 1e-2 * passes)
    return float(rel.mean()), float(rel.max())


def synthetic_frames(W, H, passes):
    """name -> (H, W, 4) float32 sums over `passes`, the frames the glare's tests use, drawn the same way: a constant, one bright pixel
    in the interior and one in a corner, a checkerboard of values spanning 1e-3 .. 1e3, and a frame poisoned with NaN, +Inf, -Inf and
    negative channels."""
    rng = np.random.default_rng(W * 1000 + H)
    P = F32(passes)
    frames = {}
    f = np.empty((H, W, 4), F32)
    f[..., :3] = F32([0.7, 0.25, 1.3]) * P
    f[..., 3] = 1.0
    frames["constant"] = f
    for name, (px, py) in (("interior", (W // 2, H // 2)), ("corner", (W - 1, 0))):
        f = np.full((H, W, 4), 0.01, F32) * P
        f[py, px, :3] = F32([900.0, 450.0, 120.0]) * P
        frames[name] = f
    ys, xs = np.mgrid[0:H, 0:W]
    f = (10.0 ** rng.uniform(-3, 0, (H, W, 4))).astype(F32)
    f[(xs + ys) % 2 == 1] = (10.0 ** rng.uniform(0, 3, (H, W, 4))).astype(F32)[(xs + ys) % 2 == 1]
    frames["checker"] = f * P
    f = (10.0 ** rng.uniform(-2, 1, (H, W, 4))).astype(F32) * P
    flat = f.reshape(-1, 4)
    count = W * H
    for pos, ch, v in ((0, 0, np.nan), (count // 2, 1, np.inf), (count - 1, 2, -np.inf), (count // 3, 0, -5.0), (count // 3 + 1, 1, np.nan),
                       (2 * count // 3, 2, -0.5)):
        flat[pos % count, ch] = v
    frames["poisoned"] = f
    return frames
