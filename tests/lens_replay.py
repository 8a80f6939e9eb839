"""The depth of field of include/kajo_hip.h (kajo_hip_lens) restated in numpy: what tests/test_hip_lens.py holds kajo_amd/csrc/lens.hip
to. m, z, u, r, d, re and c are formed in float32 exactly as the header writes them, so every comparison and clamp is the kernel's; w and
the sums are formed in float64."""
import numpy as np

F32, F64 = np.float32, np.float64
MAX_RADIUS = 16
DEFAULTS = dict(aperture=0.01, focus_distance=10.0, max_radius=16)
PI_F = F32(np.pi)


def planes(A, B, aperture, focus_distance, max_radius):
    """-> (r, z): the float32 planes of the definition (kajo_hip_lens_coc's). A, B: (H, W, 4) float32 AOV sums."""
    H = A.shape[0]
    a, b = np.ascontiguousarray(A[..., 3], F32), np.ascontiguousarray(B[..., 3], F32)
    with np.errstate(all="ignore"):
        q = b / a
        ok = (a > 0) & np.isfinite(q) & (q > 0)
        z = np.where(ok, q, F32(np.inf)).astype(F32)
        u = np.abs(F32(1.0) - F32(focus_distance) / z)
        r = np.fmin((F32(aperture) * F32(H)) * u, F32(max_radius)).astype(F32)  # (fminf: a NaN product gives maxRadius)
    return r, z


def counting(F, passes):
    """-> (m float32 (H, W, 3), counts bool (H, W))"""
    with np.errstate(all="ignore"):
        m = (np.ascontiguousarray(F[..., :3], F32) / F32(passes)).astype(F32)
    return m, np.isfinite(m).all(-1)


def restate(F, A, B, passes, aperture=DEFAULTS["aperture"], focus_distance=DEFAULTS["focus_distance"], max_radius=DEFAULTS["max_radius"]):
    """-> dict(out float32 (H, W, 4), counts, r, z, scale float64 (H, W, 3) = sum(w |m_q|) / sum(w), the size the error bound is
    relative to, out64 the blurred rgb before it is rounded to float32). aperture == 0: out is F itself."""
    F = np.ascontiguousarray(F, F32)
    H, W = F.shape[:2]
    r, z = planes(A, B, aperture, focus_distance, max_radius)
    m, counts = counting(F, passes)
    if F32(aperture) == 0:
        return dict(out=F.copy(), counts=counts, r=r, z=z, scale=np.abs(m).astype(F64))
    K = int(max_radius)
    # padded planes: a tap outside the image does not count
    mp = np.zeros((H + 2 * K, W + 2 * K, 3), F32)
    mp[K:K + H, K:K + W] = np.where(counts[..., None], m, F32(0))
    cp = np.zeros((H + 2 * K, W + 2 * K), bool)
    cp[K:K + H, K:K + W] = counts
    rp = np.zeros((H + 2 * K, W + 2 * K), F32)
    rp[K:K + H, K:K + W] = r
    zp = np.zeros((H + 2 * K, W + 2 * K), F32)
    zp[K:K + H, K:K + W] = z
    sumW = np.zeros((H, W), F64)
    sums = np.zeros((H, W, 3), F64)
    sabs = np.zeros((H, W, 3), F64)
    one = F32(1.0)
    for dy in range(-K, K + 1):
        for dx in range(-K, K + 1):
            d = np.sqrt(F32(dx * dx + dy * dy)).astype(F32)
            sl = (slice(K + dy, K + dy + H), slice(K + dx, K + dx + W))
            rq, zq, cq = rp[sl], zp[sl], cp[sl]
            re = np.where(zq <= z, rq, np.fmin(rq, r)).astype(F32)
            t = (re + one).astype(F32)
            c = np.minimum(np.maximum((t - d).astype(F32), F32(0)), one)
            c = np.where(cq, c, F32(0))
            if not c.any():
                continue
            re64 = re.astype(F64)
            w = c.astype(F64) / (1.0 + F64(PI_F) * (re64 * (re64 + 1.0)))
            sumW += w
            mq = mp[sl].astype(F64)
            sums += w[..., None] * mq
            sabs += w[..., None] * np.abs(mq)
    out = F.copy()
    with np.errstate(all="ignore"):
        blurred = (sums / sumW[..., None]) * F64(passes)
        scale = sabs / sumW[..., None]
    out[..., :3] = np.where(counts[..., None], blurred.astype(F32), F[..., :3])
    # (the pixels that do not count keep their bits: np.where on float32 copies them)
    keep = ~counts
    out.view(np.uint32)[keep] = F.view(np.uint32)[keep]
    return dict(out=out, out64=blurred, counts=counts, r=r, z=z, scale=scale, sumW=sumW)


def bound(max_radius):
    """the allowance per channel in units of scale: |out - ref| / P <= bound * scale -- two float32 sums of n = (2 maxRadius + 1)^2 terms
    of non-negative weight, plus the weights' own roundings"""
    n = (2 * int(max_radius) + 1) ** 2
    return (n + 16) * 2.0 ** -23


def aov_from_depth(depth, hits=None):
    """A and B (H, W, 4) float32 with B.w / A.w = depth where hits > 0 (hits default 4 everywhere; the quotient is formed by the stage)"""
    depth = np.asarray(depth, F32)
    H, W = depth.shape
    hits = np.full((H, W), 4.0, F32) if hits is None else np.asarray(hits, F32)
    A = np.zeros((H, W, 4), F32)
    B = np.zeros((H, W, 4), F32)
    A[..., :3] = 0.5
    A[..., 3] = hits
    B[..., 2] = 1.0
    with np.errstate(all="ignore"):
        B[..., 3] = depth * hits
    return A, B


def depth_fields(W, H, focus):
    """name -> (depth (H, W) float32, hits (H, W) float32 or None, raw B.w override or None): the depth fields of the tests"""
    f = F32(focus)
    xs = np.arange(W, dtype=F32)[None, :].repeat(H, 0)
    fields = {}
    fields["focus"] = (np.full((H, W), f, F32), None, None)
    fields["twice"] = (np.full((H, W), 2 * f, F32), None, None)
    fields["step_near"] = (np.where(xs < W // 2, f, 4 * f).astype(F32), None, None)      # the near side in focus
    fields["step_far"] = (np.where(xs < W // 2, f / 4, f).astype(F32), None, None)       # the far side in focus
    fields["ramp"] = ((f * (F32(0.25) + F32(3.0) * xs / F32(max(W - 1, 1)))).astype(F32), None, None)  # through the focus distance
    hits = np.full((H, W), 4.0, F32)
    hits[(xs.astype(int) + np.arange(H)[:, None]) % 5 == 0] = 0.0
    fields["holes"] = (np.full((H, W), 2 * f, F32), hits, None)
    raw = np.full((H, W), 2 * f * 4, F32)
    flat = raw.reshape(-1)
    for i, v in enumerate((np.nan, 0.0, -3.0, np.inf)):
        flat[(i * 7 + 1) % flat.size] = v
    fields["poisoned_depth"] = (np.full((H, W), 2 * f, F32), None, raw)
    return fields


def aov_of(field):
    depth, hits, raw = field
    A, B = aov_from_depth(depth, hits)
    if raw is not None:
        B[..., 3] = raw
    return A, B
