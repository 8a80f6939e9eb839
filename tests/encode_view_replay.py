"""The float view (include/kajo_hip.h "The float view", kajo_amd/csrc/encode_view.cpp) restated in numpy float32 and integers: the front
and the back from tests/encode_replay.py's own pieces, the two sums of tests/view_replay.py over the library's own weight rows (pure host
code: kajo_hip_view_weights). No libm enters between the front and the word: every operation is one IEEE float32 multiply, add or
compare, so the kernels and kajo_hip_encode_view_pixels are held to these words without tolerance. Nothing here calls
kajo_hip_encode_view_pixels or kajo_hip_encode_pixels."""
import numpy as np

import encode_replay as E
import view_replay as V
from kajo_amd.renderer import view_weights

F32 = np.float32

# the covering set of (format, transfer, flags, peak nits, seed, curve, exposure, white) the tests share
CONFIGS = {
    "argb8_gamma22_dither": (E.ARGB8, E.GAMMA22, E.DITHER, 1000.0, 77, E.CLAMP, 0.0, 0.0),
    "rgb10a2_srgb": (E.RGB10A2, E.SRGB, 0, 1000.0, 0, E.REINHARD, 1.5, 0.0),
    "rgba16_pq600_dither": (E.RGBA16, E.PQ, E.DITHER, 600.0, 12345, E.ACES, 0.5, 0.0),
    "rgba16_linear": (E.RGBA16, E.LINEAR, 0, 1000.0, 0, E.REINHARD, -2.25, 4.0),
    "rgba16f": (E.RGBA16F, E.LINEAR, 0, 1000.0, 0, E.ACES, -1.0, 0.0),
    "rgba16f_scene": (E.RGBA16F, E.LINEAR, E.SCENE, 1000.0, 0, E.CLAMP, 3.0, 0.0),
}
CURVE_NAMES = {E.CLAMP: "clamp", E.REINHARD: "reinhard", E.ACES: "aces"}
FORMAT_NAMES = {E.ARGB8: "argb8", E.RGB10A2: "rgb10a2", E.RGBA16: "rgba16", E.RGBA16F: "rgba16f"}
TRANSFER_NAMES = {E.GAMMA22: "gamma22", E.SRGB: "srgb", E.PQ: "pq", E.LINEAR: "linear"}


def encode_kwargs(config):
    """a CONFIGS row -> (kajo_amd.renderer.encode_params' arguments, the tone arguments)"""
    fmt, transfer, flags, peak, seed, curve, exposure, white = config
    return (dict(format=FORMAT_NAMES[fmt], transfer=TRANSFER_NAMES[transfer], dither=bool(flags & E.DITHER), scene=bool(flags & E.SCENE),
                 peak_nits=peak, dither_seed=seed), dict(curve=CURVE_NAMES[curve], exposure=exposure, white=white))


def _scene(fmt, flags):
    return fmt == E.RGBA16F and bool(flags & E.SCENE)


def front(config, mean, scale=None):
    """step 1: (H, W, 3) means -> L (H, W, 3) float32"""
    fmt, _, flags, _, _, curve, exposure, white = config
    m = np.asarray(mean, F32)
    s = E.scale_of(exposure) if scale is None else F32(scale)
    x, y = E.curve(m.reshape(-1, 3), curve, s, white)
    if _scene(fmt, flags):
        with np.errstate(invalid="ignore"):
            v = np.where(x > F32(0), x, F32(0)).astype(F32)
            y = np.where(v < F32(65504), v, F32(65504)).astype(F32)
    return y.reshape(m.shape)


def resample(L, out_w, out_h, rect=None, filter="area"):
    """step 2: L (H, W, 3) -> r (out_h, out_w, 3), the view's own rows, sums in increasing tap order from +0"""
    H, W = L.shape[:2]
    x0, y0, x1, y1 = V.rect_of(W, H, rect)
    fx, cx, wx = view_weights(W, x0, x1, out_w, filter)
    fy, cy, wy = view_weights(H, y0, y1, out_h, filter)
    T = V._axis(np.ascontiguousarray(L, F32), fx, cx, wx)  # [H, out_w, 3]
    return np.swapaxes(V._axis(np.swapaxes(T, 0, 1), fy, cy, wy), 0, 1)  # [out_h, out_w, 3]


def clamp(config, r):
    """step 3"""
    with np.errstate(invalid="ignore"):
        q = np.where(r > F32(0), r, F32(0)).astype(F32)
        top = F32(65504) if _scene(config[0], config[2]) else F32(1)
        return np.where(q < top, q, top).astype(F32)


def back(config, q):
    """step 4: q (out_h, out_w, 3) -> (out_h, out_w) words. encode_replay's steps 4-6 take q where the curve left y: CLAMP at scale 1 is the
    identity on [0, 1], and SCENE's clamp the identity on [0, 65504]. The dither runs over the output's coordinates."""
    fmt, transfer, flags, peak, seed = config[:5]
    h, w = q.shape[:2]
    return E.encode_pixels(fmt, transfer, flags, peak, seed, E.CLAMP, 0.0, 0.0, q.reshape(-1, 3), 0, 0, w, scale=1.0).reshape(h, w)


def restate(config, mean, out_w, out_h, rect=None, filter="area", scale=None):
    """(H, W, 3) means -> (out_h, out_w) words of the format: the definition word for word, the copy case included (it is the identity)"""
    return back(config, clamp(config, resample(front(config, mean, scale), out_w, out_h, rect, filter)))


def plain(config, mean, scale=None):
    """the plain encode of the frame by tests/encode_replay.py: (H, W, 3) -> (H, W) words"""
    fmt, transfer, flags, peak, seed, curve, exposure, white = config
    m = np.asarray(mean, F32)
    h, w = m.shape[:2]
    return E.encode_pixels(fmt, transfer, flags, peak, seed, curve, exposure, white, m.reshape(-1, 3), 0, 0, w, scale=scale).reshape(h, w)


def channels(config, words):
    """the three codes of every word -> (..., 3) int64 (the half format: the binary16 bits, which order as the values do for values >= 0)"""
    fmt = config[0]
    w = np.asarray(words).astype(np.uint64)
    shifts, mask = {E.ARGB8: ((16, 8, 0), 255), E.RGB10A2: ((20, 10, 0), 1023)}.get(fmt, ((0, 16, 32), 65535))
    return np.stack([(w >> np.uint64(s)) & np.uint64(mask) for s in shifts], -1).astype(np.int64)


def out_sizes(W, H):
    """name -> (out_w, out_h, rect): the same size with a fractional sub-rectangle, half the size rounded up, (2W+1) x (2H+1), and one
    output pixel of the whole frame or of a 64-pixel rectangle (the view's largest minification)"""
    return {"same_frac": (W, H, (0.25, 0.25, W - 0.25, H - 0.25)), "half_up": ((W + 1) // 2, (H + 1) // 2, None), "double_plus_1": (2 * W + 1, 2 * H + 1, None),
            "one": (1, 1, (0.0, 0.0, float(min(W, 64)), float(min(H, 64))))}


def frames(W, H, seed=11):
    """name -> (H, W, 3) float32 means: what the tests feed the stage"""
    rng = np.random.default_rng(seed + 1000 * W + H)
    random = (rng.random((H, W, 3)) * 2.0 ** rng.integers(-36, 5, (H, W, 3))).astype(F32)
    wild = random.copy()
    flat = wild.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 65505.0, 1e9, 3e38, -1e-30, 1e-45], F32)
    at = rng.choice(flat.size, min(flat.size, max(len(special), flat.size // 7)), replace=False)
    flat[at] = special[np.arange(at.size) % len(special)]
    out = {"random": random, "wild": wild}
    for name, (x, y) in dict(interior=(W // 2, H // 2), edge=(W - 1, H // 2), corner=(0, 0)).items():
        a = np.zeros((H, W, 3), F32)
        a[y, x] = (8.0, 1.0, 0.5)
        out["bright_" + name] = a
    for k, c in enumerate((0.0, 0.18, 0.7311, 1.0, 2.5)):
        out["const_%d" % k] = np.full((H, W, 3), c, F32) * np.array([1.0, 0.75, 0.5], F32)
    return out
