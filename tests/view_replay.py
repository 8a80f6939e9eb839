"""The view (include/kajo_hip.h "The view", kajo_amd/csrc/view.hip) restated in numpy float32: the library's own weight rows and transfer
tables (pure host code: kajo_hip_view_weights, kajo_hip_view_tables), the two sums in the definition's order, the encode as a count of
thresholds. No libm enters: every operation is one IEEE float32 multiply or add, so the kernels are held to these words bit for bit. Also
float64 restatements of the weights and the tables, which the CPU tests hold the library to."""
import math

import numpy as np

from kajo_amd import capi
from kajo_amd.renderer import view_tables, view_weights

F32, F64 = np.float32, np.float64
FILTERS = ("nearest", "area", "triangle", "lanczos3")


def rect_of(W, H, rect=None):
    return (0.0, 0.0, float(W), float(H)) if rect is None or not any(rect) else tuple(float(F32(v)) for v in rect)


def _axis(lin_rows, first, count, weights):
    """lin_rows [..., srcN, 3] float32 -> [..., outN, 3]: sum over a row's taps in increasing order, accumulators +0"""
    out_n = first.size
    acc = np.zeros(lin_rows.shape[:-2] + (out_n, 3), F32)
    for k in range(weights.shape[1]):
        live = k < count
        j = np.where(live, first + k, first)
        term = weights[:, k][:, None] * lin_rows[..., j, :]
        acc = np.where(live[:, None], acc + term, acc)
    return acc


def restate(image, out_w, out_h, rect=None, filter="area"):
    """(H, W) uint32 0xAARRGGBB -> (out_h, out_w) uint32, the definition word for word (the copy case included: it is the identity)"""
    src = np.ascontiguousarray(image, np.uint32)
    H, W = src.shape
    x0, y0, x1, y1 = rect_of(W, H, rect)
    lin, thr = view_tables()
    fx, cx, wx = view_weights(W, x0, x1, out_w, filter)
    fy, cy, wy = view_weights(H, y0, y1, out_h, filter)
    rgb = np.stack([(src >> 16) & 255, (src >> 8) & 255, src & 255], -1)
    T = _axis(lin[rgb], fx, cx, wx)  # [H, out_w, 3]
    v = _axis(np.swapaxes(T, 0, 1), fy, cy, wy)  # [out_w, out_h, 3]
    code = np.searchsorted(thr, np.swapaxes(v, 0, 1), side="right").astype(np.uint32)
    return np.uint32(0xFF000000) | (code[..., 0] << 16) | (code[..., 1] << 8) | code[..., 2]


def weights64(src_n, a0, a1, out_n, filter):
    """the rows of one axis in float64 -> [(first, [weights])], the header's definition read literally"""
    s = (a1 - a0) / out_n
    S = max(s, 1.0)
    inside = lambda j: int(min(max(j, 0.0), src_n - 1.0))

    def sinc(t):
        if t == 0.0:
            return 1.0
        if t == math.floor(t):
            return 0.0
        return float(np.sin(np.pi * t) / (np.pi * t))

    rows = []
    for i in range(out_n):
        u = a0 + (i + 0.5) * s
        nearest = inside(math.floor(u))
        j0, w = nearest, []
        if filter == "area":
            a, b = a0 + i * s, a0 + (i + 1) * s
            j0, j1 = inside(math.floor(a)), inside(math.ceil(b) - 1.0)
            w = [max(min(b, j + 1.0) - max(a, float(j)), 0.0) for j in range(j0, j1 + 1)]
        elif filter != "nearest":
            R = (1.0 if filter == "triangle" else 3.0) * S
            j0, j1 = inside(math.ceil(u - R - 0.5)), inside(math.floor(u + R - 0.5))
            for j in range(j0, j1 + 1):
                t = (j + 0.5 - u) / S
                if filter == "triangle":
                    w.append(max(1.0 - abs(t), 0.0))
                else:
                    w.append(sinc(t) * sinc(t / 3.0) if abs(t) < 3.0 else 0.0)
        total = 0.0
        for x in w:
            total += x
        w = [x / total for x in w] if total > 0.0 else []
        keep = [k for k, x in enumerate(w) if F32(x) != 0]
        if not keep:
            rows.append((nearest, [1.0]))
        else:
            rows.append((j0 + keep[0], w[keep[0]:keep[-1] + 1]))
    return rows


def tables64():
    c = np.arange(256, dtype=F64)
    return (c / 255.0) ** 2.2, ((c[1:] - 0.5) / 255.0) ** 2.2


def test_images(W, H, seed=7):
    """name -> (H, W) uint32: what the GPU tests feed the stage"""
    rng = np.random.default_rng(seed + 1000 * W + H)
    yy, xx = np.mgrid[0:H, 0:W]
    white, black = np.uint32(0xFFFFFFFF), np.uint32(0xFF000000)
    out = {"random": rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32) | black,
           "checker": np.where((xx + yy) & 1, white, black).astype(np.uint32)}
    for name, (x, y) in dict(interior=(W // 2, H // 2), edge=(W - 1, H // 2), corner=(0, 0)).items():
        a = np.full((H, W), black, np.uint32)
        a[y, x] = white
        out["white_" + name] = a
    for c in (0, 1, 127, 254, 255):
        out["const_%d" % c] = np.full((H, W), 0xFF000000 | c << 16 | c << 8 | c, np.uint32)
    return out
