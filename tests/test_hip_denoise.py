"""The A-trous denoiser (include/kajo_hip.h kajo_hip_denoise; kajo_amd/csrc/denoise.hip) on the GPU.

The kernels are held to `restate`, a float64 numpy restatement of the header's definition fed with the handle's own accumulation and
AOV sums, and to the image they are meant to approach: a frame of thousands of samples per pixel. K = 0 is the accumulation itself.
The call must leave the handle exactly as a twin that never denoised."""
import numpy as np
import pytest

from framelib import bits
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import stress_scene
from kajo_amd.tiles import TileLayout

pytestmark = pytest.mark.gpu
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
H3 = np.array([1 / 4, 1 / 2, 1 / 4])
LUM = np.array([0.2126, 0.7152, 0.0722])


def _shift(X, ox, oy):
    """(Y, inside): Y[y, x] = X[y + oy, x + ox] where that pixel is inside the image, 0 elsewhere."""
    h, w = X.shape[:2]
    Y = np.zeros_like(X)
    m = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        Y[y0:y1, x0:x1] = X[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        m[y0:y1, x0:x1] = True
    return Y, m


def restate(acc, A, B, passes, samples, K, sl=4.0, sn=128.0, sd=1.0, demodulate=True, extent=None):
    """include/kajo_hip.h kajo_hip_denoise in float64: (H, W, 4) sums over passes. extent: max(W, H) of the whole frame when the arrays
    are a window of it (the depth scale is relative to the frame's larger side); the window's own by default."""
    acc, A, B = (np.asarray(x, np.float64) for x in (acc, A, B))
    if K == 0:
        return acc.copy()
    h, w = acc.shape[:2]
    extent = extent or max(w, h)
    a = np.maximum(A[..., :3] / samples, 1e-3)
    nrm = np.sqrt((B[..., :3] ** 2).sum(-1, keepdims=True))
    N = np.where(nrm > 0, B[..., :3] / np.where(nrm > 0, nrm, 1), 0.0)
    z = np.where(A[..., 3] > 0, B[..., 3] / np.where(A[..., 3] > 0, A[..., 3], 1), 0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = acc[..., :3] / passes
        if demodulate:
            e = e / a
        ok = np.isfinite(e).all(-1)
        e = np.where(ok[..., None], e, 0.0)
        l = e @ LUM
        n = np.zeros((h, w))
        s1 = np.zeros((h, w))
        s2 = np.zeros((h, w))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                lq, m = _shift(l, dx, dy)
                c = m & _shift(ok, dx, dy)[0]
                n += c
                s1 += np.where(c, lq, 0)
                s2 += np.where(c, lq * lq, 0)
        nn = np.maximum(n, 1)
        v = np.where(ok, np.maximum(s2 / nn - (s1 / nn) ** 2, 0.0), 0.0)
        hasN = (N != 0).any(-1)
        for i in range(K):
            d = 2 ** i
            gs = np.zeros((h, w))
            gw = np.zeros((h, w))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    vq, m = _shift(v, dx, dy)
                    c = m & _shift(ok, dx, dy)[0]
                    wt = H3[dx + 1] * H3[dy + 1] * c
                    gs += wt * vq
                    gw += wt
            den_l = sl * np.sqrt(gs / np.where(gw > 0, gw, 1)) + 1e-6
            sw = np.zeros((h, w))
            sv = np.zeros((h, w))
            se = np.zeros((h, w, 3))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    eq, m = _shift(e, dx * d, dy * d)
                    c = m & _shift(ok, dx * d, dy * d)[0]
                    vq = _shift(v, dx * d, dy * d)[0]
                    zq = _shift(z, dx * d, dy * d)[0]
                    Nq = _shift(N, dx * d, dy * d)[0]
                    lq = _shift(l, dx * d, dy * d)[0]
                    wt = np.full((h, w), H5[dx + 2] * H5[dy + 2])
                    if dx or dy:
                        num = np.abs(z - zq)
                        den = sd * np.maximum(np.maximum(z, zq), 1e-4) * np.hypot(dx, dy) * d / extent
                        wt *= np.where(num == 0, 1.0, np.exp(-num / den))
                    dot = np.maximum((N * Nq).sum(-1), 0.0)
                    wt *= np.where(hasN & (Nq != 0).any(-1), dot ** sn, 1.0)
                    num = np.abs(l - lq)
                    wt *= np.where(ok & (num != 0), np.exp(-num / den_l), 1.0)
                    wt = np.where(c, wt, 0.0)
                    sw += wt
                    se += wt[..., None] * eq
                    sv += wt * wt * vq
            ok = sw > 0
            sw1 = np.where(ok, sw, 1)
            e = np.where(ok[..., None], se / sw1[..., None], 0.0)
            v = np.where(ok, sv / sw1 ** 2, 0.0)
            l = e @ LUM
        out = e * a * passes if demodulate else e * passes
    out = np.where(ok[..., None], out, np.nan)
    return np.concatenate([out, acc[..., 3:]], -1)


def compare(got, want, passes):
    """(mean, max) relative difference over the pixels both call finite, and whether the finite masks agree. Relative to the pixel's
    own value, floored at a mean radiance of 1e-2 (values are sums over `passes`)."""
    fg = np.isfinite(got[..., :3]).all(-1)
    fw = np.isfinite(want[..., :3]).all(-1)
    d = np.abs(got[..., :3].astype(np.float64) - want[..., :3])[fw & fg]
    rel = d / np.maximum(np.abs(want[..., :3][fw & fg]), 1e-2 * passes)
    return float(rel.mean()), float(rel.max()), bool(np.array_equal(fg, fw))


def _build(exact=False, strict=False):
    return dict(exact=exact, strict=strict)


BUILDS = {"fast": _build(), "exact": _build(exact=True), "strict": _build(strict=True)}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_zero_iterations_is_the_accumulation_bit_for_bit(scenes, build):
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(3)
        got = r.denoise(iterations=0)
        assert np.array_equal(bits(got["radiance"]), bits(r.radiance()))
        assert np.array_equal(got["argb8"], r.argb8())
        # the demodulation flag does not apply to K = 0
        assert np.array_equal(bits(r.denoise(iterations=0, demodulate=False)["radiance"]), bits(got["radiance"]))


def _parity(r, K, demodulate, **sigmas):
    acc = r.radiance()
    aov = r.aov()
    A, B = aov["raw"]
    got = r.denoise(iterations=K, demodulate=demodulate, **sigmas)
    want = restate(acc, A, B, r.passes, aov["samples"], K, demodulate=demodulate,
                   **{k: v for k, v in dict(sl=sigmas.get("sigma_luminance"), sn=sigmas.get("sigma_normal"),
                                               sd=sigmas.get("sigma_depth")).items() if v is not None})
    return got, want


# measured on one MI355X (EXACT; spheres.json 4:3 at 100x75, 4 passes of S = 4, K = 1..5 with and without demodulation; the 1000-sphere
# scene at 160x90): mean relative difference from the float64 restatement <= 6e-7, largest single channel 3e-5. Over the shapes, builds
# and sigma sets of test_shapes_builds_and_zero_sigmas_match_the_restatement (K = 1..8) and the 1080p windows: mean <= 1.1e-6 (65x5),
# largest 3.6e-5 (45x160 FAST). MEAN_TOL is about nine times the largest mean; MAX_TOL bounds single channels.
MEAN_TOL, MAX_TOL = 1e-5, 1e-3


@pytest.mark.parametrize("demodulate", [True, False])
def test_iterations_match_the_restatement(scenes, demodulate):
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, exact=True, aov=True) as r:
        r.render(4)
        for K in range(1, 6):
            got, want = _parity(r, K, demodulate)
            mean, mx, same = compare(got["radiance"], want, r.passes)
            print("K=%d demodulate=%s: mean rel %.2e max rel %.2e" % (K, demodulate, mean, mx))
            assert same, K
            assert mean <= MEAN_TOL and mx <= MAX_TOL, (K, mean, mx)
            assert np.array_equal(bits(got["radiance"][..., 3]), bits(r.radiance()[..., 3]))


def test_other_sigmas_match_the_restatement(scenes):
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, exact=True, aov=True) as r:
        r.render(2)
        got, want = _parity(r, 3, True, sigma_luminance=1.0, sigma_normal=16.0, sigma_depth=2.0)
        mean, mx, same = compare(got["radiance"], want, r.passes)
        print("sigmas 1/16/2: mean rel %.2e max rel %.2e" % (mean, mx))
        assert same and mean <= MEAN_TOL and mx <= MAX_TOL, (mean, mx)


def test_large_scene_matches_the_restatement(scenes):
    sc = stress_scene(scenes["spheres_a169"], 1000, 16)
    with HipRenderer(sc, 160, 90, spp=4, exact=True, aov=True) as r:
        r.render(2)
        assert r.aov_kernel().endswith("_lg")  # (a grid instance)
        got, want = _parity(r, 5, True)
        mean, mx, same = compare(got["radiance"], want, r.passes)
        print("1000 spheres: mean rel %.2e max rel %.2e" % (mean, mx))
        assert same and mean <= MEAN_TOL and mx <= MAX_TOL, (mean, mx)


def test_nan_and_inf_pixels_are_repaired_not_spread(scenes):
    import torch
    from bench import DevicePtr

    W, H = 100, 75
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True, aov=True) as r:
        r.render(4).wait()
        ptr, nbytes = r.tile_buffer()
        buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
        xs = np.array([0, 50, 51, 99, 20, 70])
        ys = np.array([0, 30, 30, 74, 60, 10])
        vals = [float("nan"), float("inf"), float("nan"), float("-inf"), float("nan"), float("inf")]
        _, slots = TileLayout(W, H, 1).owner_and_slot(xs, ys)
        for s, v, ch in zip(slots, vals, [0, 1, 2, 0, 1, 2]):
            buf[int(s), ch] = v
        torch.cuda.synchronize()
        acc = r.radiance()
        assert not np.isfinite(acc[ys, xs, :3]).all(-1).any()
        for K in (1, 3, 5):
            got, want = _parity(r, K, True)
            out = got["radiance"][..., :3]
            assert np.isfinite(out).all(), (K, np.argwhere(~np.isfinite(out).all(-1)))
            mean, mx, same = compare(got["radiance"], want, r.passes)
            assert same and mean <= MEAN_TOL and mx <= MAX_TOL, (K, mean, mx)
            # the repaired pixels against the restatement, which skips them too
            rel = np.abs(out[ys, xs] - want[ys, xs, :3]) / np.maximum(np.abs(want[ys, xs, :3]), 1e-2 * r.passes)
            assert rel.max() <= MAX_TOL, (K, rel.max())


def _rmse(img, ref, mask):
    return float(np.sqrt(np.mean((np.clip(img, 0, 1) - np.clip(ref, 0, 1))[mask] ** 2)))


def test_quality_against_a_converged_frame(scenes):
    """EXACT, spheres.json 16:9 at 320x180: the default denoise of a 4-spp frame against a reference of 64 x 40 = 2560 samples per pixel,
    in clamped display range over the pixels finite in both. Measured on one MI355X with the defaults: raw 4-spp RMSE 0.273, denoised
    0.088 (ratio 0.323); the reference itself moves by 0.039 when denoised (0.143 x the raw RMSE). tools/denoise_sweep.py: the sweep."""
    sc = scenes["spheres_a169"]
    W, H = 320, 180
    with HipRenderer(sc, W, H, spp=64, exact=True, aov=True, seed=12345) as ref:
        ref.render(40)
        truth = ref.radiance()[..., :3] / ref.passes
        ref_dn = ref.denoise()["radiance"][..., :3] / ref.passes
    with HipRenderer(sc, W, H, spp=4, exact=True, aov=True) as r:
        r.render(1)
        raw = r.radiance()[..., :3] / r.passes
        dn = r.denoise()["radiance"][..., :3] / r.passes
    mask = np.isfinite(truth).all(-1) & np.isfinite(raw).all(-1)
    assert np.isfinite(dn).all() and np.isfinite(ref_dn[np.isfinite(truth).all(-1)]).all()
    e_raw, e_dn, e_ref = _rmse(raw, truth, mask), _rmse(dn, truth, mask), _rmse(ref_dn, truth, mask)
    print("raw %.4f denoised %.4f (ratio %.3f); reference moved by %.4f (%.3f x raw)" % (e_raw, e_dn, e_dn / e_raw, e_ref, e_ref / e_raw))
    assert e_dn <= 0.5 * e_raw, (e_raw, e_dn)
    assert e_ref <= 0.25 * e_raw, (e_raw, e_ref)


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_denoise_leaves_the_handle_as_it_was(scenes, build):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as a, \
            HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as b:
        a.render(3)
        b.render(3)
        first = a.denoise()
        second = a.denoise()
        assert np.array_equal(bits(first["radiance"]), bits(second["radiance"]))
        assert np.array_equal(first["argb8"], second["argb8"])
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert np.array_equal(a.argb8(), b.argb8())
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        ca, cb = a.counters(), b.counters()
        assert ca["passes"] == cb["passes"] == 3 and ca["launches"] == cb["launches"] and ca["paths"] == cb["paths"]
        a.render(2)
        b.render(2)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        # and the denoise of the longer session is that of a fresh call on the twin
        assert np.array_equal(bits(a.denoise()["radiance"]), bits(b.denoise()["radiance"]))


def test_refusals_on_a_device(scenes):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 64, 48, spp=4, exact=True) as r:
        r.render(1)
        with pytest.raises(capi.KajoError) as e:
            r.denoise()
        assert e.value.code == capi.KAJO_E_STATE
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True) as r:
        with pytest.raises(capi.KajoError) as e:
            r.denoise()
        assert e.value.code == capi.KAJO_E_STATE
        r.render(1)
        with pytest.raises(capi.KajoError) as e:
            r.denoise(iterations=9)
        assert e.value.code == capi.KAJO_E_INVALID
        assert np.isfinite(r.denoise(iterations=8)["radiance"][..., :3]).all()


# 1x1 .. 65x5: frames narrower or shorter than the 5x5 footprint and the 64x4 workgroup, single rows and columns, ragged workgroups; 1x97
# and 45x160 are taller than wide (the depth scale is relative to max(W, H)).
SHAPES = [(1, 1), (1, 97), (97, 1), (3, 2), (65, 5), (45, 160)]
# every sigma at 0 in turn, and all three: sigma_depth = 0 keeps only equal depths (exp(-d / 0)), sigma_luminance = 0 leaves a scale of
# 1e-6, sigma_normal = 0 makes every normal weight pow(c, 0) = 1 (c = 0 included)
ZERO_SIGMAS = [dict(sigma_luminance=0.0), dict(sigma_normal=0.0), dict(sigma_depth=0.0),
               dict(sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0)]


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes_builds_and_zero_sigmas_match_the_restatement(scenes, shape, build):
    """K = 1..8 with the default sigmas (demodulated and not), and K = 1, 3, 8 with each zero-sigma set, in each numerics build (the
    kernels are shared; their inputs are not)."""
    W, H = shape
    worst = [0.0, 0.0]
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(3)
        runs = [(K, dm, {}) for K in range(1, 9) for dm in (True, False)] + [(K, True, z) for z in ZERO_SIGMAS for K in (1, 3, 8)]
        for K, dm, sig in runs:
            got, want = _parity(r, K, dm, **sig)
            mean, mx, same = compare(got["radiance"], want, r.passes)
            worst = [max(worst[0], mean), max(worst[1], mx)]
            assert same, (K, dm, sig)
            assert mean <= MEAN_TOL and mx <= MAX_TOL, (K, dm, sig, mean, mx)
            assert np.isfinite(want[..., :3]).any(), (K, dm, sig)
    print("%dx%d %s: mean rel <= %.2e, max rel <= %.2e" % (W, H, build, worst[0], worst[1]))


def test_full_hd_windows_match_the_restatement(scenes):
    """1920x1080, K = 5, EXACT: restated over 128x128 windows at the four corners and the centre, each padded by the filter's dependency
    radius 1 + 2 (2^K - 1) = 63 where the frame goes on; only the window itself is compared (its padding sees a false edge)."""
    W, H, K, win = 1920, 1080, 5, 128
    pad = 1 + 2 * (2 ** K - 1)
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, exact=True, aov=True) as r:
        r.render(2)
        acc = r.radiance()
        aov = r.aov()
        A, B = aov["raw"]
        got = r.denoise(iterations=K)["radiance"]
        passes = r.passes
    worst = [0.0, 0.0]
    for x0, y0 in ((0, 0), (W - win, 0), (0, H - win), (W - win, H - win), ((W - win) // 2, (H - win) // 2)):
        px0, py0 = max(0, x0 - pad), max(0, y0 - pad)
        px1, py1 = min(W, x0 + win + pad), min(H, y0 + win + pad)
        cut = np.s_[py0:py1, px0:px1]
        want = restate(acc[cut], A[cut], B[cut], passes, aov["samples"], K, extent=max(W, H))
        inner = np.s_[y0 - py0:y0 - py0 + win, x0 - px0:x0 - px0 + win]
        mean, mx, same = compare(got[y0:y0 + win, x0:x0 + win], want[inner], passes)
        worst = [max(worst[0], mean), max(worst[1], mx)]
        assert same and mean <= MEAN_TOL and mx <= MAX_TOL, ((x0, y0), mean, mx)
    print("1080p windows: mean rel <= %.2e, max rel <= %.2e" % tuple(worst))
