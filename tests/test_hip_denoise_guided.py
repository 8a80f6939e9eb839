"""The noise-guided denoiser (include/kajo_hip.h KAJO_DENOISE_NOISE_GUIDED, kajo_hip_denoise_guide_planes;
kajo_amd/csrc/denoise_guided.cpp) on the GPU.

The filter is the plain one with another v0, so the reference is the plain filter's float64 restatement (tests/test_hip_denoise.py) with
v0 handed in: `restate_v0` below repeats that module's iteration loop with its helpers and constants, and every test that uses it first
holds it to the imported `restate` -- with the spatial v0 the two agree to the last bit. `guided_v0` forms the header's v0 from the float32
planes noise() returns. A frame on which no pixel is measured must be the plain filter's bit for bit; one owner with its own records and
three owners with uploaded planes must agree bit for bit; the handle is left as a twin that never denoised."""
import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from test_hip_adaptive import SEED, median_target, unit_slots_of
from test_hip_aov_tiled import _compose
from test_hip_denoise import BUILDS, H3, H5, LUM, MAX_TOL, MEAN_TOL, _rmse, _shift, bits, compare, restate

pytestmark = pytest.mark.gpu


def _prepared(acc, A, passes, samples, demodulate):
    a = np.maximum(A[..., :3] / samples, 1e-3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = acc[..., :3] / passes
        if demodulate:
            e = e / a
    ok = np.isfinite(e).all(-1)
    return np.where(ok[..., None], e, 0.0), ok, a


def spatial_v0(e, ok):
    """the plain definition's v0: the variance of l over the counted pixels of the 3x3 window (tests/test_hip_denoise.py restate)"""
    h, w = ok.shape
    l = e @ LUM
    n, s1, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            lq, m = _shift(l, dx, dy)
            c = m & _shift(ok, dx, dy)[0]
            n += c
            s1 += np.where(c, lq, 0)
            s2 += np.where(c, lq * lq, 0)
    nn = np.maximum(n, 1)
    return np.where(ok, np.maximum(s2 / nn - (s1 / nn) ** 2, 0.0), 0.0)


def guided_v0(e, ok, mean, se):
    """-> (v0, measured): (se / m * l)^2 where the pixel counts, se >= 0, m > 0 and the result is finite; the spatial v0 elsewhere"""
    mean, se = np.asarray(mean, np.float64), np.asarray(se, np.float64)
    l = e @ LUM
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = se / np.where(mean > 0, mean, 1.0) * l
        v = t * t
    measured = ok & (se >= 0) & (mean > 0) & np.isfinite(v)
    return np.where(measured, v, spatial_v0(e, ok)), measured


def restate_v0(acc, A, B, passes, samples, K, v0, sl=4.0, sn=128.0, sd=1.0, demodulate=True):
    """tests/test_hip_denoise.py restate for K >= 1 with v0 an argument (H, W)"""
    acc, A, B = (np.asarray(x, np.float64) for x in (acc, A, B))
    h, w = acc.shape[:2]
    extent = max(w, h)
    nrm = np.sqrt((B[..., :3] ** 2).sum(-1, keepdims=True))
    N = np.where(nrm > 0, B[..., :3] / np.where(nrm > 0, nrm, 1), 0.0)
    z = np.where(A[..., 3] > 0, B[..., 3] / np.where(A[..., 3] > 0, A[..., 3], 1), 0.0)
    e, ok, a = _prepared(acc, A, passes, samples, demodulate)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        l = e @ LUM
        v = np.array(v0, np.float64)
        hasN = (N != 0).any(-1)
        for i in range(K):
            d = 2 ** i
            gs, gw = np.zeros((h, w)), np.zeros((h, w))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    vq, m = _shift(v, dx, dy)
                    c = m & _shift(ok, dx, dy)[0]
                    wt = H3[dx + 1] * H3[dy + 1] * c
                    gs += wt * vq
                    gw += wt
            den_l = sl * np.sqrt(gs / np.where(gw > 0, gw, 1)) + 1e-6
            sw, sv, se = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
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


def restate_guided(acc, A, B, passes, samples, K, mean, se, demodulate=True, **sig):
    """-> (the guided filter's frame in float64, the measured mask). The loop is first held to the imported restatement of the plain
    filter: fed with the spatial v0 it is that function's output, NaN pixels included."""
    e, ok, _ = _prepared(np.asarray(acc, np.float64), np.asarray(A, np.float64), passes, samples, demodulate)
    plain = restate_v0(acc, A, B, passes, samples, K, spatial_v0(e, ok), demodulate=demodulate, **sig)
    assert np.array_equal(plain, restate(acc, A, B, passes, samples, K, demodulate=demodulate, **sig), equal_nan=True)
    v0, measured = guided_v0(e, ok, mean, se)
    return restate_v0(acc, A, B, passes, samples, K, v0, demodulate=demodulate, **sig), measured


def _sig(sigmas):
    return {k: v for k, v in dict(sl=sigmas.get("sigma_luminance"), sn=sigmas.get("sigma_normal"), sd=sigmas.get("sigma_depth")).items()
            if v is not None}


def _parity(r, K, demodulate=True, planes=None, acc=None, **sigmas):
    """(the handle's guided frame, the restatement fed with the handle's accumulation, AOV sums and noise planes, the measured mask)"""
    acc = r.radiance() if acc is None else acc
    aov = r.aov()
    A, B = aov["raw"]
    nz = planes or r.noise()
    got = r.denoise(iterations=K, demodulate=demodulate, noise_guided=True, **sigmas)
    want, measured = restate_guided(acc, A, B, r.passes, aov["samples"], K, nz["mean"], nz["stderr"], demodulate=demodulate, **_sig(sigmas))
    return got, want, measured


def _state_error(call):
    with pytest.raises(capi.KajoError) as e:
        call()
    assert e.value.code == capi.KAJO_E_STATE, e.value
    return str(e.value)


# ---- fallback ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("shape", [(41, 23), (65, 5)], ids=["41x23", "65x5"])
def test_with_no_pixel_measured_it_is_the_plain_filter_bit_for_bit(scenes, shape, build):
    """4 and 6 passes: no pixel has two whole batches, every pixel takes the spatial variance by the plain kernel's expressions."""
    W, H = shape
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, aov=True, noise=True, **BUILDS[build]) as r:
        for more in (4, 2):
            r.render(more)
            nz = r.noise()
            assert not ((nz["stderr"] >= 0) & (nz["mean"] > 0)).any()
            for K in (1, 5, 8):
                for dm in (True, False):
                    plain = r.denoise(iterations=K, demodulate=dm)
                    guided = r.denoise(iterations=K, demodulate=dm, noise_guided=True)
                    why = (r.passes, K, dm)
                    assert np.array_equal(bits(guided["radiance"]), bits(plain["radiance"])), why
                    assert np.array_equal(guided["argb8"], plain["argb8"]), why


# ---- restatement ------------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (3, 2), (65, 5), (41, 23), (100, 75)]
CASES = [(s, "exact") for s in SHAPES] + [((41, 23), "fast"), ((41, 23), "strict")]


@pytest.mark.parametrize("shape,build", CASES, ids=["%dx%d-%s" % (s + (b,)) for s, b in CASES])
def test_measured_pixels_match_the_restatement(scenes, shape, build):
    """8 passes (n = 2) and 16: K = 1, 3, 5, 8 with the default sigmas, and sigma_luminance = 0 once. The project's tolerances for the
    plain filter apply: the arithmetic behind v0 is the same."""
    W, H = shape
    worst = [0.0, 0.0]
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, aov=True, noise=True, **BUILDS[build]) as r:
        for _ in (8, 16):
            r.render(8)
            runs = [(K, True, {}) for K in (1, 3, 5, 8)] + [(3, False, {}), (3, True, dict(sigma_luminance=0.0))]
            for K, dm, sig in runs:
                got, want, measured = _parity(r, K, dm, **sig)
                mean, mx, same = compare(got["radiance"], want, r.passes)
                worst = [max(worst[0], mean), max(worst[1], mx)]
                print("%dx%d %s P=%d K=%d dm=%s %s: mean rel %.2e max rel %.2e, measured %d of %d" %
                      (W, H, build, r.passes, K, dm, sig, mean, mx, measured.sum(), W * H))
                assert same, (r.passes, K, dm, sig)
                assert mean <= MEAN_TOL and mx <= MAX_TOL, (r.passes, K, dm, sig, mean, mx)
                assert np.array_equal(bits(got["radiance"][..., 3]), bits(r.radiance()[..., 3]))
            if r.passes == 16:
                # (if this fails the scene is wrong, not the kernel)
                assert measured.sum() > W * H / 2, (measured.sum(), W * H)
                if W * H > 1:
                    assert not np.array_equal(bits(r.denoise(iterations=3, noise_guided=True)["radiance"]), bits(r.denoise(iterations=3)["radiance"]))
    print("%dx%d %s: mean rel <= %.2e, max rel <= %.2e" % (W, H, build, worst[0], worst[1]))


# ---- owners -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(100, 75), (65, 9)], ids=["100x75", "65x9"])
def test_one_owner_with_its_records_and_three_owners_with_planes_agree_bit_for_bit(scenes, shape):
    W, H = shape
    sc = scenes["spheres_a169"]
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, aov=True, noise=True) as one:
        one.render(16)
        want = one.denoise(noise_guided=True)
        assert not np.array_equal(bits(want["radiance"]), bits(one.denoise()["radiance"]))
        # the source of the words does not matter: the handle's own planes, uploaded, give the records' frame
        nz = one.noise()
        one.denoise_guide_planes(nz["mean"], nz["stderr"])
        again = one.denoise(noise_guided=True)
        assert np.array_equal(bits(again["radiance"]), bits(want["radiance"])) and np.array_equal(again["argb8"], want["argb8"])
        # planes of another pass count give way to the records; dropped planes too
        one.render(4)
        later = one.denoise(noise_guided=True)
        one.denoise_guide_planes(None, None)
        assert np.array_equal(bits(one.denoise(noise_guided=True)["radiance"]), bits(later["radiance"]))
    owners = [HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, aov=True, aov_tiled=True, noise=True, tile_index=i, tile_count=3)
              for i in range(3)]
    try:
        root = owners[0]
        for o in owners:
            o.render(16)
        planes = None
        for o in owners:
            planes = o.noise(out=planes)
        keep = _compose(owners, matte=False)
        # a part-owner without planes
        assert "part of the frame" in _state_error(lambda: root.denoise(noise_guided=True))
        root.denoise_guide_planes(planes["mean"], planes["stderr"])
        got = root.denoise(noise_guided=True)
        assert np.array_equal(bits(got["radiance"]), bits(want["radiance"]))
        assert np.array_equal(got["argb8"], want["argb8"])
        # the plain filter and K = 0 do not look at the planes
        assert np.array_equal(bits(root.denoise(iterations=0, noise_guided=True)["radiance"]), bits(root.radiance()))
        # stale planes
        for o in owners:
            o.render(4)
        del keep
        keep = _compose(owners, matte=False)
        assert "another pass count" in _state_error(lambda: root.denoise(noise_guided=True))
        assert "another pass count" in _state_error(lambda: root.tonemap(denoise=dict(noise_guided=True)))
        assert "another pass count" in _state_error(lambda: root.present(despeckle=dict(), denoise=dict(noise_guided=True)))
        root.denoise(iterations=3)  # (the plain filter is not refused)
        root.denoise_guide_planes(None, None)
        assert "part of the frame" in _state_error(lambda: root.denoise(noise_guided=True))
        planes = None
        for o in owners:
            planes = o.noise(out=planes)
        root.denoise_guide_planes(planes["mean"], planes["stderr"])
        assert np.array_equal(bits(root.denoise(noise_guided=True)["radiance"]), bits(later["radiance"]))
        del keep
    finally:
        for o in owners:
            o.close()


def test_refusals_and_zero_iterations(scenes):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True) as r:
        r.render(8)
        assert "without the noise flag" in _state_error(lambda: r.denoise(noise_guided=True))
        assert "without the noise flag" in _state_error(lambda: r.display(denoise=dict(noise_guided=True), glare=dict()))
        assert "without the noise flag" in _state_error(lambda: r.lens(denoise=dict(noise_guided=True), aperture=0.0))
        # K = 0: the flag is ignored, as demodulation is
        got = r.denoise(iterations=0, noise_guided=True)
        assert np.array_equal(bits(got["radiance"]), bits(r.radiance())) and np.array_equal(got["argb8"], r.argb8())
        with pytest.raises(capi.KajoError) as e:
            r.denoise(iterations=9, noise_guided=True)
        assert e.value.code == capi.KAJO_E_INVALID
        # planes make the handle's own records unnecessary
        with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True, noise=True) as n:
            n.render(8)
            nz = n.noise()
            want = n.denoise(noise_guided=True)
        r.denoise_guide_planes(nz["mean"], nz["stderr"])
        assert np.array_equal(bits(r.denoise(noise_guided=True)["radiance"]), bits(want["radiance"]))
        with pytest.raises(ValueError):
            r.denoise_guide_planes(nz["mean"][:-1], nz["stderr"][:-1])
        # reset drops the planes
        r.reset()
        r.render(8)
        assert "without the noise flag" in _state_error(lambda: r.denoise(noise_guided=True))
    with HipRenderer(sc, 64, 48, spp=4, exact=True, noise=True) as r:
        r.render(8)
        _state_error(lambda: r.denoise(noise_guided=True))  # (no AOVs: what kajo_hip_denoise says)


# ---- adaptive ---------------------------------------------------------------------------------------------------------------------------

def test_an_adaptive_handle_matches_the_restatement_fed_with_its_own_planes(scenes):
    sc, (W, H) = scenes["spheres_a169"], (100, 75)
    with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, exact=True) as t:
        records = [None] * 4 + [t.render(16).noise_moments()]
    target = median_target(records, W, H, unit_slots_of(sc, W, H, exact=True))
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, aov=True, noise=True, adaptive=dict(target=target)) as r:
        r.render(32)
        s = r.adapt_state()
        assert 0 < s["activeUnits"] < s["units"], s
        batches = r.noise()["batches"]
        assert (batches == 4).any() and (batches == 8).any()
        for K in (1, 5):
            got, want, measured = _parity(r, K)
            mean, mx, same = compare(got["radiance"], want, r.passes)
            print("adaptive K=%d: mean rel %.2e max rel %.2e, measured %d of %d" % (K, mean, mx, measured.sum(), W * H))
            assert same and mean <= MEAN_TOL and mx <= MAX_TOL, (K, mean, mx)
            assert measured.sum() > W * H / 2


# ---- chains -----------------------------------------------------------------------------------------------------------------------------

def test_chains_take_the_guided_frame(scenes):
    dn = dict(iterations=3, noise_guided=True)
    copy = dict(aperture=0.0, focus_distance=3.0, max_radius=7)
    ds = dict(factor=2.0, rank=2, floor=0.01)
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, exact=True, aov=True, noise=True) as r:
        r.render(16)
        guided, plain = r.denoise(**dn), r.denoise(iterations=3)
        assert not np.array_equal(guided["argb8"], plain["argb8"])
        # the default tone parameters on the denoised frame are the denoiser's image (tests/test_hip_tonemap.py), through tonemap and
        # through present
        img, s = r.tonemap(denoise=dn)
        assert np.array_equal(img, guided["argb8"]) and s == 1.0
        img, s = r.present(denoise=dn)
        assert np.array_equal(img, guided["argb8"]) and s == 1.0
        for tone in (dict(curve="reinhard", exposure=1.0), dict(curve="aces", auto_exposure=True)):
            a, sa = r.present(denoise=dn, **tone)
            b, sb = r.tonemap(denoise=dn, **tone)
            assert np.array_equal(a, b) and sa == sb, tone
            assert not np.array_equal(a, r.tonemap(denoise=dict(iterations=3), **tone)[0]), tone
        # the chain behind present's other stages: a lens that copies hands out the denoised frame (tests/test_hip_lens.py)
        assert np.array_equal(bits(r.lens(denoise=dn, **copy)), bits(guided["radiance"]))
        # with a despeckle in front the staged frame is filtered, the records still those of the accumulation
        staged = r.despeckle(**ds)["radiance"]
        got = r.lens(despeckle=ds, denoise=dn, **copy)
        aov = r.aov()
        nz = r.noise()
        want, _ = restate_guided(staged, *aov["raw"], r.passes, aov["samples"], 3, nz["mean"], nz["stderr"])
        mean, mx, same = compare(got, want, r.passes)
        print("behind the despeckle: mean rel %.2e max rel %.2e" % (mean, mx))
        assert same and mean <= MEAN_TOL and mx <= MAX_TOL, (mean, mx)


# ---- the handle -------------------------------------------------------------------------------------------------------------------------

def _same_records(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in ("s1", "s2", "n", "bad"))


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_guided_calls_leave_the_handle_as_it_was(scenes, build):
    sc = scenes["spheres_a43"]
    kw = dict(spp=4, aov=True, noise=True, counters=True, **BUILDS[build])
    with HipRenderer(sc, 100, 75, **kw) as a, HipRenderer(sc, 100, 75, **kw) as b:
        a.render(12)
        b.render(12)
        first = a.denoise(noise_guided=True)
        nz = a.noise()
        a.denoise_guide_planes(nz["mean"], nz["stderr"])
        second = a.denoise(noise_guided=True)
        a.present(despeckle=dict(), denoise=dict(iterations=2, noise_guided=True), glare=dict(), curve="reinhard")
        assert np.array_equal(bits(first["radiance"]), bits(second["radiance"])) and np.array_equal(first["argb8"], second["argb8"])
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        assert _same_records(a.noise_moments(), b.noise_moments())
        ca, cb = a.counters(), b.counters()
        assert ca["passes"] == cb["passes"] == 12 and ca["launches"] == cb["launches"] and ca["paths"] == cb["paths"]
        a.render(6)
        b.render(6)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert _same_records(a.noise_moments(), b.noise_moments())
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        # and the guided denoise of the longer session is that of a first call on the twin
        assert np.array_equal(bits(a.denoise(noise_guided=True)["radiance"]), bits(b.denoise(noise_guided=True)["radiance"]))


# ---- does it do its job -----------------------------------------------------------------------------------------------------------------

QUALITY_SEEDS = (SEED, 12345, 777, 20240229)


def test_quality_against_a_converged_frame(scenes):
    """EXACT, spheres.json 16:9 at 320x180, RMSE in clamped display range over the pixels finite in both, as the plain filter's quality test
    forms it. The truth is 64 x 40 = 2560 samples per pixel; the noisy frames are 16 passes of S = 4, four seeds.
    The hard condition: the guided filter moves the truth strictly less than the plain filter does.
    The noisy frame is measured against the plain filter, the parent's code: e_guided <= e_plain * (1 + s), s the relative spread
    (max - min over mean) of e_plain across the seeds. Figures: DESIGN.md section 6p.
    Measured on one MI355X: the truth moves by 0.03909 under the plain filter and by 0.01778 under the guided one (ratio 0.455). Noisy
    frames, per seed (raw, plain, guided): 0.10282 0.04926 0.03936; 0.10044 0.04841 0.03789; 0.10165 0.04823 0.03871; 0.10261 0.04812
    0.03859 -- guided / plain 0.78 .. 0.80, s = 0.0235, 92 % of the pixels measured."""
    sc = scenes["spheres_a169"]
    W, H = 320, 180
    with HipRenderer(sc, W, H, spp=64, exact=True, aov=True, noise=True, seed=12345) as ref:
        ref.render(40)
        truth = ref.radiance()[..., :3] / ref.passes
        ref_plain = ref.denoise()["radiance"][..., :3] / ref.passes
        ref_guided = ref.denoise(noise_guided=True)["radiance"][..., :3] / ref.passes
    fin = np.isfinite(truth).all(-1)
    e_ref_plain, e_ref_guided = _rmse(ref_plain, truth, fin), _rmse(ref_guided, truth, fin)
    print("truth moved by: plain %.5f guided %.5f (ratio %.3f)" % (e_ref_plain, e_ref_guided, e_ref_guided / e_ref_plain))
    rows = []
    for seed in QUALITY_SEEDS:
        with HipRenderer(sc, W, H, spp=4, exact=True, aov=True, noise=True, seed=seed) as r:
            r.render(16)
            raw = r.radiance()[..., :3] / r.passes
            plain = r.denoise()["radiance"][..., :3] / r.passes
            guided = r.denoise(noise_guided=True)["radiance"][..., :3] / r.passes
            nz = r.noise()
        mask = fin & np.isfinite(raw).all(-1)
        assert np.isfinite(plain).all() and np.isfinite(guided).all()
        rows.append((_rmse(raw, truth, mask), _rmse(plain, truth, mask), _rmse(guided, truth, mask)))
        print("seed %d: raw %.5f plain %.5f guided %.5f (guided / plain %.3f), measured %d of %d" %
              ((seed,) + rows[-1] + (rows[-1][2] / rows[-1][1], int(((nz["stderr"] >= 0) & (nz["mean"] > 0)).sum()), W * H)))
    e_plain = np.array([r[1] for r in rows])
    s = float((e_plain.max() - e_plain.min()) / e_plain.mean())
    print("spread of e_plain across the seeds: s = %.4f" % s)
    assert e_ref_guided < e_ref_plain, (e_ref_guided, e_ref_plain)
    for (e_raw, e_p, e_g), seed in zip(rows, QUALITY_SEEDS):
        assert e_g <= e_p * (1 + s), (seed, e_raw, e_p, e_g, s)


# ---- the driver: hip::Scheduler fills the planes from all owners ------------------------------------------------------------------------

import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_one_gpu_and_three_owners_write_the_same_guided_image(scenes, tmp_path):
    """kajo_render --denoise FILE --denoise-noise-guided: the file is HipRenderer.denoise(noise_guided=True)'s image, the same bytes from
    one GPU and from three tiled owners (whose planes the scheduler uploads to the first), through the plain call and through the
    display chain; it differs from the plain filter's; --json reports the measured pixels."""
    sc = scenes["spheres_a169"]
    pod = str(tmp_path / "scene.pod")
    sc.write_pod(pod)

    def run(name, *extra):
        out = str(tmp_path / (name + ".png"))
        cmd = [BIN, "-w", "96", "-h", "54", "--spp", "4", "--passes", "16", "--exact", "--scene-pod", pod, "--json", "-o", "", "--denoise", out, *extra]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (name, p.stderr[-2000:])
        return json.loads(p.stdout.strip().splitlines()[-1]), open(out, "rb").read()

    plain, png_plain = run("plain")
    assert "denoise_noise_guided" not in plain and "denoise_measured_px" not in plain
    one, png1 = run("one", "--denoise-noise-guided")
    three, png3 = run("three", "--denoise-noise-guided", "--gpus", "3", "--same-device", "--aov-tiled")
    assert png1 == png3 and png1 != png_plain
    assert one["denoise_noise_guided"] is True and one["passes"] == three["passes"] == 16
    assert 96 * 54 / 2 < one["denoise_measured_px"] == three["denoise_measured_px"] <= 96 * 54
    with HipRenderer(sc, 96, 54, spp=4, exact=True, aov=True, noise=True) as r:
        r.render(16)
        nz = r.noise()
        assert one["denoise_measured_px"] == int(((nz["stderr"] >= 0) & (nz["mean"] > 0)).sum())
    # through the display chain (a glare in front of the tone curve)
    _, chain1 = run("chain1", "--denoise-noise-guided", "--glare", "0.1")
    _, chain3 = run("chain3", "--denoise-noise-guided", "--glare", "0.1", "--gpus", "3", "--same-device", "--aov-tiled")
    _, chain_plain = run("chainp", "--glare", "0.1")
    assert chain1 == chain3 and chain1 != chain_plain
