"""The glare (bloom) pyramid (include/kajo_hip.h kajo_hip_glare, kajo_hip_display_*; kajo_amd/csrc/glare.hip) on the GPU.

The kernels are held to `restate`, a float64 numpy restatement of the header's definition, over synthetic frames written into the
accumulation through the tile buffer and over rendered frames. Where the definition makes the output a copy (strength 0, no level, a
1x1 frame, no glare parameters) the images must be those of the existing calls bit for bit. Image and scale must not depend on how
many owners the frame was dealt to, and the calls must leave the handle exactly as a twin that never glared.

Tolerance (derived, not tuned): every quantity in the pyramid is a convex sum of non-negative terms, so the relative error of G and B0
is at most the number of float32 roundings on the way times 2^-24 -- under 700 for 12 levels down and up, 4.2e-5. Asserted per channel
at counting pixels: |out - ref| / P <= 1e-4 (|m| + G_ref + B0_ref) + 1e-30; identical bits at the others."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import bits, read_pfm, read_png
from framelib import upload_frame as _upload
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import Scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
LUM = np.array([0.2126, 0.7152, 0.0722])
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
REL_TOL, ABS_TOL = 1e-4, 1e-30


def _reduce_axis(B, axis):
    """One axis of `reduce`: taps 2X - 1 .. 2X + 2 with weights [1, 3, 3, 1], renormalised over the taps inside."""
    B = np.moveaxis(B, axis, 0)
    w = B.shape[0]
    idx = 2 * np.arange((w + 1) // 2)[:, None] + np.arange(-1, 3)[None, :]
    wt = np.array([1.0, 3.0, 3.0, 1.0])[None, :] * ((idx >= 0) & (idx < w))
    taps = B[np.clip(idx, 0, w - 1)]  # (w2, 4, ...)
    shape = wt.shape + (1,) * (B.ndim - 1)
    out = (taps * wt.reshape(shape)).sum(1) / wt.sum(1).reshape((-1,) + (1,) * (B.ndim - 1))
    return np.moveaxis(out, 0, axis)


def _up_axis(U, axis, size):
    """One axis of `up` to `size` samples: the tap at x >> 1 with weight 3, its neighbour towards x with weight 1 where it is inside."""
    U = np.moveaxis(U, axis, 0)
    x = np.arange(size)
    x0 = x >> 1
    x1 = x0 + np.where(x & 1, 1, -1)
    inside = ((x1 >= 0) & (x1 < U.shape[0])).astype(np.float64)
    shape = (-1,) + (1,) * (U.ndim - 1)
    out = (3.0 * U[x0] + inside.reshape(shape) * U[np.clip(x1, 0, U.shape[0] - 1)]) / (3.0 + inside).reshape(shape)
    return np.moveaxis(out, 0, axis)


def _up(U, h, w):
    return _up_axis(_up_axis(U, 1, w), 0, h)


def restate(F, passes, levels=6, strength=0.1, threshold=0.0):
    """include/kajo_hip.h kajo_hip_glare in float64 (the mean m in float32, as the kernels' division forms it): dict(out (H, W, 4) sums
    over passes, counts, m, G, B0, n)."""
    F = np.asarray(F, np.float32)
    H, W = F.shape[:2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m32 = F[..., :3] / np.float32(passes)
        counts = np.isfinite(m32).all(-1)
        m = np.where(counts[..., None], m32.astype(np.float64), 0.0)
    x = np.maximum(m, 0.0)
    l = x @ LUM
    k = np.ones_like(l) if threshold == 0 else np.maximum(l - threshold, 0.0) / np.maximum(l, 1e-6)
    B = [x * k[..., None] * counts[..., None]]
    while len(B) - 1 < levels and (B[-1].shape[0] > 1 or B[-1].shape[1] > 1):
        B.append(_reduce_axis(_reduce_axis(B[-1], 1), 0))
    n = len(B) - 1
    out = F.astype(np.float64)
    G = np.zeros_like(B[0])
    if n > 0:
        U = B[n]
        for lev in range(n - 1, 0, -1):
            U = (B[lev] + (n - lev) * _up(U, *B[lev].shape[:2])) / (n - lev + 1)
        G = _up(U, H, W)
        if strength != 0:
            out[..., :3] = np.where(counts[..., None], (m + strength * (G - B[0])) * passes, out[..., :3])
    return dict(out=out, counts=counts, m=m, G=G, B0=B[0], n=n)


def check_against(got, F, passes, **params):
    """The assertion of the module docstring; -> the largest |out - ref| / P over the allowance (1 = at the bound)."""
    want = restate(F, passes, **params)
    c = want["counts"]
    assert np.array_equal(bits(got[~c]), bits(np.asarray(F, np.float32)[~c])), params  # the pixels that do not count: as they went in
    assert np.array_equal(bits(got[..., 3]), bits(np.asarray(F, np.float32)[..., 3])), params
    assert np.isfinite(got[c][:, :3]).all(), params
    with np.errstate(invalid="ignore"):  # (the pixels that do not count hold NaN / Inf on both sides)
        err = np.abs(got[..., :3].astype(np.float64) - want["out"][..., :3]) / passes
    allow = REL_TOL * (np.abs(want["m"]) + want["G"] + want["B0"]) + ABS_TOL
    ratio = float((err[c] / allow[c]).max()) if c.any() else 0.0
    assert ratio <= 1.0, (params, ratio, np.argwhere((err > allow) & c[..., None])[:5])
    return ratio


def synthetic_frames(W, H, passes):
    """name -> (H, W, 4) float32 sums over `passes`: a constant, one bright pixel in the interior and one in a corner, a checkerboard
    of values spanning 1e-3 .. 1e3, and a frame with NaN, +Inf, -Inf and negative pixels."""
    rng = np.random.default_rng(W * 1000 + H)
    P = np.float32(passes)
    frames = {}
    f = np.empty((H, W, 4), np.float32)
    f[..., :3] = np.float32([0.7, 0.25, 1.3]) * P
    f[..., 3] = 1.0
    frames["constant"] = f
    for name, (px, py) in (("interior", (W // 2, H // 2)), ("corner", (W - 1, 0))):
        f = np.full((H, W, 4), 0.01, np.float32) * P
        f[py, px, :3] = np.float32([900.0, 450.0, 120.0]) * P
        frames[name] = f
    ys, xs = np.mgrid[0:H, 0:W]
    f = (10.0 ** rng.uniform(-3, 0, (H, W, 4))).astype(np.float32)
    f[(xs + ys) % 2 == 1] = (10.0 ** rng.uniform(0, 3, (H, W, 4))).astype(np.float32)[(xs + ys) % 2 == 1]
    frames["checker"] = f * P
    f = (10.0 ** rng.uniform(-2, 1, (H, W, 4))).astype(np.float32) * P
    flat = f.reshape(-1, 4)
    count = W * H
    for i, (pos, ch, v) in enumerate(((0, 0, np.nan), (count // 2, 1, np.inf), (count - 1, 2, -np.inf), (count // 3, 0, -5.0),
                                      (count // 3 + 1, 1, np.nan), (2 * count // 3, 2, -0.5))):
        flat[pos % count, ch] = v
    frames["poisoned"] = f
    return frames


SHAPES = [(1, 1), (2, 1), (7, 5), (41, 23), (65, 9), (130, 70)]
LEVELS = (1, 3, 6, 12)
THRESHOLDS = (0.0, 1.0)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_synthetic_frames_match_the_restatement(scenes, shape):
    """Every synthetic frame x levels 1, 3, 6, 12 x threshold 0, 1 x strength 0.1, 1 at each shape: odd sizes at every level, levels
    beyond what the frame holds, frames smaller than a workgroup and ones of several. NaN / Inf pixels come out with their bits, no
    neighbour becomes non-finite, and the neighbours equal the restatement, which leaves such pixels out."""
    W, H = shape
    passes = 3
    worst = 0.0
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        for name, frame in synthetic_frames(W, H, passes).items():
            _upload(r, frame, passes)
            for levels in LEVELS:
                for threshold in THRESHOLDS:
                    for strength in (0.1, 1.0):
                        params = dict(levels=levels, strength=strength, threshold=threshold)
                        ratio = check_against(r.glare(**params), frame, passes, **params)
                        worst = max(worst, ratio)
            if name == "poisoned" and W * H >= 35:
                counts = restate(frame, passes)["counts"]
                assert 4 <= (~counts).sum() <= 6 and counts.any()  # (the frame does hold pixels of both kinds)
    print("%dx%d: largest |out - ref| / P over its allowance %.4f" % (W, H, worst))


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_a_constant_frame_stays_constant_up_to_the_edges(scenes, shape):
    """c > 0 everywhere: the output is c within 1e-6 relative at every pixel, edges and corners included -- what the renormalisation
    over the taps inside is for (clamped or zero-padded edges would darken or brighten the border)."""
    W, H = shape
    passes = 4
    c = np.float32([0.7, 0.25, 1.3])
    frame = np.empty((H, W, 4), np.float32)
    frame[..., :3] = c * np.float32(passes)
    frame[..., 3] = 2.0
    worst = 0.0
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        _upload(r, frame, passes)
        for levels in LEVELS:
            for strength in (0.1, 1.0):
                out = r.glare(levels=levels, strength=strength)[..., :3].astype(np.float64) / passes
                rel = np.abs(out - c.astype(np.float64)) / c.astype(np.float64)
                worst = max(worst, float(rel.max()))
                assert rel.max() <= 1e-6, (levels, strength, rel.max(), np.argwhere(rel > 1e-6)[:5])
    print("%dx%d: constant frame off by at most %.2e relative" % (W, H, worst))


@pytest.fixture(scope="module")
def rendered(scenes):
    """spheres.json 16:9 at 160x90, EXACT, 3 passes of S = 4 with the AOVs: (accumulation, denoised radiance K = 3); computed once."""
    with HipRenderer(scenes["spheres_a169"], 160, 90, spp=4, exact=True, aov=True) as r:
        r.render(3)
        acc = r.radiance()
        dn = r.denoise(iterations=3)["radiance"]
        glared = {(lv, th): r.glare(levels=lv, threshold=th) for lv in LEVELS for th in THRESHOLDS}
        after = r.glare(levels=6, strength=0.3, threshold=1.0, denoise=dict(iterations=3))
    acc.setflags(write=False)
    dn.setflags(write=False)
    return dict(acc=acc, denoised=dn, glared=glared, after_denoise=after, passes=3)


def test_rendered_frame_matches_the_restatement(rendered):
    worst = 0.0
    for (levels, threshold), got in rendered["glared"].items():
        worst = max(worst, check_against(got, rendered["acc"], rendered["passes"], levels=levels, threshold=threshold))
    print("spheres 160x90: largest |out - ref| / P over its allowance %.4f" % worst)
    # the lights are far brighter than 1: with the default parameters their neighbourhood gains energy
    got = rendered["glared"][(6, 0.0)]
    assert not np.array_equal(bits(got), bits(rendered["acc"]))


def test_glare_after_denoise_is_the_restatement_of_the_denoised_frame(rendered):
    ratio = check_against(rendered["after_denoise"], rendered["denoised"], rendered["passes"], levels=6, strength=0.3, threshold=1.0)
    print("glare after denoise: %.4f of the allowance" % ratio)


TONES = [dict(), dict(curve="reinhard", exposure=1.0, white=2.0), dict(curve="aces", auto_exposure=True)]


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_copy_cases_are_the_existing_calls_bit_for_bit(scenes, build):
    """strength 0, levels 0 and a 1x1 frame: kajo_hip_glare is radiance(), kajo_hip_display_argb8 is kajo_hip_tonemap_argb8, and with
    the default tone parameters the plain resolve -- in every numerics build."""
    for W, H, copies in ((100, 75, [dict(strength=0.0), dict(levels=0), dict(levels=0, strength=0.0, threshold=2.0)]),
                         (1, 1, [dict(), dict(levels=12, strength=1.0)])):
        with HipRenderer(scenes["spheres_a43"], W, H, spp=4, **BUILDS[build]) as r:
            r.render(3)
            acc = r.radiance()
            for g in copies:
                assert np.array_equal(bits(r.glare(**g)), bits(acc)), (W, H, g)
                for tone in TONES:
                    img, s = r.display(glare=g, **tone)
                    want, s_want = r.tonemap(**tone)
                    assert np.array_equal(img, want) and bits(np.float32(s)) == bits(np.float32(s_want)), (W, H, g, tone)
                assert np.array_equal(r.display(glare=g)[0], r.argb8()), (W, H, g)
        # and from the handle's own tiles, before anything composed the float frame
        with HipRenderer(scenes["spheres_a43"], W, H, spp=4, **BUILDS[build]) as r:
            r.render(3)
            assert np.array_equal(r.display(glare=copies[0])[0], r.argb8())


def test_no_glare_parameters_is_the_tone_mapping_bit_for_bit(scenes):
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, exact=True, aov=True) as r:
        r.render(3)
        for tone in TONES:
            for dn in (None, dict(iterations=3), dict(iterations=0)):
                img, s = r.display(denoise=dn, glare=None, **tone)
                want, s_want = r.tonemap(denoise=dn, **tone)
                assert np.array_equal(img, want) and bits(np.float32(s)) == bits(np.float32(s_want)), (tone, dn)


def test_display_is_the_tone_mapping_of_the_glared_frame(scenes):
    """kajo_hip_display_argb8 = the existing tone kernels over kajo_hip_glare's frame: written back into a twin's accumulation, the
    glared frame tone-maps to the same image and the same automatic scale (which is measured after glare)."""
    g = dict(levels=5, strength=0.4, threshold=0.5)
    with HipRenderer(scenes["spheres_a169"], 130, 70, spp=4, exact=True) as r, HipRenderer(scenes["spheres_a169"], 130, 70, spp=4, exact=True) as twin:
        r.render(3)
        glared = r.glare(**g)
        _upload(twin, glared, 3)
        for tone in TONES[1:]:
            img, s = r.display(glare=g, **tone)
            want, s_want = twin.tonemap(**tone)
            assert np.array_equal(img, want) and bits(np.float32(s)) == bits(np.float32(s_want)), tone
        plain, s_plain = r.tonemap(**TONES[2])
        assert s != s_plain or not np.array_equal(img, plain)


def _glare_params(**kw):
    p = capi.KajoGlareParams()
    capi.lib().kajo_hip_default_glare_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _display_gathered(root, gathered, W, H, g, tone):
    """kajo_hip_display_gathered_argb8_device on `root` -> (argb8, scale)."""
    import torch
    L = capi.lib()
    out = torch.empty(W * H, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    capi.check(L.kajo_hip_display_gathered_argb8_device(root._h, src, None if g is None else C.byref(g), C.byref(tone), C.c_void_p(out.data_ptr())))
    scale = root.tone_scale()
    root.wait()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(H, W), scale


def test_image_and_scale_do_not_depend_on_the_owners(scenes):
    """1, 2, 3 and 8 owners gathered on one GPU through the gathered twin, and the whole-frame handle (its tiles, its composed frame):
    the same image bits and, under automatic exposure, the same scale bits; also on a second call and on a twin handle. Ragged frame:
    tiles and workgroups cut by the edges, odd sizes at every level."""
    from test_hip_tonemap import _gathered, _tone_params
    sc = scenes["spheres_a169"]
    W, H = 200, 77
    gl = dict(levels=6, strength=0.25, threshold=0.5)
    case = dict(curve="reinhard", auto_exposure=True)
    g, t = _glare_params(**gl), _tone_params(**case)
    with HipRenderer(sc, W, H, spp=4, exact=True) as r, HipRenderer(sc, W, H, spp=4, exact=True) as twin:
        r.render(3)
        twin.render(3)
        img, s = r.display(glare=gl, **case)
        again, s2 = r.display(glare=gl, **case)
        assert np.array_equal(img, again) and bits(np.float32(s)) == bits(np.float32(s2))
        t_img, t_s = twin.display(glare=gl, **case)
        assert np.array_equal(img, t_img) and bits(np.float32(s)) == bits(np.float32(t_s))
        own, s3 = _display_gathered(r, None, W, H, g, t)
        assert np.array_equal(own, img) and bits(np.float32(s3)) == bits(np.float32(s))
        first = r.glare(**gl)  # composes the float frame: the calls now read it
        assert np.array_equal(bits(first), bits(twin.glare(**gl))) and np.array_equal(bits(first), bits(r.glare(**gl)))
        f_img, f_s = r.display(glare=gl, **case)
        assert np.array_equal(f_img, img) and bits(np.float32(f_s)) == bits(np.float32(s))
        assert not np.array_equal(img, r.tonemap(**case)[0])
        # without glare parameters the gathered twin is kajo_hip_tonemap_gathered_argb8_device
        assert np.array_equal(_display_gathered(r, None, W, H, None, t)[0], r.tonemap(**case)[0])
    for count in (1, 2, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile_index=k, tile_count=count) for k in range(count)]
        try:
            for o in owners:
                o.render(3)
            gathered = _gathered(owners)
            got, gs = _display_gathered(owners[0], gathered, W, H, g, t)
            assert np.array_equal(got, img), count
            assert bits(np.float32(gs)) == bits(np.float32(s)), (count, gs, s)
        finally:
            for o in owners:
                o.close()


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_glare_leaves_the_handle_as_it_was(scenes, build):
    """radiance(), aov() and counters() (kernelMs included) of a handle that glared, displayed and displayed from gathered buffers are
    those of a twin that never did; so are the passes rendered afterwards."""
    from test_hip_tonemap import _tone_params
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as a, \
            HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        a.glare()
        a.glare(levels=12, strength=1.0, threshold=1.0, denoise=dict(iterations=2))
        a.display(glare=dict(), curve="aces", auto_exposure=True)
        a.display(denoise=dict(iterations=3), glare=dict(levels=3), curve="reinhard", exposure=1.0)
        _display_gathered(a, None, 100, 75, _glare_params(), _tone_params("reinhard", auto_exposure=True))
        assert a.counters()["kernelMs"] == ms
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert np.array_equal(a.argb8(), b.argb8())
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        ca, cb = a.counters(), b.counters()
        for key in ("passes", "launches", "paths", "traversals", "vertices"):
            assert ca[key] == cb[key], key
        assert ca["passes"] == 3
        a.render(2)
        b.render(2)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert a.counters()["passes"] == 5
        assert np.array_equal(bits(a.glare()), bits(b.glare()))
        img, s = a.display(glare=dict(), curve="aces", auto_exposure=True)
        t_img, t_s = b.display(glare=dict(), curve="aces", auto_exposure=True)
        assert np.array_equal(img, t_img) and s == t_s


def test_refusals_and_states_on_a_device(scenes):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 64, 48, spp=4, exact=True) as r:
        for call in (r.glare, lambda: r.display(glare=dict())):
            with pytest.raises(capi.KajoError) as e:
                call()
            assert e.value.code == capi.KAJO_E_STATE  # nothing rendered yet
        r.render(1)
        with pytest.raises(capi.KajoError) as e:
            r.glare(denoise={})  # (no AOVs: what kajo_hip_denoise says)
        assert e.value.code == capi.KAJO_E_STATE
        with pytest.raises(capi.KajoError) as e:
            r.glare(levels=13)
        assert e.value.code == capi.KAJO_E_INVALID
        with pytest.raises(capi.KajoError) as e:
            r.display(glare=dict(strength=2.0))
        assert e.value.code == capi.KAJO_E_INVALID
        assert np.isfinite(r.glare(levels=12, strength=1.0)[..., :3]).all()
    with HipRenderer(sc, 64, 48, spp=4, exact=True, tile_index=1, tile_count=2) as part:
        part.render(1)
        for call in (part.glare, lambda: part.display(glare=dict())):
            with pytest.raises(capi.KajoError) as e:
                call()
            assert e.value.code == capi.KAJO_E_STATE


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("gpus", [["--gpus", "1"], ["--gpus", "3", "--same-device"]])
def test_driver_glares_as_the_c_abi(tmp_path, gpus):
    """kajo_render --glare 0.2 --glare-levels 4 --tonemap reinhard: the pixels of HipRenderer.display on the same frame, one owner and
    three gathered on one device; --hdr stays the accumulation / P; --glare 0 writes the image written without the option."""
    scene = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
    out, raw, hdr = str(tmp_path / "o.png"), str(tmp_path / "o.raw"), str(tmp_path / "o.pfm")
    base = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "--json", *gpus]
    p = subprocess.run(base + ["-o", out, "--raw", raw, "--hdr", hdr, "--glare", "0.2", "--glare-levels", "4", "--tonemap", "reinhard", scene],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout.strip().splitlines()[-1])["tone_scale"] == 1.0
    acc = np.fromfile(raw, np.float32).reshape(54, 96, 4)
    png = read_png(out)
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    with HipRenderer(sc, 96, 54, exact=True) as r:
        r.render(2)
        assert np.array_equal(bits(r.radiance()), bits(acc))
        px, _ = r.display(glare=dict(strength=0.2, levels=4), curve="reinhard")
        plain, _ = r.tonemap(curve="reinhard")
    assert not np.array_equal(px, plain)
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (px >> shift) & 255), k
    assert (png[..., 3] == 255).all()
    assert np.array_equal(bits(read_pfm(hdr)), bits(acc[..., :3] / np.float32(2)))
    # --glare 0: the image written without the option
    zero, none = str(tmp_path / "z.png"), str(tmp_path / "n.png")
    for path, extra in ((zero, ["--glare", "0", "--glare-levels", "4"]), (none, [])):
        p = subprocess.run(base + ["-o", path, "--tonemap", "reinhard", *extra, scene], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
    assert np.array_equal(read_png(zero), read_png(none))
    assert np.array_equal(read_png(none)[..., 0], (plain >> 16) & 255)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_glares_the_denoised_image(tmp_path):
    """--denoise FILE with --glare and a tone option writes HipRenderer.display(denoise=..., glare=..., tone)."""
    scene = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
    dn = str(tmp_path / "d.png")
    p = subprocess.run([BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "-o", "", "--denoise", dn, "--glare", "0.2", "--glare-levels", "4",
                        "--glare-threshold", "0.5", "--tonemap", "aces", scene], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")
    with HipRenderer(sc, 96, 54, exact=True, aov=True) as r:
        r.render(2)
        px, _ = r.display(denoise=dict(iterations=5), glare=dict(strength=0.2, levels=4, threshold=0.5), curve="aces")
    png = read_png(dn)
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (px >> shift) & 255), k
