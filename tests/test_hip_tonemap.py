"""Exposure, tone curves and automatic exposure (include/kajo_hip.h kajo_hip_tonemap_argb8; kajo_amd/csrc/tonemap.inc.hip) on the GPU.

The default parameters must be the plain resolve bit for bit -- from a handle's own tiles, from a composed frame, from gathered tile
buffers, from the denoised frame -- in every numerics build. Other parameters are held to `restate`, a float64 numpy restatement of the
header's definition fed with the handle's own accumulation. Image and scale must not depend on how many owners the frame was dealt to, and
the call must leave the handle exactly as a twin that never tone-mapped."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import bits, read_pfm, read_png
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import Scene, stress_scene
from kajo_amd.tiles import TileLayout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
LUM = np.array([0.2126, 0.7152, 0.0722])
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
CURVES = {"clamp": 0, "reinhard": 1, "aces": 2}


def restate(acc, passes, curve="clamp", exposure=0.0, white=0.0, auto_exposure=False, key=0.18):
    """include/kajo_hip.h kajo_hip_tonemap_argb8 in float64 (the mean m in float32, as the kernels' division forms it): (argb8 channels
    (H, W, 3) as int, s)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m32 = acc[..., :3].astype(np.float32) / np.float32(passes)
        counts = np.isfinite(m32).all(-1)
        m = m32.astype(np.float64)
        a = 1.0
        if auto_exposure and counts.any():
            l = np.where(counts[..., None], m, 0.0) @ LUM
            a = key / np.exp(np.mean(np.log(1e-4 + np.maximum(l, 0.0))[counts]))
        s = 2.0 ** exposure * a
        x = m * s
        clamp = np.nan_to_num(np.clip(x, 0.0, 1.0), nan=0.0)
        if curve == "reinhard":
            xc = np.where(counts[..., None], x, 0.0)
            L = xc @ LUM
            Ld = L * (1 + L / white ** 2) / (1 + L) if white > 0 else L / (1 + L)
            y = np.where((L > 0)[..., None], np.clip(xc * (Ld / np.where(L > 0, L, 1.0))[..., None], 0.0, 1.0), 0.0)
        elif curve == "aces":
            xc = np.where(counts[..., None], x, 0.0)
            y = np.clip(xc * (2.51 * xc + 0.03) / (xc * (2.43 * xc + 0.59) + 0.14), 0.0, 1.0)
        else:
            y = clamp
        y = np.where(counts[..., None], y, clamp)
        out = np.floor(y ** (1 / 2.2) * 255 + 0.5).astype(np.int64)
    return out, s


def channels(argb8):
    return np.stack([(argb8 >> 16) & 255, (argb8 >> 8) & 255, argb8 & 255], -1).astype(np.int64)


def _gathered(owners):
    """The owners' tile buffers side by side on the device, as a gather leaves them (torch tensor)."""
    import torch
    from bench import DevicePtr
    parts = []
    for o in owners:
        o.wait()
        ptr, nbytes = o.tile_buffer()
        parts.append(torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").clone())
    torch.cuda.synchronize()  # (the handles run on streams of their own)
    g = torch.cat(parts)
    torch.cuda.synchronize()  # (... and so does the call that reads g: the concatenation on torch's stream must be done before it)
    return g


def _tone_params(curve="clamp", exposure=0.0, white=0.0, auto_exposure=False, key=0.18):
    p = capi.KajoToneParams()
    capi.lib().kajo_hip_default_tone_params(C.byref(p))
    p.curve = CURVES[curve]
    p.flags = capi.KAJO_TONE_AUTO_EXPOSURE if auto_exposure else 0
    p.exposure, p.white, p.key = exposure, white, key
    return p


def _gathered_image(root, gathered, W, H, tone=None, resolve=False):
    """kajo_hip_tonemap_gathered_argb8_device (or, resolve=True, kajo_hip_resolve_gathered_argb8_device) on `root` -> (argb8, scale)."""
    import torch
    L = capi.lib()
    out = torch.empty(W * H, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    scale = None
    if resolve:
        capi.check(L.kajo_hip_resolve_gathered_argb8_device(root._h, src, C.c_void_p(out.data_ptr())))
    else:
        p = tone or _tone_params()
        capi.check(L.kajo_hip_tonemap_gathered_argb8_device(root._h, src, C.byref(p), C.c_void_p(out.data_ptr())))
        scale = root.tone_scale()
    root.wait()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(H, W), scale


def _scene(scenes, which):
    return scenes["spheres_a43"] if which == "small" else stress_scene(scenes["spheres_a169"], 1000, 16)


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("which", ["small", "grid1000"])
def test_default_parameters_are_the_resolve_bit_for_bit(scenes, build, which):
    """Own tiles, composed frame of three owners, gathered buffers: tonemap() with the defaults == argb8(), s = 1."""
    sc = _scene(scenes, which)
    W, H = (100, 75) if which == "small" else (160, 90)
    with HipRenderer(sc, W, H, spp=4, **BUILDS[build]) as r:
        r.render(3).wait()
        img, s = r.tonemap()
        assert s == 1.0
        want = r.argb8()
        assert np.array_equal(img, want)
        own, s = _gathered_image(r, None, W, H)
        assert np.array_equal(own, want) and s == 1.0
        r.radiance()  # composes the float frame: both now read it
        assert np.array_equal(r.tonemap()[0], r.argb8())
    owners = [HipRenderer(sc, W, H, spp=4, tile_index=k, tile_count=3, **BUILDS[build]) for k in range(3)]
    try:
        for o in owners:
            o.render(3)
        g = _gathered(owners)
        resolved, _ = _gathered_image(owners[0], g, W, H, resolve=True)
        mapped, s = _gathered_image(owners[0], g, W, H)
        assert np.array_equal(mapped, resolved) and s == 1.0
        assert np.array_equal(resolved, want)  # (the frame is the same for any tiling)
        owners[0].compose(g.data_ptr())
        img, s = owners[0].tonemap()
        assert np.array_equal(img, owners[0].argb8()) and np.array_equal(img, want) and s == 1.0
    finally:
        for o in owners:
            o.close()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_default_parameters_on_the_denoised_frame_are_the_denoisers_image(scenes, build):
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(3)
        for K in (0, 3, 5):
            img, s = r.tonemap(denoise=dict(iterations=K))
            assert np.array_equal(img, r.denoise(iterations=K)["argb8"]) and s == 1.0, K
        img, _ = r.tonemap(denoise=dict(iterations=2, demodulate=False, sigma_luminance=2.0))
        assert np.array_equal(img, r.denoise(iterations=2, demodulate=False, sigma_luminance=2.0)["argb8"])


CASES = [dict(curve=c, exposure=e) for c in ("clamp", "reinhard", "aces") for e in (-4.0, 0.0, 2.5)] + \
        [dict(curve="reinhard", white=2.0), dict(curve="reinhard", exposure=2.5, white=0.5)] + \
        [dict(curve=c, auto_exposure=True) for c in ("clamp", "reinhard", "aces")] + \
        [dict(curve="reinhard", white=1.5, auto_exposure=True, key=0.5), dict(curve="aces", exposure=-1.0, auto_exposure=True, key=0.09)]


# Share of channels that may be one step off the restatement (none may be further). Measured on one MI355X: 0.0005-0.0007 % in
# test_curves_exposure_and_auto_exposure_match_the_restatement (per build), 0.00007-0.00017 % at the rectangle counts below (EXACT,
# 1x1 .. 3840x2160); the bound, 0.01 %, is about fourteen times the largest.
ONE_OFF = 1e-4


def _against_restatement(r, acc, cases, tag):
    off, total = 0, 0
    for case in cases:
        img, s = r.tonemap(**case)
        want, s_want = restate(acc, r.passes, **case)
        got = channels(img)
        d = np.abs(got - want)
        assert d.max() <= 1, (tag, case, d.max(), np.argwhere(d > 1)[:5])
        assert ((img >> 24) == 255).all()
        assert abs(s - s_want) <= 1e-5 * s_want, (tag, case, s, s_want)
        if not case.get("auto_exposure"):
            assert abs(s - 2.0 ** case.get("exposure", 0.0)) <= 1e-7 * 2.0 ** case.get("exposure", 0.0), (case, s)
        off += int((d == 1).sum())
        total += d.size
    return off, total


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_curves_exposure_and_auto_exposure_match_the_restatement(scenes, build):
    """Every channel within 1 of the float64 restatement, the automatic scale within 1e-5 relative. Measured on one MI355X over these
    cases (spheres.json 4:3 at 160x120, 4 passes of S = 4, and the 1000-sphere scene at 160x90, 1 137 600 channels per build): 6 (EXACT,
    STRICT) and 8 (FAST) channels one off, 0.0005-0.0007 %, none further; at most ONE_OFF (0.01 %) may be one off."""
    off = total = 0
    with HipRenderer(scenes["spheres_a43"], 160, 120, spp=4, **BUILDS[build]) as r:
        r.render(4)
        acc = r.radiance()
        o, t = _against_restatement(r, acc, CASES, "small")
        off, total = off + o, total + t
    with HipRenderer(_scene(scenes, "grid1000"), 160, 90, spp=4, **BUILDS[build]) as r:
        r.render(2)
        acc = r.radiance()
        o, t = _against_restatement(r, acc, CASES[-5:], "grid1000")
        off, total = off + o, total + t
    print("%s: %d of %d channels one off (%.4f %%)" % (build, off, total, 100.0 * off / total))
    assert off <= ONE_OFF * total, (off, total)


def test_non_finite_pixels_are_skipped_and_clamped(scenes):
    """NaN / Inf written into the accumulation: the log-average skips them, and every curve maps them as CLAMP does (the resolve's NaN
    -> 0, +Inf -> 255, -Inf -> 0 per channel)."""
    import torch
    from bench import DevicePtr
    W, H = 100, 75
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        r.render(4).wait()
        ptr, nbytes = r.tile_buffer()
        buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
        xs = np.array([0, 50, 51, 99, 20, 70])
        ys = np.array([0, 30, 30, 74, 60, 10])
        vals = [float("nan"), float("inf"), float("nan"), float("-inf"), float("nan"), float("inf")]
        chs = np.array([0, 1, 2, 0, 1, 2])
        _, slots = TileLayout(W, H, 1).owner_and_slot(xs, ys)
        for sl, v, ch in zip(slots, vals, chs):
            buf[int(sl), ch] = v
        torch.cuda.synchronize()
        acc = r.radiance()
        assert not np.isfinite(acc[ys, xs, :3]).all(-1).any()
        plain = channels(r.argb8())
        for case in (dict(curve="reinhard", auto_exposure=True), dict(curve="aces", auto_exposure=True), dict(curve="clamp", exposure=-2.0)):
            img, s = r.tonemap(**case)
            want, s_want = restate(acc, r.passes, **case)
            assert np.isfinite(s) and abs(s - s_want) <= 1e-5 * s_want, (case, s, s_want)
            got = channels(img)
            assert np.abs(got - want).max() <= 1, case
            # the poisoned channels exactly as CLAMP maps them: NaN and -Inf to 0, +Inf to 255
            assert np.array_equal(got[ys, xs, chs], [0, 255, 0, 0, 0, 255]), (case, got[ys, xs, chs])
        # the default still equals the resolve there
        assert np.array_equal(channels(r.tonemap()[0]), plain)


@pytest.mark.parametrize("case", [dict(curve="reinhard", auto_exposure=True), dict(curve="aces", exposure=1.5, auto_exposure=True, key=0.3)])
def test_image_and_scale_do_not_depend_on_the_owners(scenes, case):
    """1, 2, 3 and 8 owners gathered on one GPU, and the whole-frame handle (its tiles and its composed frame): the same image bits and the
    same scale bits; also on a second call and on a twin handle. Ragged frame: rectangles and tiles cut by the edges."""
    sc = scenes["spheres_a169"]
    W, H = 200, 77
    p = _tone_params(**case)
    with HipRenderer(sc, W, H, spp=4, exact=True) as r, HipRenderer(sc, W, H, spp=4, exact=True) as twin:
        r.render(3)
        twin.render(3)
        img, s = r.tonemap(**case)
        again, s2 = r.tonemap(**case)
        assert np.array_equal(img, again) and bits(np.float32(s)) == bits(np.float32(s2))
        t_img, t_s = twin.tonemap(**case)
        assert np.array_equal(img, t_img) and np.float32(s) == np.float32(t_s)
        own, s3 = _gathered_image(r, None, W, H, tone=p)
        assert np.array_equal(own, img) and np.float32(s3) == np.float32(s)
        r.radiance()  # now from the composed frame
        f_img, f_s = r.tonemap(**case)
        assert np.array_equal(f_img, img) and np.float32(f_s) == np.float32(s)
    for count in (1, 2, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile_index=k, tile_count=count) for k in range(count)]
        try:
            for o in owners:
                o.render(3)
            g = _gathered(owners)
            got, gs = _gathered_image(owners[0], g, W, H, tone=p)
            assert np.array_equal(got, img), count
            assert np.float32(gs) == np.float32(s), (count, gs, s)
        finally:
            for o in owners:
                o.close()


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_tone_mapping_leaves_the_handle_as_it_was(scenes, build):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as a, \
            HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as b:
        a.render(3)
        b.render(3)
        a.tonemap(curve="aces", auto_exposure=True)
        a.tonemap(curve="reinhard", exposure=1.0, denoise=dict(iterations=3))
        _gathered_image(a, None, 100, 75, tone=_tone_params("reinhard", auto_exposure=True))
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert np.array_equal(a.argb8(), b.argb8())
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        ca, cb = a.counters(), b.counters()
        assert ca["passes"] == cb["passes"] == 3 and ca["launches"] == cb["launches"] and ca["paths"] == cb["paths"]
        assert ca["traversals"] == cb["traversals"]
        a.render(2)
        b.render(2)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert a.counters()["passes"] == 5
        img, s = a.tonemap(curve="aces", auto_exposure=True)
        t_img, t_s = b.tonemap(curve="aces", auto_exposure=True)
        assert np.array_equal(img, t_img) and s == t_s


def test_refusals_and_states_on_a_device(scenes):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 64, 48, spp=4, exact=True) as r:
        with pytest.raises(capi.KajoError) as e:
            r.tone_scale()
        assert e.value.code == capi.KAJO_E_STATE
        with pytest.raises(capi.KajoError) as e:
            r.tonemap()
        assert e.value.code == capi.KAJO_E_STATE
        r.render(1)
        with pytest.raises(capi.KajoError) as e:
            r.tonemap(denoise={})  # (no AOVs: what kajo_hip_denoise says)
        assert e.value.code == capi.KAJO_E_STATE
        with pytest.raises(capi.KajoError) as e:
            r.tonemap(exposure=33.0)
        assert e.value.code == capi.KAJO_E_INVALID
        img, s = r.tonemap(exposure=3.0)
        assert s == 8.0 and r.tone_scale() == 8.0
    with HipRenderer(sc, 64, 48, spp=4, exact=True, tile_index=1, tile_count=2) as part:
        part.render(1)
        with pytest.raises(capi.KajoError) as e:
            part.tonemap()
        assert e.value.code == capi.KAJO_E_STATE
        with pytest.raises(capi.KajoError, match="gathered"):
            _gathered_image(part, None, 64, 48)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("gpus", [["--gpus", "1"], ["--gpus", "3", "--same-device"]])
def test_driver_tonemaps_as_the_c_abi(tmp_path, scenes, gpus):
    """kajo_render --tonemap aces --auto-exposure: the pixels and the scale of HipRenderer.tonemap on the same frame, one owner and three
    gathered on one device; --hdr is the accumulation / P in float32; --json reports the scale."""
    out, raw, hdr = str(tmp_path / "o.png"), str(tmp_path / "o.raw"), str(tmp_path / "o.pfm")
    cmd = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "-o", out, "--raw", raw, "--hdr", hdr, "--json", *gpus,
           "--tonemap", "aces", "--auto-exposure", os.path.join(ROOT, "kajo_amd", "data", "caustics.json")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    acc = np.fromfile(raw, np.float32).reshape(54, 96, 4)
    png = read_png(out)
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    with HipRenderer(sc, 96, 54, exact=True) as r:
        r.render(2)
        assert np.array_equal(bits(r.radiance()), bits(acc))
        px, s = r.tonemap(curve="aces", auto_exposure=True)
    assert np.array_equal(png[..., 0], (px >> 16) & 255) and np.array_equal(png[..., 1], (px >> 8) & 255)
    assert np.array_equal(png[..., 2], px & 255) and (png[..., 3] == 255).all()
    assert np.float32(stats["tone_scale"]) == np.float32(s) and s != 1.0
    assert np.array_equal(bits(read_pfm(hdr)), bits(acc[..., :3] / np.float32(2)))


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_default_json_and_denoised_tone(tmp_path, scenes):
    """Without a tone option the JSON line has no tone_scale; --denoise with a tone option writes HipRenderer.tonemap(denoise=...)."""
    base = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "--json", "-o", ""]
    scene = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
    p = subprocess.run(base + [scene], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "tone_scale" not in json.loads(p.stdout.strip().splitlines()[-1])
    dn = str(tmp_path / "d.png")
    p = subprocess.run(base + ["--denoise", dn, "--tonemap", "reinhard", "--exposure", "1.5", "--white", "3", scene], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout.strip().splitlines()[-1])["tone_scale"] == pytest.approx(2 ** 1.5, rel=1e-7)
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")
    with HipRenderer(sc, 96, 54, exact=True, aov=True) as r:
        r.render(2)
        px, _ = r.tonemap(curve="reinhard", exposure=1.5, white=3.0, denoise=dict(iterations=5))
    png = read_png(dn)
    assert np.array_equal(png[..., 0], (px >> 16) & 255) and np.array_equal(png[..., 2], px & 255)


def _rects(W, H):
    return -(-W // 64) * -(-H // 16)


# Frames by their count of 64x16 logavg rectangles, walking kajo_tone_scale through each branch: lane t sums rectangles t, t + 256, ...,
# eight loads at a time while r + 1792 < count, then one at a time. 1: one partial in all; 257: lane 0 sums two, in the remainder loop;
# 1793: lane 0 alone takes the eight-load loop; 2048: every lane takes it once; 2040 (1080p): lanes 0..247 take it; 8100 (4K, BASELINE
# configs[2]): lanes take it three or four times and the remainder loop after. Three of the six frames are taller than wide.
RECT_FRAMES = [(1, 1, 1), (64, 16, 1), (64, 4112, 257), (700, 2600, 1793), (1000, 2048, 2048), (1920, 1080, 2040), (3840, 2160, 8100)]
AUTO_CASES = [dict(curve="clamp", auto_exposure=True), dict(curve="reinhard", white=1.5, auto_exposure=True, key=0.5),
              dict(curve="aces", exposure=-1.0, auto_exposure=True, key=0.09)]


@pytest.mark.parametrize("frame", RECT_FRAMES, ids=["%dx%d" % f[:2] for f in RECT_FRAMES])
def test_rectangle_counts_match_the_restatement(scenes, frame):
    """Every channel within 1 of the float64 restatement and the automatic scale within 1e-5 relative, EXACT, at each rectangle count; at
    most ONE_OFF of the channels one off. Measured on one MI355X (one pass of S = 4, three cases): 0 at 1, 64x16 and 257 rectangles; 24
    of 16 380 000 at 1793, 13 of 18 432 000 at 2048, 31 of 18 662 400 at 2040, 94 of 74 649 600 at 8100."""
    W, H, count = frame
    assert _rects(W, H) == count
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        r.render(1)
        acc = r.radiance()
        off, total = _against_restatement(r, acc, AUTO_CASES, "%dx%d" % (W, H))
    print("%dx%d (%d rectangles): %d of %d channels one off (%.5f %%)" % (W, H, count, off, total, 100.0 * off / total))
    assert off <= ONE_OFF * total, (off, total)


@pytest.mark.parametrize("case", [dict(curve="reinhard", auto_exposure=True), dict(curve="aces", exposure=1.5, auto_exposure=True, key=0.3)])
def test_4k_image_and_scale_do_not_depend_on_the_owners(scenes, case):
    """At 3840x2160 (8100 rectangles): 1, 3 and 8 owners gathered on one GPU and the whole-frame handle, the same image bits and the same
    scale bits."""
    sc = scenes["spheres_a169"]
    W, H = 3840, 2160
    p = _tone_params(**case)
    with HipRenderer(sc, W, H, spp=4, exact=True) as r:
        r.render(1)
        img, s = r.tonemap(**case)
    for count in (1, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile_index=k, tile_count=count) for k in range(count)]
        try:
            for o in owners:
                o.render(1)
            g = _gathered(owners)
            got, gs = _gathered_image(owners[0], g, W, H, tone=p)
            del g
            assert np.array_equal(got, img), count
            assert bits(np.float32(gs)) == bits(np.float32(s)), (count, gs, s)
        finally:
            for o in owners:
                o.close()


def test_all_non_finite_frame(scenes):
    """Every pixel of the accumulation poisoned through the tile buffer: nothing counts, so the log-average is skipped and s is exactly
    2^exposure for every curve; every channel as CLAMP maps it (NaN and -Inf to 0, +Inf to 255), within 1 of the restatement."""
    import torch
    from bench import DevicePtr
    W, H = 100, 75
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        r.render(2).wait()
        ptr, nbytes = r.tile_buffer()
        buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
        buf[:, 0] = float("nan")
        buf[1::2, 1] = float("inf")
        buf[2::3, 2] = float("-inf")
        torch.cuda.synchronize()
        acc = r.radiance()
        assert not np.isfinite(acc[..., :3]).all(-1).any()
        clamp = channels(r.argb8())
        for curve in CURVES:
            for e in (-2.0, 0.0, 1.5):
                case = dict(curve=curve, exposure=e, auto_exposure=True)
                img, s = r.tonemap(**case)
                want, s_want = restate(acc, r.passes, **case)
                assert s == np.float32(2.0 ** e) and s_want == 2.0 ** e, (case, s)  # (the scale is a float32 word)
                got = channels(img)
                assert np.abs(got - want).max() <= 1, case
                if e == 0.0:
                    assert np.array_equal(got, clamp), case
                assert (got[..., 0] == 0).all(), case  # (NaN in every red channel)
