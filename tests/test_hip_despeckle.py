"""The despeckle stage (include/kajo_hip.h kajo_hip_despeckle, kajo_hip_present_*; kajo_amd/csrc/despeckle.hip) on the GPU.

The kernels are held to `restate`, a numpy float32 restatement of the header's definition with its order of operations, over synthetic
frames written into the accumulation through the tile buffer and over a rendered frame. Every operand of a decision is a float32 IEEE
result, so the SETS of clamped and of repaired pixels and the two counts must equal the restatement's exactly, and a pixel that is
neither carries its input bits. Without despeckle parameters the images are those of the existing calls bit for bit. Image, scale and
counts must not depend on how many owners the frame was dealt to, and the calls leave the handle as a twin that never despeckled.

Changed pixels: a clamped channel is (m * (b / l)) * P, a repaired one (sum of at most 24 terms / n) * P: fewer than 30 float32
roundings, 1.8e-6 relative to the terms' magnitudes, which with a factor 5 gives |out - ref| / P <= 1e-5 * A + 1e-30 per channel, A =
|m * (b / l)| for a clamped pixel and (the sum of |terms|) / n for a repaired one. Measured on one MI355X the kernels' words are simply
the restatement's bits (every operation is one correctly rounded float32 operation on both sides, in the same order), so
`check_against` asserts identical bits, which is the stricter of the two, and still reports the share of the allowance used (0)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import bits, read_pfm, read_png, upload_frame
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import Scene
from kajo_amd.tiles import TileLayout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
REL_TOL, ABS_TOL = 1e-5, 1e-30
F32 = np.float32
RING = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]  # row-major


def _mean_and_luminance(F, passes):
    with np.errstate(invalid="ignore", over="ignore"):
        m = F[..., :3] / F32(passes)
        counts = np.isfinite(m).all(-1)
        x = np.maximum(m, F32(0))
        l = (F32(0.2126) * x[..., 0] + F32(0.7152) * x[..., 1]) + F32(0.0722) * x[..., 2]
    return m, counts, l


def _defaults():
    p = capi.KajoDespeckleParams()
    capi.lib().kajo_hip_default_despeckle_params(C.byref(p))
    return dict(factor=p.factor, rank=p.rank, floor=p.floor)


CLASSIC = dict(factor=4.0, rank=2, floor=0.05)  # the setting the properties below are stated for, whatever the defaults are


def restate(F, passes, factor=None, rank=None, floor=None):
    """include/kajo_hip.h kajo_hip_despeckle in numpy float32, operation for operation: dict(out (H, W, 4) float32, clamped and repaired
    (H, W) bool, allow (H, W, 3) float64 = the A of the module docstring at the changed pixels). Arguments left None: the library's defaults."""
    d = _defaults()
    factor, rank, floor = (d[k] if v is None else v for k, v in (("factor", factor), ("rank", rank), ("floor", floor)))
    F = np.ascontiguousarray(F, F32)
    H, W = F.shape[:2]
    P = F32(passes)
    m, counts, l = _mean_and_luminance(F, passes)
    allow = np.zeros((H, W, 3))
    C_ = F.copy()
    clamped = np.zeros((H, W), bool)
    if factor != 0:
        pad = np.full((H + 2, W + 2), F32(-1))
        pad[1:-1, 1:-1] = np.where(counts, l, F32(-1))
        nb = np.stack([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dx, dy in RING], -1)
        n = (nb >= 0).sum(-1)
        srt = -np.sort(-nb, axis=-1)  # descending
        r = np.clip(np.minimum(rank, n), 1, 8)
        Lr = np.take_along_axis(srt, (r - 1)[..., None], -1)[..., 0]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            b = F32(factor) * np.maximum(Lr, F32(floor))
            clamped = counts & (n >= 3) & (l > b)
            s = b / l
            scaled = m * s[..., None]
            C_[..., :3] = np.where(clamped[..., None], scaled * P, F[..., :3])
        assert b.dtype == F32 and scaled.dtype == F32
        allow[clamped] = np.abs(scaled[clamped].astype(np.float64))
    mC, countsC, _ = _mean_and_luminance(C_, passes)
    out = C_.copy()
    repaired = np.zeros((H, W), bool)
    for y, x in np.argwhere(~countsC):
        for reach in (1, 2):
            total, mag, k = np.zeros(3, F32), np.zeros(3), 0
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    qx, qy = x + dx, y + dy
                    if (dx or dy) and 0 <= qx < W and 0 <= qy < H and countsC[qy, qx]:
                        total = total + mC[qy, qx]
                        mag += np.abs(mC[qy, qx].astype(np.float64))
                        k += 1
            if k:
                with np.errstate(over="ignore"):
                    out[y, x, :3] = (total / F32(k)) * P
                repaired[y, x] = True
                allow[y, x] = mag / k
                break
    return dict(out=out, clamped=clamped, repaired=repaired, allow=allow)


def check_against(got, F, passes, **params):
    """got = HipRenderer.despeckle()'s dict. The assertions of the module docstring; -> (the largest |out - ref| / P over its allowance,
    the number of changed words whose bits differ from the restatement's)."""
    F = np.ascontiguousarray(F, F32)
    want = restate(F, passes, **params)
    out = got["radiance"]
    changed = want["clamped"] | want["repaired"]
    moved = (bits(out[..., :3]) != bits(F[..., :3])).any(-1)
    assert not (moved & ~changed).any(), (params, np.argwhere(moved & ~changed)[:5])  # every other pixel: the bits it went in with
    assert np.array_equal(bits(out[..., 3]), bits(F[..., 3])), params
    assert (got["clamped"], got["repaired"]) == (int(want["clamped"].sum()), int(want["repaired"].sum())), params
    # the sets: a clamped pixel is one that counts and came out changed, a repaired pixel one that did not count and came out finite
    _, counts, _ = _mean_and_luminance(F, passes)
    with np.errstate(invalid="ignore", over="ignore"):
        finite_out = np.isfinite(out[..., :3] / F32(passes)).all(-1)
    assert np.array_equal(~counts & finite_out, want["repaired"]), params
    differ = bits(out[..., :3]) != bits(want["out"][..., :3])
    assert not (differ.any(-1) & ~changed).any(), params
    assert not (want["clamped"] & ~moved & (bits(want["out"][..., :3]) != bits(F[..., :3])).any(-1)).any(), params  # clamped pixels did change
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(out[..., :3].astype(np.float64) - want["out"][..., :3].astype(np.float64)) / passes
    allow = REL_TOL * want["allow"] + ABS_TOL
    ok = np.isfinite(err) | ~changed[..., None]
    assert ok.all(), (params, np.argwhere(~ok)[:5])
    ratio = float((err[changed] / allow[changed]).max()) if changed.any() else 0.0
    print("   %s: %d clamped, %d repaired, %.4f of the allowance, %d words differ in bits" % (params, got["clamped"], got["repaired"], ratio, int(differ.sum())))
    assert ratio <= 1.0, (params, ratio, np.argwhere((err > allow) & changed[..., None])[:5])
    assert not differ.any(), (params, np.argwhere(differ)[:5])
    return ratio, int(differ.sum())


def _upload(r, frame, passes, tile=(64, 16)):
    """framelib.upload_frame behind a wait for the handle's own work (this file writes into handles that have just rendered or filtered)"""
    r.wait()
    upload_frame(r, frame, passes, tile)


SPIKE = F32([900.0, 450.0, 120.0])


def _background(W, H, passes, rng, level=0.3):
    f = np.empty((H, W, 4), F32)
    f[..., :3] = (level * rng.uniform(0.8, 1.25, (H, W, 3))).astype(F32) * F32(passes)
    f[..., 3] = rng.uniform(0, 2, (H, W)).astype(F32)
    return f


def synthetic_frames(W, H, passes):
    """name -> (H, W, 4) float32 sums over `passes`; every feature is placed modulo the frame, so the small shapes hold them crowded."""
    rng = np.random.default_rng(W * 1000 + H)
    P = F32(passes)
    at = lambda x, y: (y % H, x % W)
    frames = {}
    f = np.empty((H, W, 4), F32)
    f[..., :3] = F32([0.7, 0.25, 1.3]) * P
    f[..., 3] = 1.0
    frames["constant"] = f
    f = _background(W, H, passes, rng)  # a spike in the interior, on an edge and in a corner
    for x, y in ((W // 2, H // 2), (0, H // 2), (W - 1, 0)):
        f[at(x, y)][:3] = SPIKE * P
    frames["spikes"] = f
    f = _background(W, H, passes, rng)  # two adjacent spikes
    f[at(W // 2, H // 2)][:3] = SPIKE * P
    f[at(W // 2 + 1, H // 2)][:3] = SPIKE * P * F32(0.5)
    frames["pair"] = f
    f = _background(W, H, passes, rng)  # a 2x2 and a 3x3 bright block
    for x0, y0, k in ((3, 3, 2), (10, 8, 3)):
        for j in range(k):
            for i in range(k):
                f[at(x0 + i, y0 + j)][:3] = F32(50.0) * P
    frames["blocks"] = f
    f = _background(W, H, passes, rng)  # isolated NaN, +Inf, -Inf; a 3x3 and a 5x5 NaN block; a NaN beside a spike
    f[at(2, 2)][0] = np.nan
    f[at(W - 1, H - 1)][1] = np.inf
    f[at(0, H - 1)][2] = -np.inf
    for x0, y0, k in ((6, 1, 3), (12, 10, 5)):
        for j in range(k):
            for i in range(k):
                f[at(x0 + i, y0 + j)][:3] = np.nan
    f[at(25, 5)][:3] = np.nan
    f[at(26, 5)][:3] = SPIKE * P
    frames["nonfinite"] = f
    frames["all_nan"] = np.full((H, W, 4), np.nan, F32)
    f = _background(W, H, passes, rng)  # negative channels: a bright pixel with one, a pixel negative throughout, a dim one
    f[at(W // 2, H // 2)][:3] = F32([500.0, -3.0, 20.0]) * P
    f[at(W // 3, H // 3)][:3] = F32([-5.0, -1.0, -0.5]) * P
    f[at(2, H - 2)][:3] = F32([0.3, -0.2, 0.3]) * P
    frames["negative"] = f
    f = np.zeros((H, W, 4), F32)  # a dim pixel on black: below factor * floor = 0.2 it stays, above it is bounded to 0.2
    f[at(W // 3, H // 2)][:3] = F32(0.1) * P
    f[at(2 * W // 3, H // 2)][:3] = F32(0.5) * P
    frames["dim_on_black"] = f
    ys, xs = np.mgrid[0:H, 0:W]
    f = (10.0 ** rng.uniform(-3, 0, (H, W, 4))).astype(F32)
    odd = (xs + ys) % 3 == 1
    f[odd] = (10.0 ** rng.uniform(0, 3, (H, W, 4))).astype(F32)[odd]
    flat = f.reshape(-1, 4)
    for pos, ch, v in ((0, 0, np.nan), (W * H // 2, 1, np.inf), (W * H - 1, 2, -np.inf), (W * H // 3, 0, -5.0), (W * H // 3 + 1, 1, np.nan)):
        flat[pos % (W * H), ch] = v
    frames["mixed"] = f * P
    return frames


SHAPES = [(1, 1), (2, 1), (7, 5), (41, 23), (65, 9), (130, 70)]
PARAMS = [dict(), CLASSIC, dict(factor=4.0, rank=1, floor=0.05), dict(factor=8.0, rank=4, floor=0.0), dict(factor=1.0, rank=3, floor=0.2), dict(factor=0.0)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_synthetic_frames_match_the_restatement(scenes, shape):
    """Every synthetic frame x five parameter sets at each shape: partial workgroups, one row, frames smaller than the 5x5 window."""
    W, H = shape
    passes = 3
    worst, differ = 0.0, 0
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        for name, frame in synthetic_frames(W, H, passes).items():
            _upload(r, frame, passes)
            print(name)
            for params in PARAMS:
                ratio, d = check_against(r.despeckle(**params), frame, passes, **params)
                worst, differ = max(worst, ratio), differ + d
    print("%dx%d: largest |out - ref| / P over its allowance %.4f; %d changed words differ from the restatement's bits" % (W, H, worst, differ))


def test_properties_of_the_definition(scenes):
    """At 41x23, with factor 4, rank 2, floor 0.05 (CLASSIC) unless said: a constant frame, the 2x2 and 3x3 blocks and a finite frame at factor 0 come
    out with their input bits; spikes are bounded wherever they sit; of two adjacent spikes, one half as bright as the other, both are clamped at rank 2 and neither
    at rank 1 (each one's brightest neighbour is the other, and factor 4 times half the brighter is above it);
    NaN / Inf pixels come out finite except the centre of the 5x5 block and the all-NaN frame; the mean beside a spike uses the CLAMPED
    spike; negative channels are scaled with the rest; the dim pixel below the floor's bound stays and the one above it is bounded."""
    W, H, passes = 41, 23, 3
    frames = synthetic_frames(W, H, passes)
    lum = lambda px: _mean_and_luminance(px[None, None, :], passes)[2][0, 0]
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        def run(name, **params):
            _upload(r, frames[name], passes)
            return r.despeckle(**dict(CLASSIC, **params))
        for name in ("constant", "blocks"):
            for rank in (1, 2, 3):
                got = run(name, rank=rank)
                assert np.array_equal(bits(got["radiance"]), bits(frames[name])) and (got["clamped"], got["repaired"]) == (0, 0), (name, rank)
        for name in ("spikes", "pair", "blocks", "negative", "dim_on_black", "constant"):
            got = run(name, factor=0.0)
            assert np.array_equal(bits(got["radiance"]), bits(frames[name])) and (got["clamped"], got["repaired"]) == (0, 0), name
        got = run("spikes")
        assert got["clamped"] == 3
        for x, y in ((W // 2, H // 2), (0, H // 2), (W - 1, 0)):
            assert lum(got["radiance"][y, x]) <= 4.0 * 0.3 * 1.25 * 1.001 and lum(got["radiance"][y, x]) >= 4.0 * 0.3 * 0.8 * 0.999, (x, y)
            a, b = got["radiance"][y, x, :3].astype(np.float64), frames["spikes"][y, x, :3].astype(np.float64)
            assert np.allclose(a / a[1], b / b[1], rtol=1e-5)  # the hue is kept
        x, y = W // 2, H // 2
        both, one = run("pair"), run("pair", rank=1)
        assert both["clamped"] == 2 and one["clamped"] == 0
        assert np.array_equal(bits(one["radiance"]), bits(frames["pair"]))
        for px in (both["radiance"][y, x], both["radiance"][y, x + 1]):
            assert lum(px) <= 4.0 * 0.3 * 1.25 * 1.001
        got = run("nonfinite")
        fin = np.isfinite(got["radiance"][..., :3]).all(-1)
        assert (~fin).sum() == 1 and not fin[12, 14]  # the centre of the 5x5 block, with its input bits
        assert np.array_equal(bits(got["radiance"][12, 14]), bits(frames["nonfinite"][12, 14]))
        assert got["repaired"] == 3 + 9 + 24 + 1 and got["clamped"] == 1
        # the NaN beside the spike: the mean of its 8 neighbours with the spike at its clamped height, far below a mean with the spike in
        assert lum(got["radiance"][5, 25]) < 1.0 and lum(got["radiance"][5, 26]) < 4.0 * 0.3 * 1.25 * 1.001
        plain = run("nonfinite", factor=0.0)
        assert lum(plain["radiance"][5, 25]) > 50.0 and plain["clamped"] == 0 and plain["repaired"] == got["repaired"]
        got = run("all_nan")
        assert np.array_equal(bits(got["radiance"]), bits(frames["all_nan"])) and (got["clamped"], got["repaired"]) == (0, 0)
        got = run("negative")
        px, was = got["radiance"][H // 2, W // 2, :3], frames["negative"][H // 2, W // 2, :3]
        assert px[1] < 0 and px[1] / px[0] == pytest.approx(was[1] / was[0], rel=1e-5) and px[0] < was[0] / 50
        assert np.array_equal(bits(got["radiance"][H // 3, W // 3]), bits(frames["negative"][H // 3, W // 3]))  # l = 0: never above a bound
        got = run("dim_on_black")
        assert got["clamped"] == 1
        assert np.array_equal(bits(got["radiance"][H // 2, W // 3]), bits(frames["dim_on_black"][H // 2, W // 3]))
        assert lum(got["radiance"][H // 2, 2 * W // 3]) == pytest.approx(4.0 * 0.05, rel=1e-5)
        assert run("dim_on_black", floor=0.0)["clamped"] == 2  # (what the floor is for)


TONES = [dict(), dict(curve="reinhard", exposure=1.0, white=2.0), dict(curve="aces", auto_exposure=True)]


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_without_despeckle_parameters_present_is_display_bit_for_bit(scenes, build):
    """present(despeckle=None) = display(), image and scale, in every numerics build; with the default tone, no glare and no denoiser
    the plain resolve; and factor 0 on a finite frame gives the accumulation's bits and, presented, the plain images."""
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(3)
        for tone in TONES:
            for dn in (None, dict(iterations=2)):
                for gl in (None, dict(levels=4, strength=0.3)):
                    img, s = r.present(despeckle=None, denoise=dn, glare=gl, **tone)
                    want, s_want = r.display(denoise=dn, glare=gl, **tone)
                    assert np.array_equal(img, want) and bits(F32(s)) == bits(F32(s_want)), (tone, dn, gl)
        assert np.array_equal(r.present()[0], r.argb8())
        acc = r.radiance().copy()
        acc[~np.isfinite(acc)] = 0.5  # (a finite frame, whatever the render left)
        _upload(r, acc, 3)
        off = r.despeckle(factor=0.0)
        assert np.array_equal(bits(off["radiance"]), bits(acc)) and (off["clamped"], off["repaired"]) == (0, 0)
        for tone in TONES:
            for dn in (None, dict(iterations=2)):
                img, s = r.present(despeckle=dict(factor=0.0), denoise=dn, glare=dict(levels=4, strength=0.3), **tone)
                want, s_want = r.display(denoise=dn, glare=dict(levels=4, strength=0.3), **tone)
                assert np.array_equal(img, want) and bits(F32(s)) == bits(F32(s_want)), (tone, dn)


def test_present_is_the_existing_chain_over_the_despeckled_frame(scenes):
    """kajo_hip_present_argb8 = the existing denoise, glare and tone kernels over kajo_hip_despeckle's frame: written back into a twin's
    accumulation, the despeckled frame displays to the same image and the same automatic scale, with and without the denoiser (which
    takes the frame in the handle's tile layout)."""
    sc = scenes["spheres_a169"]
    gl = dict(levels=5, strength=0.4, threshold=0.5)
    with HipRenderer(sc, 130, 70, spp=4, exact=True, aov=True) as r, HipRenderer(sc, 130, 70, spp=4, exact=True, aov=True) as twin:
        r.render(1)
        twin.render(1)
        ds = r.despeckle(**CLASSIC)
        assert ds["clamped"] > 0
        _upload(twin, ds["radiance"], 1)
        for tone in TONES:
            for dn in (None, dict(iterations=3), dict(iterations=0)):
                for g in (None, gl):
                    img, s = r.present(despeckle=CLASSIC, denoise=dn, glare=g, **tone)
                    want, s_want = twin.display(denoise=dn, glare=g, **tone)
                    assert np.array_equal(img, want) and bits(F32(s)) == bits(F32(s_want)), (tone, dn, g)
        assert r.despeckle_counts() == (ds["clamped"], ds["repaired"])
        assert not np.array_equal(r.present(despeckle=CLASSIC, denoise=dict(iterations=3))[0], r.display(denoise=dict(iterations=3))[0])


def _despeckle_params(**kw):
    p = capi.KajoDespeckleParams()
    capi.lib().kajo_hip_default_despeckle_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _present_gathered(root, gathered, W, H, d, g, tone):
    """kajo_hip_present_gathered_argb8_device on `root` -> (argb8, scale, counts)."""
    import torch
    L = capi.lib()
    out = torch.empty(W * H, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    ref = lambda p: None if p is None else C.byref(p)
    capi.check(L.kajo_hip_present_gathered_argb8_device(root._h, src, ref(d), ref(g), C.byref(tone), C.c_void_p(out.data_ptr())))
    scale = root.tone_scale()
    counts = root.despeckle_counts() if d is not None else None
    root.wait()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(H, W), scale, counts


def test_frame_image_and_counts_do_not_depend_on_the_owners(scenes):
    """1, 2, 3 and 8 owners gathered on one GPU through the gathered twin, and the whole-frame handle (its tiles, its composed frame):
    the same image bits, scale bits and counts; also on a second call and on a twin handle. The FLOAT frame is compared, with the
    restatement and bit for bit, for the whole-frame handle, its second call and its twin only: the gathered twin has no float
    read-back, so for 2, 3 and 8 owners what is asserted is the 8-bit image after glare and an automatic exposure (whose scale, a
    log-average over every pixel of the despeckled frame, is compared in bits) and the two counts. A ragged frame with a NaN pixel
    written in, so that both kernels have work in tiles cut by the edges."""
    from test_hip_glare import _glare_params
    from test_hip_tonemap import _gathered, _tone_params
    import torch
    sc = scenes["spheres_a169"]
    W, H = 200, 77
    ds = dict(factor=2.0, rank=2, floor=0.01)
    gl = dict(levels=4, strength=0.25)
    case = dict(curve="reinhard", auto_exposure=True)
    d, g, t = _despeckle_params(**ds), _glare_params(**gl), _tone_params(**case)
    holes = [(0, 0), (W - 1, H - 1), (65, 17), (66, 17), (130, 40)]

    def poison(owners):
        # NaN into the same image pixels, whoever owns them
        layout = TileLayout(W, H, len(owners))
        for o in owners:
            o.wait()
        for x, y in holes:
            owner, slot = layout.owner_and_slot(np.array([x]), np.array([y]))
            from bench import DevicePtr
            ptr, nbytes = owners[int(owner[0])].tile_buffer()
            buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
            buf[int(slot[0]), 0] = float("nan")
        torch.cuda.synchronize()

    with HipRenderer(sc, W, H, spp=4, exact=True) as r, HipRenderer(sc, W, H, spp=4, exact=True) as twin:
        for h in (r, twin):
            h.render(1)
            poison([h])
        img, s = r.present(despeckle=ds, glare=gl, **case)
        counts = r.despeckle_counts()
        assert counts[0] > 0 and counts[1] == len(holes)
        again, s2 = r.present(despeckle=ds, glare=gl, **case)
        assert np.array_equal(img, again) and bits(F32(s)) == bits(F32(s2)) and r.despeckle_counts() == counts
        t_img, t_s = twin.present(despeckle=ds, glare=gl, **case)
        assert np.array_equal(img, t_img) and bits(F32(s)) == bits(F32(t_s)) and twin.despeckle_counts() == counts
        own, s3, c3 = _present_gathered(r, None, W, H, d, g, t)
        assert np.array_equal(own, img) and bits(F32(s3)) == bits(F32(s)) and c3 == counts
        first = r.despeckle(**ds)  # composes the float frame: the calls now read it
        assert (first["clamped"], first["repaired"]) == counts
        check_against(first, r.radiance(), 1, **ds)
        assert np.array_equal(bits(first["radiance"]), bits(twin.despeckle(**ds)["radiance"]))
        assert np.array_equal(bits(first["radiance"]), bits(r.despeckle(**ds)["radiance"]))
        f_img, f_s = r.present(despeckle=ds, glare=gl, **case)
        assert np.array_equal(f_img, img) and bits(F32(f_s)) == bits(F32(s))
        assert not np.array_equal(img, r.display(glare=gl, **case)[0])
        # without despeckle parameters the gathered twin is kajo_hip_display_gathered_argb8_device
        assert np.array_equal(_present_gathered(r, None, W, H, None, g, t)[0], r.display(glare=gl, **case)[0])
    for count in (1, 2, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile_index=k, tile_count=count) for k in range(count)]
        try:
            for o in owners:
                o.render(1)
            poison(owners)
            gathered = _gathered(owners)
            got, gs, gc = _present_gathered(owners[0], gathered, W, H, d, g, t)
            assert np.array_equal(got, img), count
            assert bits(F32(gs)) == bits(F32(s)) and gc == counts, (count, gs, s, gc, counts)
        finally:
            for o in owners:
                o.close()


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_despeckle_leaves_the_handle_as_it_was(scenes, build):
    """radiance(), aov() and counters() (kernelMs included) of a handle that despeckled and presented are those of a twin that never
    did; so are the passes rendered afterwards."""
    from test_hip_glare import _glare_params
    from test_hip_tonemap import _tone_params
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as a, \
            HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        a.despeckle()
        a.despeckle(factor=0.0)
        a.present(despeckle=dict(), glare=dict(), curve="aces", auto_exposure=True)
        a.present(despeckle=dict(factor=2.0, rank=1), denoise=dict(iterations=3), glare=dict(levels=3), curve="reinhard", exposure=1.0)
        _present_gathered(a, None, 100, 75, _despeckle_params(), _glare_params(), _tone_params("reinhard", auto_exposure=True))
        assert a.counters()["kernelMs"] == ms
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert np.array_equal(a.argb8(), b.argb8())
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        ca, cb = a.counters(), b.counters()
        for key in ("passes", "launches", "paths", "traversals", "vertices"):
            assert ca[key] == cb[key], key
        assert ca["passes"] == 3
        assert np.array_equal(a.denoise()["argb8"], b.denoise()["argb8"])
        a.render(2)
        b.render(2)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert a.counters()["passes"] == 5
        assert np.array_equal(bits(a.despeckle()["radiance"]), bits(b.despeckle()["radiance"]))


def test_refusals_and_states_on_a_device(scenes):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 64, 48, spp=4, exact=True) as r:
        with pytest.raises(capi.KajoError) as e:
            r.despeckle_counts()
        assert e.value.code == capi.KAJO_E_STATE
        for call in (r.despeckle, lambda: r.present(despeckle=dict())):
            with pytest.raises(capi.KajoError) as e:
                call()
            assert e.value.code == capi.KAJO_E_STATE  # nothing rendered yet
        r.render(1)
        with pytest.raises(capi.KajoError) as e:
            r.present(despeckle=dict(), denoise={})  # (no AOVs: what kajo_hip_denoise says)
        assert e.value.code == capi.KAJO_E_STATE
        for bad in (dict(factor=0.5), dict(rank=0), dict(rank=5), dict(floor=-1.0)):
            with pytest.raises(capi.KajoError) as e:
                r.despeckle(**bad)
            assert e.value.code == capi.KAJO_E_INVALID
            with pytest.raises(capi.KajoError) as e:
                r.present(despeckle=bad)
            assert e.value.code == capi.KAJO_E_INVALID
        L = capi.lib()  # either output pointer may be NULL
        p = _despeckle_params()
        capi.check(L.kajo_hip_despeckle(r._h, C.byref(p), None, None))
        assert r.despeckle_counts() == (lambda d: (d["clamped"], d["repaired"]))(r.despeckle())
    with HipRenderer(sc, 64, 48, spp=4, exact=True, tile_index=1, tile_count=2) as part:
        part.render(1)
        for call in (part.despeckle, lambda: part.present(despeckle=dict())):
            with pytest.raises(capi.KajoError) as e:
                call()
            assert e.value.code == capi.KAJO_E_STATE


RENDERED_PARAMS = dict(default=dict(), classic=CLASSIC, rank1=dict(factor=4.0, rank=1, floor=0.05), wide=dict(factor=8.0, rank=3, floor=0.2))


@pytest.fixture(scope="module")
def rendered(scenes):
    """spheres.json 16:9 at 160x90, EXACT, 4 spp x 1 pass with the AOVs; computed once."""
    with HipRenderer(scenes["spheres_a169"], 160, 90, spp=4, exact=True, aov=True) as r:
        r.render(1)
        acc = r.radiance()
        aov = r.aov()
        out = {name: r.despeckle(**p) for name, p in RENDERED_PARAMS.items()}
    acc.setflags(write=False)
    return dict(acc=acc, aov=aov, out=out, passes=1)


def test_rendered_frame_matches_the_restatement_and_keeps_the_lights(rendered):
    """Sets and counts equal the restatement's; the frame has fireflies to clamp; and no pixel inside a light's disc changes. The disc:
    the pixels whose every camera sample hit a surface of albedo 0 -- in spheres.json the three emissive spheres and nothing else --
    and whose luminance is at least the dimmest emission's."""
    for name, got in rendered["out"].items():
        check_against(got, rendered["acc"], rendered["passes"], **RENDERED_PARAMS[name])
    assert rendered["out"]["classic"]["clamped"] > 0
    A = rendered["aov"]["raw"][0]
    disc = (A[..., 3] == rendered["aov"]["samples"]) & (A[..., :3] == 0).all(-1)
    assert 20 <= disc.sum() <= 2000, disc.sum()
    for name in ("default", "classic"):
        got = rendered["out"][name]
        changed = (bits(got["radiance"]) != bits(rendered["acc"])).any(-1)
        print("%s: light discs %d pixels, %d of them changed; %d pixels clamped in all" % (name, disc.sum(), (changed & disc).sum(), got["clamped"]))
        assert not (changed & disc).any(), (name, np.argwhere(changed & disc)[:10])


def test_a_nan_in_the_accumulation_leaves_no_black_pixel(scenes):
    """NaN written into the accumulation at pixels whose eight neighbours are not black (a 4-spp frame has black pixels of its own):
    display() shows the (0, 0, 0) dots the clamp makes of them, present(despeckle=...) none of them, and no black pixel the frame did
    not have before."""
    W, H = 160, 90
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, exact=True) as r:
        r.render(1)
        frame = r.radiance().copy()
        before = r.display(curve="reinhard")[0] & 0xFFFFFF
        lit = np.pad(before != 0, 1, constant_values=True)
        ring = np.all([lit[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dx, dy in RING], axis=0) & (before != 0)
        ys, xs = np.nonzero(ring)
        assert len(xs) > 100
        spots = [(int(xs[i]), int(ys[i])) for i in np.linspace(0, len(xs) - 1, 7).astype(int)]
        for x, y in spots:
            frame[y, x, :3] = np.nan
        _upload(r, frame, 1)
        plain = r.display(curve="reinhard")[0] & 0xFFFFFF
        img = r.present(despeckle=dict(factor=0.0), curve="reinhard")[0] & 0xFFFFFF
        assert r.despeckle_counts() == (0, int(restate(frame, 1, factor=0.0)["repaired"].sum())) and r.despeckle_counts()[1] >= len(spots)
        for x, y in spots:
            assert plain[y, x] == 0 and img[y, x] != 0, (x, y)
        assert not ((img == 0) & (before != 0)).any()
        img = r.present(despeckle=dict(), curve="reinhard")[0] & 0xFFFFFF
        for x, y in spots:
            assert img[y, x] != 0, (x, y)


def _rmse(img, ref, mask):
    return float(np.sqrt(np.mean((np.clip(img, 0, 1) - np.clip(ref, 0, 1))[mask] ** 2)))


def test_quality_against_a_converged_frame(scenes):
    """tests/test_hip_denoise.py's quality setup -- EXACT, spheres.json 16:9 at 320x180, truth 64 spp x 40 passes, noisy frame 4 spp x 1
    pass -- RMSE in clamped display range over the pixels finite in the truth and the raw frame. Directions only, which need no number:
    despeckling does not raise the error of the raw frame (b <= a) nor of the denoised one (d <= c), and it moves the truth by less
    than it moves the raw frame. Asserted at the library's defaults (factor 16, rank 1, floor 0.2). tools/despeckle_sweep.py: the
    sweep; DESIGN.md section 6f: the figures. A setting of factor 4, rank 2, floor 0.05 does NOT keep d <= c (measured on one MI355X:
    (a) 0.2727, (b) 0.2522, (c) 0.0880, (d) 0.1201): at 4 spp most pixels several times their neighbours are signal, and the clamp
    removes energy the denoiser would have spread."""
    sc = scenes["spheres_a169"]
    W, H = 320, 180
    with HipRenderer(sc, W, H, spp=64, exact=True, aov=True, seed=12345) as ref:
        ref.render(40)
        truth = ref.radiance()[..., :3] / ref.passes
        truth_ds = ref.despeckle()["radiance"][..., :3] / ref.passes
    with HipRenderer(sc, W, H, spp=4, exact=True, aov=True) as r:
        r.render(1)
        raw = r.radiance()[..., :3] / r.passes
        ds = r.despeckle()["radiance"][..., :3] / r.passes
        dn = r.denoise()["radiance"][..., :3] / r.passes
        # (d): the denoiser over the despeckled frame, as present() runs it -- here through a twin accumulation, to read the float frame
        _upload(r, r.despeckle()["radiance"], 1)
        ds_dn = r.denoise()["radiance"][..., :3] / r.passes
    mask = np.isfinite(truth).all(-1) & np.isfinite(raw).all(-1)
    a, b, c, d = (_rmse(x, truth, mask) for x in (raw, ds, dn, ds_dn))
    move_truth, move_raw = _rmse(truth_ds, truth, mask), _rmse(ds, raw, mask)
    print("RMSE raw %.4f, despeckled %.4f, denoised %.4f, despeckled + denoised %.4f; despeckle moves the truth by %.4f, the raw frame by %.4f"
          % (a, b, c, d, move_truth, move_raw))
    assert b <= a and d <= c, (a, b, c, d)
    assert move_truth < move_raw, (move_truth, move_raw)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("gpus", [["--gpus", "1"], ["--gpus", "3", "--same-device"]])
def test_driver_despeckles_as_the_c_abi(tmp_path, gpus):
    """kajo_render --despeckle --despeckle-factor 2 --glare 0.2 --tonemap reinhard: the pixels of HipRenderer.present on the same frame,
    one owner and three gathered on one device; --hdr stays the accumulation / P; without the option, the image written today."""
    scene = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
    out, raw, hdr = str(tmp_path / "o.png"), str(tmp_path / "o.raw"), str(tmp_path / "o.pfm")
    base = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "--json", *gpus]
    p = subprocess.run(base + ["-o", out, "--raw", raw, "--hdr", hdr, "--despeckle", "--despeckle-factor", "2", "--despeckle-floor", "0.01", "--glare", "0.2",
                               "--glare-levels", "4", "--tonemap", "reinhard", scene], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    acc = np.fromfile(raw, np.float32).reshape(54, 96, 4)
    png = read_png(out)
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    with HipRenderer(sc, 96, 54, exact=True) as r:
        r.render(2)
        assert np.array_equal(bits(r.radiance()), bits(acc))
        px, _ = r.present(despeckle=dict(factor=2.0, floor=0.01), glare=dict(strength=0.2, levels=4), curve="reinhard")
        counts = r.despeckle_counts()
        plain, _ = r.display(glare=dict(strength=0.2, levels=4), curve="reinhard")
    assert counts[0] > 0 and not np.array_equal(px, plain)
    assert (stats["despeckle_clamped"], stats["despeckle_repaired"]) == counts
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (px >> shift) & 255), k
    assert np.array_equal(bits(read_pfm(hdr)), bits(acc[..., :3] / F32(2)))
    none = str(tmp_path / "n.png")
    p = subprocess.run(base + ["-o", none, "--glare", "0.2", "--glare-levels", "4", "--tonemap", "reinhard", scene], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    png = read_png(none)
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (plain >> shift) & 255), k


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_despeckles_in_front_of_the_denoiser(tmp_path):
    """--denoise FILE with --despeckle, --glare and a tone option writes HipRenderer.present(despeckle=..., denoise=..., glare=..., tone)."""
    scene = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
    dn = str(tmp_path / "d.png")
    p = subprocess.run([BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "-o", "", "--denoise", dn, "--despeckle", "--despeckle-factor", "2", "--despeckle-rank", "2", "--despeckle-floor", "0.01",
                        "--glare", "0.2",
                        "--glare-levels", "4", "--tonemap", "aces", scene], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")
    with HipRenderer(sc, 96, 54, exact=True, aov=True) as r:
        r.render(2)
        px, _ = r.present(despeckle=dict(factor=2.0, rank=2, floor=0.01), denoise=dict(iterations=5), glare=dict(strength=0.2, levels=4), curve="aces")
        assert r.despeckle_counts()[0] > 0
    png = read_png(dn)
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (px >> shift) & 255), k
