"""Local tone mapping (include/kajo_hip.h kajo_hip_local, kajo_hip_present_local_*; kajo_amd/csrc/local.hip) on the GPU.

The kernels are held to tests/local_replay.py, a float64 numpy restatement of the header's definition, over synthetic frames written
into the accumulation through the tile buffer and over rendered frames: the counting masks must agree exactly, the pixels that do not
count and the .w channel keep their bits, and the counting pixels are compared as test_hip_denoise.compare does. Where the definition
makes the output a copy (compression 1 and detail 1, no parameters) the images are those of the existing calls bit for bit. Image and
pivot must not depend on how many owners the frame was dealt to, and the calls must leave the handle as a twin that never ran them."""
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
from kajo_amd.scene import Scene, stress_scene
from local_replay import DEFAULTS, base_layer, compare, mean_and_mask, restate, synthetic_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
F32, F64 = np.float32, np.float64

# Relative difference to the float64 restatement over the counting pixels, floored at a mean radiance of 1e-2 (local_replay.compare).
# The device's log2f / exp2f differ from numpy's in the last places and g = exp2(L' - L) carries that over tens of stops. Measured on
# the MI355X over every case of this file (synthetic frames, every shape and the whole parameter grid; the rendered frames in the
# three numerics builds; the 1000-sphere scene; the frames behind the denoiser and with a metered pivot):
#   largest mean        1.64e-6  (130x70 synthetic frames)
#   largest single      1.20e-5  (likewise; the rendered frames stay under 3.4e-7 and 1.1e-5)
# The bounds are about ten times those: the mean is the sensitive check, the margin covers other frames and the FAST build's inputs.
MEAN_BOUND = 1.6e-5
MAX_BOUND = 1.2e-4

SHAPES = [(1, 1), (2, 1), (7, 5), (41, 23), (65, 9), (130, 70)]
ITERATIONS = (0, 1, 3, 5, 8)
COMPRESSIONS = (0.4, 1.0)
DETAILS = (0.0, 1.0, 2.0)
SIGMAS = (0.5, 2.0)
SEEN = dict(mean=0.0, max=0.0)  # the largest figures of the session, printed by every test that compares


def check_against(got, F, passes, what="", want=None, **params):
    """The conditions of the module docstring against the restatement of F; -> (mean, max) over the counting pixels."""
    want = want if want is not None else restate(F, passes, **params)
    F = np.asarray(F, F32)
    c = want["counts"]
    assert np.array_equal(mean_and_mask(got, passes)[1], c), (what, params)           # the same pixels count: a condition, no tolerance
    assert np.array_equal(bits(got[~c]), bits(F[~c])), (what, params)                   # the others: as they went in
    assert np.array_equal(bits(got[..., 3]), bits(F[..., 3])), (what, params)
    mean, worst = compare(got, want["out"], passes, c)
    print("%s %s: mean %.3e max %.3e" % (what, sorted(params.items()), mean, worst))
    SEEN["mean"], SEEN["max"] = max(SEEN["mean"], mean), max(SEEN["max"], worst)
    assert mean <= MEAN_BOUND and worst <= MAX_BOUND, (what, params, mean, worst)
    return mean, worst


def _report(what):
    print("%s: largest mean so far %.3e, largest single %.3e" % (what, SEEN["mean"], SEEN["max"]))


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_synthetic_frames_match_the_restatement(scenes, shape):
    """Every synthetic frame x K 0, 1, 3, 5, 8 x compression 0.4, 1 x detail 0, 1, 2 x sigmaRange 0.5, 2 at each shape: frames smaller
    than a tap's reach (only the centre tap remains), odd sizes, frames smaller than a workgroup and ones of several, and K = 8, whose
    step of 128 is wider than every frame here. NaN / Inf pixels come out with their bits and make no neighbour non-finite."""
    W, H = shape
    passes = 3
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        for name, frame in synthetic_frames(W, H, passes).items():
            _upload(r, frame, passes)
            copy = restate(frame, passes, compression=1.0, detail=1.0)
            for K in ITERATIONS:
                for sigma in SIGMAS:
                    B = base_layer(copy["L"], K, sigma)  # (the base layer does not depend on the other two parameters)
                    for comp in COMPRESSIONS:
                        for detail in DETAILS:
                            params = dict(iterations=K, compression=comp, detail=detail, sigma_range=sigma)
                            got = r.local(**params)
                            if comp == 1.0 and detail == 1.0:
                                assert np.array_equal(bits(got), bits(frame)), (name, params)  # the copy case
                                continue
                            p = F64(F32(DEFAULTS["pivot"]))
                            with np.errstate(invalid="ignore"):
                                g = np.exp2((p + F64(F32(comp)) * (B - p)) + F64(F32(detail)) * (copy["L"] - B) - copy["L"])
                            out = frame.astype(F64)
                            out[..., :3] = np.where(copy["counts"][..., None], copy["m"].astype(F64) * g[..., None] * passes, out[..., :3])
                            check_against(got, frame, passes, "%dx%d %s" % (W, H, name), want=dict(out=out, counts=copy["counts"]), **params)
            if name == "poisoned" and W * H >= 35:
                assert 4 <= (~copy["counts"]).sum() <= 6 and copy["counts"].any()  # (the frame does hold pixels of both kinds)
    _report("%dx%d" % (W, H))


def test_the_shared_base_layer_shortcut_is_the_restatement():
    """(no GPU work: the loop above forms `out` from a base layer shared between cases; it must be restate()'s own)"""
    frame = synthetic_frames(41, 23, 3)["poisoned"]
    r = restate(frame, 3, iterations=3, compression=0.4, detail=2.0, sigma_range=0.5)
    B = base_layer(r["L"], 3, 0.5)
    p = F64(F32(DEFAULTS["pivot"]))
    with np.errstate(invalid="ignore"):
        g = np.exp2((p + F64(F32(0.4)) * (B - p)) + 2.0 * (r["L"] - B) - r["L"])
    c = r["counts"]
    assert np.array_equal((r["m"].astype(F64) * g[..., None] * 3)[c], r["out"][..., :3][c])


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rendered_frame_matches_the_restatement(scenes, build):
    """spheres 100x75, 4 passes of S = 4, in each numerics build: the output is the restatement of the handle's own frame, and it
    differs from the input."""
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, **BUILDS[build]) as r:
        r.render(4)
        acc = r.radiance()
        for params in (dict(), dict(iterations=3, compression=0.4, detail=2.0, sigma_range=0.5), dict(iterations=8, detail=0.0)):
            got = r.local(**params)
            check_against(got, acc, 4, "spheres %s" % build, **params)
            assert not np.array_equal(bits(got[..., :3]), bits(acc[..., :3]))
    _report("spheres 100x75 %s" % build)


def test_rendered_large_scene_matches_the_restatement(scenes):
    with HipRenderer(stress_scene(scenes["spheres_a169"], 1000, 16), 160, 90, spp=4, exact=True) as r:
        r.render(4)
        acc = r.radiance()
        got = r.local()
        check_against(got, acc, 4, "1000 spheres")
        assert not np.array_equal(bits(got[..., :3]), bits(acc[..., :3]))
    _report("1000 spheres 160x90")


TONES = [dict(), dict(curve="reinhard", exposure=1.0, white=2.0), dict(curve="aces", auto_exposure=True)]
COPY = dict(compression=1.0, detail=1.0)


def _same_result(a, b):
    return all(bits(F32([a[k]]))[0] == bits(F32([b[k]]))[0] if isinstance(a[k], float) else a[k] == b[k] for k in a) and a.keys() == b.keys()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_copy_cases_are_the_existing_calls_bit_for_bit(scenes, build):
    """compression = detail = 1: kajo_hip_local is radiance(), present(local=copy, ...) is present(...), image and scale or result,
    with and without each other stage; present(local=None) is the metered call."""
    ds, dn, gl, mt = dict(factor=2.0, rank=2, floor=0.01), dict(iterations=2), dict(levels=4, strength=0.25), dict(percentile=0.4, auto_white=True)
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(3)
        acc = r.radiance()
        for copy in (COPY, dict(COPY, iterations=0), dict(COPY, metered=True, sigma_range=0.5, pivot=3.0)):
            assert np.array_equal(bits(r.local(**copy)), bits(acc)), copy
            assert np.array_equal(bits(r.local(glare=gl, **copy)), bits(r.glare(**gl)))
            for tone in TONES:
                for stages in (dict(), dict(despeckle=ds), dict(denoise=dn), dict(glare=gl), dict(despeckle=ds, denoise=dn, glare=gl)):
                    img, s = r.present(local=copy, **stages, **tone)
                    want, s_want = r.present(**stages, **tone)
                    assert np.array_equal(img, want) and bits(F32([s]))[0] == bits(F32([s_want]))[0], (copy, tone, stages)
                    if not tone.get("auto_exposure"):
                        img, res = r.present(local=copy, meter=mt, **stages, **tone)
                        want, res_want = r.present(meter=mt, **stages, **tone)
                        assert np.array_equal(img, want) and _same_result(res, res_want), (copy, tone, stages)
            assert np.array_equal(r.present(local=copy)[0], r.argb8())
        with pytest.raises(capi.KajoError) as e:
            r.local_pivot()  # a copy is not a run of the stage
        assert e.value.code == capi.KAJO_E_STATE
        # local == NULL: kajo_hip_present_local_argb8 is kajo_hip_present_metered_argb8
        L = capi.lib()
        t, m = r._tone_params(curve="reinhard"), r._meter_params(**mt)
        for meter in (None, m):
            a, b = np.empty((75, 100), np.uint32), np.empty((75, 100), np.uint32)
            ra, rb = capi.KajoMeterResult(), capi.KajoMeterResult()
            ref = None if meter is None else C.byref(meter)
            capi.check(L.kajo_hip_present_local_argb8(r._h, None, None, None, None, ref, C.byref(t), a.ctypes.data_as(C.c_void_p), C.byref(ra)))
            capi.check(L.kajo_hip_present_metered_argb8(r._h, None, None, None, ref, C.byref(t), b.ctypes.data_as(C.c_void_p), C.byref(rb)))
            assert np.array_equal(a, b) and _same_result(r._meter_result(ra), r._meter_result(rb))


LOCAL = dict(iterations=4, compression=0.5, detail=1.5, sigma_range=1.5, pivot=-1.0)
METERS = [dict(), dict(percentile=0.4, auto_white=True)]


def test_chain_is_the_metered_path_over_the_stage_s_own_frame(scenes):
    """present(local=L, meter=M, **tone) = the existing metered path over kajo_hip_local's frame, written into a twin's accumulation:
    the same ARGB8 and the same result, so the meter of the chain measures the frame after the stage. Without a meter: the existing
    tone mapping of that frame, image and scale (automatic exposure is measured after the stage too)."""
    sc = scenes["spheres_a169"]
    gl = dict(levels=4, strength=0.25)
    with HipRenderer(sc, 130, 70, spp=4, exact=True) as r, HipRenderer(sc, 130, 70, spp=4, exact=True) as twin:
        r.render(3)
        for stages in (dict(), dict(despeckle=dict(factor=2.0, floor=0.01), glare=gl)):
            frame = r.local(**stages, **LOCAL)
            _upload(twin, frame, 3)
            for mt in METERS:
                for tone in TONES[:2]:
                    img, res = r.present(local=LOCAL, meter=mt, **stages, **tone)
                    want, res_want = twin.present(meter=mt, **tone)
                    assert np.array_equal(img, want) and _same_result(res, res_want), (stages, mt, tone)
                    plain, res_plain = r.present(meter=mt, **stages, **tone)
                    assert not np.array_equal(img, plain)
            for tone in TONES:
                img, s = r.present(local=LOCAL, **stages, **tone)
                want, s_want = twin.tonemap(**tone)
                assert np.array_equal(img, want) and bits(F32([s]))[0] == bits(F32([s_want]))[0], (stages, tone)
        # the stage compresses the range the chain's meter reports
        _, after = r.present(local=LOCAL, meter=dict())
        _, before = r.present(meter=dict())
        assert after["maxBin"] - after["minBin"] < before["maxBin"] - before["minBin"]


def test_chain_with_the_denoiser_in_front(scenes):
    """The stage takes the denoised frame: kajo_hip_local(denoise=...) is the restatement of kajo_hip_denoise's frame, and the chain's
    image is the tone mapping of it."""
    sc = scenes["spheres_a43"]
    dn = dict(iterations=3)
    with HipRenderer(sc, 100, 75, spp=4, exact=True, aov=True) as r, HipRenderer(sc, 100, 75, spp=4, exact=True) as twin:
        r.render(3)
        denoised = r.denoise(**dn)["radiance"]
        frame = r.local(denoise=dn, **LOCAL)
        check_against(frame, denoised, 3, "after denoise", **LOCAL)
        assert not np.array_equal(bits(frame), bits(r.local(**LOCAL)))
        _upload(twin, frame, 3)
        img, res = r.present(denoise=dn, local=LOCAL, meter=METERS[1], curve="reinhard")
        want, res_want = twin.present(meter=METERS[1], curve="reinhard")
        assert np.array_equal(img, want) and _same_result(res, res_want)
    _report("after denoise")


def test_metered_pivot(scenes):
    """KAJO_LOCAL_PIVOT_METERED: the pivot used is log2(value(q)) of the meter's histogram of the stage's input frame, rounded to float,
    reported by kajo_hip_local_pivot, and the frame is the restatement's with that pivot; an all-black frame falls back to the field."""
    sc = scenes["spheres_a43"]
    gl = dict(levels=4, strength=0.25)
    with HipRenderer(sc, 100, 75, spp=4, exact=True) as r:
        r.render(3)
        acc = r.radiance()
        for q in (0.5, 0.1, 1.0):
            got = r.local(metered=True, pivot_percentile=q, pivot=5.0)
            want = F32(np.log2(F64(F32(r.meter(percentile=q)[1]["anchorL"]))))
            assert bits(F32([r.local_pivot()]))[0] == bits(F32([want]))[0], (q, r.local_pivot(), want)
            check_against(got, acc, 3, "metered pivot", pivot=float(want))
        # behind the glare the histogram is the glared frame's
        glared = r.glare(**gl)
        got = r.local(glare=gl, metered=True, pivot_percentile=0.9)
        want = F32(np.log2(F64(F32(r.meter(glare=gl, percentile=0.9)[1]["anchorL"]))))
        assert bits(F32([r.local_pivot()]))[0] == bits(F32([want]))[0]
        check_against(got, glared, 3, "metered pivot after glare", pivot=float(want))
        # a fixed pivot is reported as given
        r.local(pivot=-3.25)
        assert r.local_pivot() == -3.25
        # no metered pixel: the field
        black = np.zeros((75, 100, 4), F32)
        _upload(r, black, 3)
        got = r.local(metered=True, pivot=1.5)
        assert r.local_pivot() == 1.5
        check_against(got, black, 3, "black", pivot=1.5)
    _report("metered pivot")


def _local_params(**kw):
    p = capi.KajoLocalParams()
    capi.lib().kajo_hip_default_local_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _local_gathered(root, gathered, W, H, d, g, l, m, tone):
    """kajo_hip_present_local_gathered_argb8_device on `root` -> (argb8, result dict)."""
    import torch
    L = capi.lib()
    out = torch.empty(W * H, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    ref = lambda p: None if p is None else C.byref(p)
    result = capi.KajoMeterResult()
    capi.check(L.kajo_hip_present_local_gathered_argb8_device(root._h, src, ref(d), ref(g), ref(l), ref(m), C.byref(tone), C.c_void_p(out.data_ptr()),
                                                              C.byref(result)))
    root.wait()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(H, W), root._meter_result(result)


@pytest.mark.parametrize("tile", [(64, 16), (32, 8)], ids=["tile64x16", "tile32x8"])
def test_image_and_pivot_do_not_depend_on_the_owners(scenes, tile):
    """130x70 on one handle and on 2, 3 and 8 owners on one GPU, gathered as the existing owner tests gather: the gathered twin's ARGB8,
    its result and the pivot it reports are the whole-frame handle's bit for bit; so are a second call and a twin handle."""
    from test_hip_tonemap import _gathered
    sc = scenes["spheres_a169"]
    W, H = 130, 70
    lp = dict(iterations=5, compression=0.6, metered=True, pivot_percentile=0.5)
    gl, mt, tone = dict(levels=3, strength=0.2), dict(percentile=0.5), dict(curve="reinhard")
    with HipRenderer(sc, W, H, spp=4, exact=True, tile=tile) as r, HipRenderer(sc, W, H, spp=4, exact=True, tile=tile) as twin:
        r.render(3)
        twin.render(3)
        img, res = r.present(glare=gl, local=lp, meter=mt, **tone)
        pivot = r.local_pivot()
        again, res2 = r.present(glare=gl, local=lp, meter=mt, **tone)
        assert np.array_equal(img, again) and _same_result(res, res2) and r.local_pivot() == pivot
        t_img, t_res = twin.present(glare=gl, local=lp, meter=mt, **tone)
        assert np.array_equal(img, t_img) and _same_result(res, t_res) and twin.local_pivot() == pivot
        frame = r.local(glare=gl, **lp)  # (composes nothing: the stages read the tiles)
        assert np.array_equal(bits(frame), bits(twin.local(glare=gl, **lp)))
        l, g, m, t = r._local_params(**lp), r._glare_params(**gl), r._meter_params(**mt), r._tone_params(**tone)
        own, own_res = _local_gathered(r, None, W, H, None, g, l, m, t)
        assert np.array_equal(own, img) and _same_result(own_res, res) and r.local_pivot() == pivot
        r.radiance()  # composes the float frame: the calls now read it, row-major
        f_img, f_res = r.present(glare=gl, local=lp, meter=mt, **tone)
        assert np.array_equal(f_img, img) and _same_result(f_res, res) and r.local_pivot() == pivot
        assert not np.array_equal(img, r.present(glare=gl, meter=mt, **tone)[0])
        # without a meter the twin does not touch the result
        plain, _ = r.present(glare=gl, local=lp, **tone)
        got, untouched = _local_gathered(r, None, W, H, None, g, l, None, t)
        assert np.array_equal(got, plain) and untouched["pixels"] == 0
    for count in (2, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile=tile, tile_index=k, tile_count=count) for k in range(count)]
        try:
            for o in owners:
                o.render(3)
            gathered = _gathered(owners)
            got, got_res = _local_gathered(owners[0], gathered, W, H, None, g, l, m, t)
            assert np.array_equal(got, img), count
            assert _same_result(got_res, res), (count, got_res, res)
            assert bits(F32([owners[0].local_pivot()]))[0] == bits(F32([pivot]))[0], count
        finally:
            for o in owners:
                o.close()


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_the_stage_leaves_the_handle_as_it_was(scenes, build):
    """radiance(), argb8(), aov() and counters() (kernelMs included) of a handle that ran the stage every way are those of a twin that
    never did; so are the passes rendered afterwards."""
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as a, \
            HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        a.local()
        a.local(iterations=8, compression=0.4, detail=2.0, metered=True, denoise=dict(iterations=2), glare=dict(), despeckle=dict())
        a.present(local=dict(), curve="aces", auto_exposure=True)
        a.present(local=dict(metered=True), meter=dict(auto_white=True), denoise=dict(iterations=3), curve="reinhard")
        _local_gathered(a, None, 100, 75, None, None, a._local_params(metered=True), a._meter_params(), a._tone_params("reinhard"))
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
        assert np.array_equal(bits(a.local()), bits(b.local()))
        img, res = a.present(local=dict(), meter=dict(), curve="aces")
        t_img, t_res = b.present(local=dict(), meter=dict(), curve="aces")
        assert np.array_equal(img, t_img) and _same_result(res, t_res)


def test_refusals_and_states_on_a_device(scenes):
    import torch
    L = capi.lib()
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 64, 48, spp=4, exact=True) as r:
        out = torch.empty(64 * 48, dtype=torch.int32, device="cuda")
        l, t = _local_params(), r._tone_params()
        for call in (lambda: L.kajo_hip_local(r._h, None, None, None, C.byref(l), None),
                     lambda: L.kajo_hip_present_local_argb8(r._h, None, None, None, C.byref(l), None, C.byref(t), None, None),
                     lambda: L.kajo_hip_present_local_gathered_argb8_device(r._h, None, None, None, C.byref(l), None, C.byref(t),
                                                                            C.c_void_p(out.data_ptr()), None)):
            assert call() == capi.KAJO_E_STATE and "nothing rendered" in L.kajo_hip_last_error().decode()
        with pytest.raises(capi.KajoError) as e:
            r.local_pivot()
        assert e.value.code == capi.KAJO_E_STATE  # before the first use
        r.render(1)
        with pytest.raises(capi.KajoError) as e:
            r.local_pivot()
        assert e.value.code == capi.KAJO_E_STATE
        for call in (lambda: r.local(denoise={}), lambda: r.present(local=dict(), denoise={})):
            with pytest.raises(capi.KajoError) as e:
                call()  # (no AOVs: what kajo_hip_denoise says)
            assert e.value.code == capi.KAJO_E_STATE
        for call in (lambda: r.local(iterations=9), lambda: r.present(local=dict(compression=0.0)), lambda: r.local(sigma_range=float("nan"))):
            with pytest.raises(capi.KajoError) as e:
                call()
            assert e.value.code == capi.KAJO_E_INVALID
        with pytest.raises(capi.KajoError):
            r.local_pivot()  # (a refused call is not a use)
        assert L.kajo_hip_local(r._h, None, None, None, C.byref(l), None) == 0  # radiance may be NULL
        assert r.local_pivot() == F32(np.log2(0.18))
    with HipRenderer(sc, 64, 48, spp=4, exact=True, tile_index=1, tile_count=2) as part:
        part.render(1)
        for call in (part.local, lambda: part.present(local=dict())):
            with pytest.raises(capi.KajoError) as e:
                call()
            assert e.value.code == capi.KAJO_E_STATE  # a share of the frame, not composed


@pytest.fixture(scope="module")
def driver_reference():
    """caustics 96x54, 2 passes, through the C ABI: the accumulation, the image and the result of the chain the driver is asked for, the
    pivot it used, and the image without the stage; computed once."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    with HipRenderer(sc, 96, 54, exact=True) as r:
        r.render(2)
        acc = r.radiance()
        px, res = r.present(local=dict(compression=0.6, metered=True), meter=dict(percentile=0.5))
        pivot = r.local_pivot()
        plain, _ = r.present(meter=dict(percentile=0.5))
    assert not np.array_equal(px, plain)
    return dict(acc=acc, px=px, res=res, pivot=pivot, plain=plain)


DRIVER = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "--json"]
SCENE = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("owners", ["1", "3-on-one-device", "2"])
def test_driver_maps_as_the_c_abi(tmp_path, driver_reference, owners):
    """kajo_render --local-contrast 0.6 --local-pivot metered --meter-exposure 0.5 writes the PNG HipRenderer.present gives on the same
    frame: one owner, three gathered on one device, and two -- on two GPUs where the box shows more than one, else on one device;
    --json reports the pivot and the parameters; --hdr stays the accumulation / P."""
    import torch
    gpus = {"1": ["--gpus", "1"], "3-on-one-device": ["--gpus", "3", "--same-device"],
            "2": ["--gpus", "2"] + ([] if torch.cuda.device_count() > 1 else ["--same-device"])}[owners]
    ref = driver_reference
    out, raw, hdr = str(tmp_path / "o.png"), str(tmp_path / "o.raw"), str(tmp_path / "o.pfm")
    p = subprocess.run(DRIVER + gpus + ["-o", out, "--raw", raw, "--hdr", hdr, "--local-contrast", "0.6", "--local-pivot", "metered",
                                        "--meter-exposure", "0.5", SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    assert np.array_equal(bits(np.fromfile(raw, np.float32).reshape(54, 96, 4)), bits(ref["acc"]))
    png = read_png(out)
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (ref["px"] >> shift) & 255), k
    assert F32(stats["local_pivot"]) == F32(ref["pivot"]), (stats["local_pivot"], ref["pivot"])
    assert (F32(stats["local_compression"]), stats["local_detail"], stats["local_range"], stats["local_iterations"]) == (F32(0.6), 1.0, 2.0, 5)
    assert stats["local_pivot_metered"] is True and stats["local_pivot_percentile"] == 0.5
    assert F32(stats["meter_exposure"]) == F32(ref["res"]["exposure"]) and stats["meter_metered"] == ref["res"]["metered"]
    assert np.array_equal(bits(read_pfm(hdr)), bits(ref["acc"][..., :3] / F32(2)))


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_with_contrast_one_writes_the_plain_image(tmp_path, driver_reference):
    one, none = str(tmp_path / "1.png"), str(tmp_path / "n.png")
    for path, extra in ((one, ["--local-contrast", "1", "--local-pivot", "metered"]), (none, [])):
        p = subprocess.run(DRIVER + ["--gpus", "1", "-o", path, "--meter-exposure", "0.5", *extra, SCENE], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        stats = json.loads(p.stdout.strip().splitlines()[-1])
        assert ("local_pivot" in stats) == bool(extra) and stats.get("local_pivot") is None
    assert np.array_equal(read_png(one), read_png(none))
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(read_png(none)[..., k], (driver_reference["plain"] >> shift) & 255), k
