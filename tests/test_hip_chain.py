"""The identities include/kajo_hip.h promises of the display chain (despeckle -> denoise -> grade -> lens -> glare -> local -> meter ->
tone -> view), on the GPU: every chain entry point gives the words and the KajoMeterResult of the whole-chain call with the remaining
stages NULL -- kajo_hip_present_grade_argb8 for the handle's own frame, kajo_hip_present_grade_gathered_argb8_device for tiles --, the
radiance entries repeat themselves, kajo_hip_meter measures what kajo_hip_present_metered_argb8 maps, and the refusals that need a
handle's state keep their code and text. One 70 x 37 frame (ragged against the 64 x 16 tile on both axes) of two passes with the AOV and
matte flags, FAST and STRICT; every stage set so that it changes the frame."""
import ctypes as C

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu

W, H, OUT_W, OUT_H = 70, 37, 35, 18
STAGES = ("despeckle", "denoise", "grade", "lens", "glare", "local", "meter", "tone", "view")
STRUCTS = {"despeckle": capi.KajoDespeckleParams, "denoise": capi.KajoDenoiseParams, "grade": capi.KajoGradeParams, "lens": capi.KajoLensParams,
           "glare": capi.KajoGlareParams, "local": capi.KajoLocalParams, "meter": capi.KajoMeterParams, "tone": capi.KajoToneParams,
           "view": capi.KajoViewParams}
# the stages of every entry point's signature, in the header's order of arguments
HOST = {
    "kajo_hip_tonemap_argb8": ("tone", "denoise"),
    "kajo_hip_display_argb8": ("denoise", "glare", "tone"),
    "kajo_hip_present_argb8": ("despeckle", "denoise", "glare", "tone"),
    "kajo_hip_present_metered_argb8": ("despeckle", "denoise", "glare", "meter", "tone"),
    "kajo_hip_present_local_argb8": ("despeckle", "denoise", "glare", "local", "meter", "tone"),
    "kajo_hip_present_lens_argb8": ("despeckle", "denoise", "lens", "glare", "local", "meter", "tone"),
    "kajo_hip_present_view_argb8": ("despeckle", "denoise", "lens", "glare", "local", "meter", "tone", "view"),
    "kajo_hip_present_grade_argb8": ("despeckle", "denoise", "grade", "lens", "glare", "local", "meter", "tone", "view"),
}
GATHERED = {
    "kajo_hip_tonemap_gathered_argb8_device": ("tone",),
    "kajo_hip_display_gathered_argb8_device": ("glare", "tone"),
    "kajo_hip_present_gathered_argb8_device": ("despeckle", "glare", "tone"),
    "kajo_hip_present_metered_gathered_argb8_device": ("despeckle", "glare", "meter", "tone"),
    "kajo_hip_present_local_gathered_argb8_device": ("despeckle", "glare", "local", "meter", "tone"),
    "kajo_hip_present_view_gathered_argb8_device": ("despeckle", "glare", "local", "meter", "tone", "view"),
    "kajo_hip_present_grade_gathered_argb8_device": ("despeckle", "grade", "glare", "local", "meter", "tone", "view"),
}
RADIANCE = {
    "kajo_hip_glare": ("glare", "denoise"),
    "kajo_hip_local": ("despeckle", "denoise", "glare", "local"),
    "kajo_hip_lens": ("despeckle", "denoise", "lens"),
    "kajo_hip_grade": ("despeckle", "denoise", "grade"),
}
METER = ("despeckle", "denoise", "glare", "meter")
STATE = -4  # KAJO_E_STATE
INVALID = -1


def stage_params():
    """every stage's parameters, none of them the identity"""
    L = capi.lib()
    p = {}
    for s in STAGES:
        p[s] = STRUCTS[s]()
        getattr(L, "kajo_hip_default_%s_params" % s)(C.byref(p[s]))
    p["glare"].strength = 0.25
    p["local"].compression = 0.5
    p["lens"].aperture = 0.05
    p["grade"].global_.slope[0], p["grade"].global_.slope[2] = 1.25, 0.75
    p["view"].outW, p["view"].outH = OUT_W, OUT_H  # the whole frame at half the size
    p["tone"].curve = capi.KAJO_TONE_REINHARD
    p["tone"].exposure = 0.5
    return p


def ref(p, stages, s):
    return C.byref(p[s]) if s in stages else None


def words_of(stages):
    return OUT_W * OUT_H if "view" in stages else W * H


def call_host(h, name, stages, p):
    """(rc, ARGB8 words, the meter result's bytes) of a host entry point with the stages of its signature, or of the whole-chain call"""
    out = np.zeros(words_of(stages), np.uint32)
    res = capi.KajoMeterResult()
    args = [h] + [ref(p, stages, s) for s in HOST[name]] + [out.ctypes.data_as(C.c_void_p)]
    args.append(None if name in ("kajo_hip_tonemap_argb8", "kajo_hip_display_argb8", "kajo_hip_present_argb8") else C.byref(res))
    rc = getattr(capi.lib(), name)(*args)
    return rc, out, bytes(res)


def call_gathered(h, name, stages, p):
    import torch
    out = torch.zeros(words_of(stages), dtype=torch.int32, device="cuda")
    res = capi.KajoMeterResult()
    args = [h, None] + [ref(p, stages, s) for s in GATHERED[name]] + [C.c_void_p(out.data_ptr())]
    if "meter" in GATHERED[name]:
        args.append(C.byref(res))
    rc = getattr(capi.lib(), name)(*args)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().view(np.uint32), bytes(res)


def call_radiance(h, name, p, stages=None):
    out = np.zeros(W * H * 4, np.float32)
    stages = RADIANCE[name] if stages is None else stages
    rc = getattr(capi.lib(), name)(h, *[ref(p, stages, s) for s in RADIANCE[name]], out.ctypes.data_as(C.c_void_p))
    return rc, out.view(np.uint32)


def call_meter(h, p):
    hist = np.zeros(capi.KAJO_METER_BINS, np.uint32)
    res = capi.KajoMeterResult()
    rc = capi.lib().kajo_hip_meter(h, *[C.byref(p[s]) for s in METER], hist.ctypes.data_as(C.c_void_p), C.byref(res))
    return rc, hist, res


def error():
    return (capi.lib().kajo_hip_last_error() or b"").decode()


def collect(scene, strict):
    """Every output the tests compare, by name: run once per numerics build (and by the job that compares two builds of the library)"""
    got = {}
    p = stage_params()
    with HipRenderer(scene, W, H, strict=strict, aov=True, matte=True) as r:
        h = r._h
        for name, stages in HOST.items():
            got["unrendered/" + name] = (call_host(h, name, stages, p)[0], error())
        for name, stages in GATHERED.items():
            got["unrendered/" + name] = (call_gathered(h, name, stages, p)[0], error())
        for name in RADIANCE:
            got["unrendered/" + name] = (call_radiance(h, name, p)[0], error())
        got["unrendered/kajo_hip_meter"] = (call_meter(h, p)[0], error())
        r.render(2)
        for name, stages in HOST.items():
            got["host/" + name] = call_host(h, name, stages, p)
            got["host-whole/" + name] = call_host(h, "kajo_hip_present_grade_argb8", stages, p)
        for name, stages in GATHERED.items():
            got["gathered/" + name] = call_gathered(h, name, stages, p)
            got["gathered-whole/" + name] = call_gathered(h, "kajo_hip_present_grade_gathered_argb8_device", stages, p)
        counts = (C.c_int64 * 2)()
        for name in ("kajo_hip_local", "kajo_hip_lens", "kajo_hip_grade", "kajo_hip_glare"):
            got["radiance/" + name] = (call_radiance(h, name, p), call_radiance(h, name, p))
            got["counts/" + name] = (capi.lib().kajo_hip_despeckle_counts(h, counts), counts[0], counts[1])
        got["meter"] = call_meter(h, p)
        got["metered"] = call_host(h, "kajo_hip_present_metered_argb8", METER + ("tone",), p)
        outside = stage_params()
        outside["view"].x1, outside["view"].y1 = float(W + 10), float(H)
        for name, stages in HOST.items():
            if "view" in stages:
                got["outside/" + name] = (call_host(h, name, tuple(s for s in stages if s != "lens"), outside)[0], error())
        for name, stages in GATHERED.items():
            if "view" in stages:
                got["outside/" + name] = (call_gathered(h, name, stages, outside)[0], error())
    with HipRenderer(scene, W, H, strict=strict) as r:  # no AOVs: nothing to focus a lens by (and no denoiser, which would say so first)
        r.render(2)
        for name, stages in HOST.items():
            if "lens" in stages:
                got["no-aov/" + name] = (call_host(r._h, name, tuple(s for s in stages if s != "denoise"), p)[0], error())
        got["no-aov/kajo_hip_lens"] = (call_radiance(r._h, "kajo_hip_lens", p, ("despeckle", "lens"))[0], error())
    return got


@pytest.fixture(scope="module", params=["fast", "strict"])
def got(request, scenes):
    return collect(scenes["spheres_a1"], request.param == "strict")


def test_host_entries_are_the_whole_chain_with_the_other_stages_null(got):
    for name in HOST:
        rc, words, result = got["host/" + name]
        wrc, wwords, wresult = got["host-whole/" + name]
        assert rc == 0 and wrc == 0, name
        assert np.array_equal(words, wwords) and result == wresult, name
        assert len(np.unique(words)) > 16, name  # an image, not a constant
    # the stages are not the identity: every longer chain gives another image (but for the despeckle, which finds nothing to repair here)
    seen = [got["host/" + n][1].tobytes() for n in HOST if n != "kajo_hip_present_argb8"]
    assert len(set(seen)) == len(seen)


def test_gathered_entries_are_the_whole_chain_with_the_other_stages_null(got):
    for name in GATHERED:
        rc, words, result = got["gathered/" + name]
        wrc, wwords, wresult = got["gathered-whole/" + name]
        assert rc == 0 and wrc == 0, name
        assert np.array_equal(words, wwords) and result == wresult, name
    seen = [got["gathered/" + n][1].tobytes() for n in GATHERED if n != "kajo_hip_present_gathered_argb8_device"]
    assert len(set(seen)) == len(seen)


def test_radiance_entries_repeat_themselves_and_keep_the_despeckle_counts(got):
    for name in RADIANCE:
        (rc0, a), (rc1, b) = got["radiance/" + name]
        assert rc0 == 0 and rc1 == 0 and np.array_equal(a, b), name
        assert np.isfinite(a.view(np.float32)).all() and a.any(), name
        rc, repaired, clamped = got["counts/" + name]
        assert rc == 0 and repaired >= 0 and clamped >= 0, name


def test_meter_measures_the_frame_present_metered_maps(got):
    rc, hist, res = got["meter"]
    prc, _, presult = got["metered"]
    assert rc == 0 and prc == 0
    assert bytes(res) == presult
    assert res.metered == int(hist[1:].sum()) and res.under == int(hist[0]) and res.pixels == W * H


def test_state_refusals_keep_their_code_and_text(got):
    names = list(HOST) + list(GATHERED) + list(RADIANCE) + ["kajo_hip_meter"]
    for name in names:
        assert got["unrendered/" + name] == (STATE, "nothing rendered yet"), name
    lensed = [n for n in HOST if "lens" in HOST[n]] + ["kajo_hip_lens"]
    assert len(lensed) == 4
    for name in lensed:
        assert got["no-aov/" + name] == (STATE, "the handle was created without the AOV flag: no depth to focus the lens by"), name
    viewed = [n for n in list(HOST) + list(GATHERED) if "view" in {**HOST, **GATHERED}[n]]
    assert len(viewed) == 4
    for name in viewed:
        assert got["outside/" + name] == (INVALID, "view rectangle must lie inside the frame"), name
