"""Noise and adaptive handles at every launch shape kajo_hip_render chooses (kajo_amd/csrc/launch_plan.h kajoLaunchShape), not only
S = 4 on spheres_a169: the pass-split kernels without chunks, chunks of 3, 4, 5, 8, 9 and 16 waves, the unsplit kernels with one wave
and with four per block, a small scene planned with four waves (units of 256 slots), three large-scene classes up to the large-LDS
opt-in, KAJO_FLAG_NO_ONE_LIGHT, depth 0 and other launch lengths. tests/adaptive_shape_cases.py names the cases;
tests/test_launch_shapes_cpu.py proves from the host's own plan which path each takes, before and behind the first retirement.

The reference is tests/test_hip_adaptive.py's: a KAJO_FLAG_NOISE twin rendered four passes at a time, the numpy restatement of the rule
over its records, `expected` for what the adaptive handle must hold. Frame, records, pass plane and state are compared bit for bit, for
the cuts (32,), (16, 2, 14), (16, 3, 13) and (1,) * 32 -- a two-pass and a three-pass launch directly behind the first retirement -- one
owner and three, allowance 0. The twin is held too: its frame to a handle without the flag rendered in one call, its records to
tests/test_hip_noise.py's float64 restatement over its own frames. Then the counters flag, KAJO_FLAG_NO_REORDER and a wait behind every
launch must not move a bit, and the guided denoiser and a display chain must read an adaptive handle of 256-slot units as they read a
noise handle that holds the same buffers."""
import ctypes as C

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from adaptive_shape_cases import CASES, CUTS, FLAG_CASES, OWNERS, PASSES, case_scene, create_keywords, launches
from test_hip_adaptive import FLOOR, SEED, expected, median_target, restate, run, same_records, twin, u32, unit_of, unit_slots_of
from test_hip_noise import restate_moments

pytestmark = pytest.mark.gpu

_SCENES, _PLANS = {}, {}


def scene_of(scenes, case):
    if case["scene"] not in _SCENES:
        _SCENES[case["scene"]] = case_scene(scenes, case["scene"])
    return _SCENES[case["scene"]]


def same_frame(a, b):
    """bit for bit, a NaN equal to a NaN"""
    return np.array_equal(u32(a)[~np.isnan(a)], u32(b)[~np.isnan(a)]) and np.array_equal(np.isnan(a), np.isnan(b))


def plan_of(scenes, name):
    """(scene, W, H, S, create keywords, twin frames, twin records, unit slots, target) of a case, the condition of every case asserted:
    with the median target some unit retires at 16 and some unit is still active at 32, for one owner and for three"""
    if name not in _PLANS:
        case = CASES[name]
        sc, (W, H), S, kw = scene_of(scenes, case), case["size"], case["spp"], create_keywords(case)
        frames, records, _ = twin(sc, name, W, H, kw, spp=S)
        slots = unit_slots_of(sc, W, H, spp=S, **kw)
        target = median_target(records, W, H, slots)
        for owners in OWNERS:
            retired = restate(records, W, H, owners, slots, target, 0)
            assert target > 0 and (retired == 16).any() and (retired == 0).any(), (name, owners, target, np.unique(retired))
        _PLANS[name] = (sc, W, H, S, kw, frames, records, slots, target)
    return _PLANS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_twin_is_a_handle_without_the_flag_and_its_records_the_restatement(scenes, name):
    """the noise handle's cut at every fourth pass, at this shape, against the kernels the oracle tests cover: render(32) of a plain handle"""
    sc, W, H, S, kw, frames, records, _, _ = plan_of(scenes, name)
    with HipRenderer(sc, W, H, spp=S, seed=SEED, **kw) as plain:
        want = plain.render(PASSES).radiance()
    assert same_frame(frames[PASSES // 4], want), name
    assert same_records(records[PASSES // 4], restate_moments(frames[1:])), name
    assert same_records(records[4], restate_moments(frames[1:5])), name


@pytest.mark.parametrize("owners", OWNERS, ids=["one-owner", "three-owners"])
@pytest.mark.parametrize("name", list(CASES))
def test_frame_records_pass_plane_and_state_at_every_launch_shape(scenes, name, owners):
    sc, W, H, S, kw, frames, records, slots, target = plan_of(scenes, name)
    n = int(np.sqrt(float(S)))
    retired = restate(records, W, H, owners, slots, target, 0)
    frame, rec, plane = expected(frames, records, retired)
    before = restate(records, W, H, owners, slots, target, 0, passes=16)
    paths = n * n * (16 * W * H + 16 * int((before == 0).sum()))
    _, unit, _ = unit_of(W, H, 1, slots)
    for cuts in CUTS:
        got = run(sc, W, H, cuts, owners, dict(target=target, floor=FLOOR, allowance=0), spp=S, **kw)
        why = (name, owners, cuts)
        assert np.array_equal(u32(got[0]), u32(frame)), (why, np.argwhere((u32(got[0]) != u32(frame)).any(-1))[:4])
        assert same_records(got[1], rec), why
        assert np.array_equal(got[2], plane), (why, np.argwhere(got[2] != plane)[:4])
        s = got[3]
        assert (s["pixels"], s["activePixels"], s["paths"], s["unitSlots"]) == (W * H, int((retired == 0).sum()), paths, slots), (why, s)
        assert s["lastDecisionPass"] == PASSES, (why, s)
        if owners == 1:
            assert s["activeUnits"] == len(np.unique(unit[retired == 0])), (why, s)


VARIANTS = ("counters", "no-reorder", "wait")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", FLAG_CASES)
def test_flags_and_waits_that_must_not_move_a_bit(scenes, name, variant):
    """the counters flag (a short grid writes the counters), KAJO_FLAG_NO_REORDER (no cost order at all, against one that arrives at the
    decision) and a wait behind every launch (the measured cost order arrives before the decision instead of at it)"""
    sc, W, H, S, kw, frames, records, slots, target = plan_of(scenes, name)
    n = int(np.sqrt(float(S)))
    retired = restate(records, W, H, 1, slots, target, 0)
    frame, rec, plane = expected(frames, records, retired)
    ppl = kw.get("passes_per_launch", 0)
    for cuts in CUTS:
        seen = {}

        def behind(p):
            if variant == "wait":
                p.wait()
            if variant == "counters":
                seen.update(p.counters())

        more = dict(kw)
        if variant == "counters":
            more["counters"] = True
        if variant == "no-reorder":
            more["flags"] = more.get("flags", 0) | capi.KAJO_FLAG_NO_REORDER
        got = run(sc, W, H, cuts, 1, dict(target=target, floor=FLOOR, allowance=0), spp=S, behind=behind, **more)
        why = (name, variant, cuts)
        assert np.array_equal(u32(got[0]), u32(frame)), why
        assert same_records(got[1], rec), why
        assert np.array_equal(got[2], plane), why
        assert got[3]["activePixels"] == int((retired == 0).sum()), why
        if variant == "counters":
            # the nominal count: every pass counts every pixel's samples, rendered or not; a launch per cut while a unit is active
            assert seen["passes"] == PASSES and seen["paths"] == W * H * n * n * PASSES, (why, seen)
            assert seen["launches"] == len(launches(cuts, ppl)), (why, seen)


HIP = None


def copy_tile_buffer(dst, src):
    """src's tile buffer over dst's, device to device"""
    global HIP
    HIP = HIP or C.CDLL("libamdhip64.so")
    src.wait()
    dst.wait()
    (sp, sn), (dp, dn) = src.tile_buffer(), dst.tile_buffer()
    assert sn == dn and sn > 0
    assert HIP.hipMemcpy(C.c_void_p(dp), C.c_void_p(sp), C.c_size_t(sn), C.c_int(3)) == 0


@pytest.mark.parametrize("name", FLAG_CASES)
def test_the_guided_denoiser_and_a_chain_read_an_adaptive_handle_as_a_noise_handle_with_its_buffers(scenes, name):
    """Every reader knows nothing of the flag, at a unit of 64 slots and of 256: a KAJO_FLAG_NOISE handle whose tile buffer is overwritten
    with the adaptive handle's and whose noise planes are the adaptive handle's (kajo_hip_denoise_guide_planes: uploaded planes go before
    the handle's own records) gives the same bits. The AOVs are the same already: tests/test_hip_adaptive.py."""
    sc, W, H, S, kw, frames, records, slots, target = plan_of(scenes, name)
    dn = dict(noise_guided=True, iterations=3)
    chain = dict(despeckle={}, glare=dict(strength=0.2), curve="reinhard")
    with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, noise=True, adaptive=dict(target=target, floor=FLOOR, allowance=0), **kw) as r, \
            HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, noise=True, **kw) as t:
        r.render(PASSES)
        t.render(PASSES)
        s = r.adapt_state()
        assert 0 < s["activeUnits"] < s["units"] and s["unitSlots"] == slots, s
        assert not np.array_equal(u32(r.radiance()), u32(frames[PASSES // 4]))  # (retired slots were extended, not rendered)
        copy_tile_buffer(t, r)  # (before anything reads t: a handle composes its frame once per pass count)
        nz = r.noise()
        assert (nz["batches"] == 4).any() and (nz["batches"] == 8).any()
        t.denoise_guide_planes(nz["mean"], nz["stderr"])
        assert np.array_equal(u32(t.radiance()), u32(r.radiance()))
        got, want = r.denoise(**dn), t.denoise(**dn)
        assert np.array_equal(u32(got["radiance"]), u32(want["radiance"])) and np.array_equal(got["argb8"], want["argb8"]), name
        assert not np.array_equal(u32(got["radiance"]), u32(r.denoise(iterations=3)["radiance"]))  # (the planes were looked at)
        (a, sa), (b, sb) = r.present(**chain), t.present(**chain)
        assert np.array_equal(a, b) and sa == sb, name
