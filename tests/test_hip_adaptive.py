"""Adaptive sampling (KAJO_FLAG_ADAPTIVE with KAJO_FLAG_NOISE; include/kajo_hip.h "Adaptive sampling", kajo_amd/csrc/adapt_kernels.cpp) on
the GPU.

The reference is a twin handle with KAJO_FLAG_NOISE alone, rendered four passes at a time: its frames and records after every batch. A
numpy restatement of the rule finds every unit's retirement pass from the twin's records and forms what the adaptive handle must hold:
the twin's frame and records at P for an active unit, twin(p) * (float)(P / p) and the records at p for a unit retired at p. Frame,
records, pass plane and state are compared bit for bit, for every numerics build, ragged and multi-tile frames, a large-scene instance,
the SPLIT and the unsplit kernels, any cut of the passes into calls, one owner and three, allowance 0 and 8. (A slot with a batch that was
not finite has p = 4 n below its unit's retirement pass: `expected` follows the header there.) Two frames large enough for the step and
pass-plane kernels to stride beyond their 2048 workgroups are held to a vectorised restatement, itself held to the loop on the small
cases. Other tile shapes: tests/test_hip_noise_tile_shapes.py."""
import ctypes as C

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, NOISE_MOMENTS
from kajo_amd.tiles import TileLayout
from scenes_extra import dense_scene

pytestmark = pytest.mark.gpu

SEED = 0o715517
F32, F64 = np.float32, np.float64
BUILDS = {"fast": {}, "exact": dict(exact=True), "strict": dict(strict=True)}
CASES = {"spheres-41x23": ("spheres", 41, 23), "spheres-65x9": ("spheres", 65, 9), "spheres-100x75": ("spheres", 100, 75),
         "grid60-41x23": ("grid60", 41, 23)}
CUTS = ((32,), (4, 28), (1, 2, 29), (3, 5, 24), (1,) * 32)
FLOOR = 1e-2
PASSES = 32
HUGE, TINY = 1e30, 1e-30


@pytest.fixture(scope="module")
def the_scenes(scenes):
    return {"spheres": scenes["spheres_a169"], "grid60": dense_scene(scenes["spheres_a169"], 60, 3, seed=11)}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_records(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in ("s1", "s2", "n", "bad"))


_TWINS = {}


def twin(sc, key, W, H, kw, spp=4):
    """frames[b], records[b] after batch b = 1 .. 8 of a KAJO_FLAG_NOISE handle (index 0: nothing rendered); rendered once per case.
    kw: the create keywords of the case (tests/test_hip_adaptive_launch_shapes.py: other sample counts, depths, launch lengths)"""
    k = (key, W, H, spp, tuple(sorted(kw.items())))
    if k not in _TWINS:
        with HipRenderer(sc, W, H, spp=spp, seed=SEED, noise=True, **kw) as t:
            frames, records = [np.zeros((H, W, 4), F32)], [t.noise_moments()]
            for _ in range(PASSES // 4):
                frames.append(t.render(4).radiance().copy())
                records.append(t.noise_moments())
            launches = t.counters()["launches"]
        for a in frames + records:
            a.setflags(write=False)
        _TWINS[k] = (frames, records, launches)
    return _TWINS[k]


def rel32(rec, floor=FLOOR):
    """the estimate's evaluation in float64, rounded to float32; -1 with fewer than two batches"""
    n = rec["n"].astype(F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = rec["s1"] / (4.0 * n)
        v = np.maximum(rec["s2"] - rec["s1"] * rec["s1"] / n, 0.0) / (n - 1.0)
        rel = (np.sqrt(v / n) / 4.0) / (np.maximum(m, 0.0) + F64(F32(floor)))
    return np.where(rec["n"] >= 2, rel, -1.0).astype(F32)


def unit_of(W, H, owners, unit_slots, tile=(64, 16)):
    """per pixel: (owner, unit of the owner, pixel block of the owner)"""
    ys, xs = np.mgrid[0:H, 0:W]
    owner, slot = TileLayout(W, H, owners, tile).owner_and_slot(xs, ys)
    return owner, slot // unit_slots, slot // 64


def restate(records, W, H, owners, unit_slots, target, allowance, passes=PASSES, min_passes=16, every=4, tile=(64, 16)):
    """-> the pass every pixel's unit retired at (0: still active after `passes`)"""
    owner, unit, block = unit_of(W, H, owners, unit_slots, tile)
    ukey = owner.astype(np.int64) * (1 << 32) + unit
    bkey = owner.astype(np.int64) * (1 << 32) + block
    retired = np.zeros((H, W), np.int64)
    for P in range(4 * every, passes + 1, 4 * every):
        if P < min_passes:
            continue
        rec = records[P // 4]
        loud = (rec["n"] < 2) | (rel32(rec) > F32(target))
        for u in np.unique(ukey[retired == 0]):
            inside = ukey == u
            quiet = all(loud[inside & (bkey == b)].sum() <= allowance for b in np.unique(bkey[inside]))
            if quiet:
                retired[inside] = P
    return retired


def restate_fast(records, W, H, owners, unit_slots, target, allowance, passes=PASSES, min_passes=16, every=4, tile=(64, 16)):
    """restate() without its loop over units: the loud pixels of every pixel block counted with np.bincount over the blocks' keys, a unit
    quiet when none of its blocks is over the allowance (np.minimum.at over the blocks' units). The test below holds it equal to restate()
    on every small case; the frames of many thousands of units use it."""
    owner, unit, block = unit_of(W, H, owners, unit_slots, tile)
    _, ui = np.unique(owner.astype(np.int64) * (1 << 32) + unit, return_inverse=True)
    _, bi = np.unique(owner.astype(np.int64) * (1 << 32) + block, return_inverse=True)
    ui, bi = ui.reshape(-1), bi.reshape(-1)
    unit_of_block = np.zeros(bi.max() + 1, np.int64)
    unit_of_block[bi] = ui  # (every pixel of a block lies in one unit)
    assert np.array_equal(unit_of_block[bi], ui)
    retired_unit = np.zeros(ui.max() + 1, np.int64)
    for P in range(4 * every, passes + 1, 4 * every):
        if P < min_passes:
            continue
        rec = records[P // 4]
        loud = ((rec["n"] < 2) | (rel32(rec) > F32(target))).reshape(-1)
        count = np.bincount(bi, weights=loud, minlength=unit_of_block.size).astype(np.int64)
        quiet = np.ones(retired_unit.size, np.int64)
        np.minimum.at(quiet, unit_of_block, (count <= allowance).astype(np.int64))
        retired_unit[(quiet == 1) & (retired_unit == 0)] = P
    return retired_unit[ui].reshape(H, W)


def expected(frames, records, retired, P=PASSES):
    """What the adaptive handle holds after P passes. A slot retired at p is its frame at p times (float)(P / (4 n)) and reports 4 n, n the
    slot's own finite batches (include/kajo_hip.h "WHAT EVERY READER SEES"): p itself unless a batch of the slot was not finite; with n = 0
    the slot is left as it was."""
    frame, rec = frames[P // 4].copy(), records[P // 4].copy()
    plane = np.full(retired.shape, P, np.uint32)
    for p in np.unique(retired[retired > 0]):
        at = retired == p
        base, r = frames[p // 4][at], records[p // 4][at]
        own = 4.0 * r["n"].astype(F64)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            f = (F64(P) / own).astype(F32)
            frame[at] = np.where((own > 0)[:, None], base * f[:, None], base)
        rec[at] = r
        plane[at] = (4 * r["n"]).astype(np.uint32)
    return frame, rec, plane


def median_target(records, W, H, unit_slots):
    """the median of the units' worst relative error at pass 16"""
    _, unit, _ = unit_of(W, H, 1, unit_slots)
    rel = rel32(records[4])
    assert (records[4]["n"] >= 2).all()
    return float(F32(np.median([rel[unit == u].max() for u in np.unique(unit)])))


HIP = None


def tile_frame(parts, W, H, tile=(64, 16)):
    """the owners' tile buffers, composed on the host"""
    global HIP
    HIP = HIP or C.CDLL("libamdhip64.so")
    layout = TileLayout(W, H, len(parts), tile)
    g = np.zeros((len(parts), layout.slots_per_owner, 4), F32)
    for i, p in enumerate(parts):
        p.wait()
        ptr, nbytes = p.tile_buffer()
        assert nbytes == g[i].nbytes
        assert HIP.hipMemcpy(g[i].ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), C.c_int(2)) == 0
    return layout.compose(g)


def run(sc, W, H, cuts, owners, adaptive, spp=4, behind=None, **kw):
    """behind: called with the owner's handle behind every render call (a wait, a look at the counters)"""
    parts = [HipRenderer(sc, W, H, spp=spp, seed=SEED, noise=True, adaptive=adaptive, tile_index=i, tile_count=owners, **kw) for i in range(owners)]
    try:
        rec, plane = np.zeros((H, W), NOISE_MOMENTS), np.zeros((H, W), np.uint32)
        state = {}
        for p in parts:
            for c in cuts:
                p.render(c)
                if behind:
                    behind(p)
            p.noise_moments(out=rec)
            p.adapt_passes(out=plane)
            s = p.adapt_state()
            for k, v in s.items():  # (the owners' counts add; an owner without a tile decides nothing)
                state[k] = max(state.get(k, 0), v) if k in ("lastDecisionPass", "unitSlots") else state.get(k, 0) + v
        frame = parts[0].radiance().copy() if owners == 1 else tile_frame(parts, W, H, kw.get("tile", (64, 16)))
        return frame, rec, plane, state
    finally:
        for p in parts:
            p.close()


def unit_slots_of(sc, W, H, spp=4, **kw):
    with HipRenderer(sc, W, H, spp=spp, seed=SEED, noise=True, adaptive=True, **kw) as r:
        return r.adapt_state()["unitSlots"]


@pytest.mark.parametrize("nosplit", [False, True], ids=["split", "nosplit"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("build", list(BUILDS))
def test_frame_records_pass_plane_and_state_are_the_restatement_bit_for_bit(the_scenes, build, case, nosplit):
    key, W, H = CASES[case]
    sc = the_scenes[key]
    kw = dict(BUILDS[build], flags=capi.KAJO_FLAG_NO_SPLIT if nosplit else 0)
    frames, records, _ = twin(sc, key, W, H, kw)
    slots = unit_slots_of(sc, W, H, **kw)
    target = median_target(records, W, H, slots)
    for allowance in (0, 8):
        params = dict(target=target, floor=FLOOR, allowance=allowance)
        for owners in (1, 3):
            retired = restate(records, W, H, owners, slots, target, allowance)
            if allowance == 0:
                assert (retired == 16).any() and (retired == 0).any(), (case, np.unique(retired))
            frame, rec, plane = expected(frames, records, retired)
            before = restate(records, W, H, owners, slots, target, allowance, passes=16)
            paths = 4 * 16 * (W * H + int((before == 0).sum()))
            composed = {}
            for cuts in CUTS:
                got = run(sc, W, H, cuts, owners, params, **kw)
                why = (build, case, nosplit, allowance, owners, cuts)
                assert np.array_equal(u32(got[0]), u32(frame)), why
                assert same_records(got[1], rec), why
                assert np.array_equal(got[2], plane), why
                s = got[3]
                assert (s["pixels"], s["activePixels"], s["paths"], s["unitSlots"]) == (W * H, int((retired == 0).sum()), paths, slots), (why, s)
                # (a handle whose units have all retired decides nothing more)
                assert s["lastDecisionPass"] == (PASSES if (before == 0).any() else 16), (why, s)
                composed[owners] = s
            if owners == 3:
                one = run(sc, W, H, (PASSES,), 1, params, **kw)[3]
                assert (composed[3]["units"], composed[3]["activeUnits"]) == (one["units"], one["activeUnits"]), (composed[3], one)
            else:
                # the units the image does not reach retire at the first decision; those it reaches, by the restatement
                _, unit, _ = unit_of(W, H, 1, slots)
                assert composed[1]["activeUnits"] == len(np.unique(unit[retired == 0])), (composed[1], case)


@pytest.mark.parametrize("case", list(CASES))
def test_the_vectorised_restatement_is_the_loop_on_every_small_case(the_scenes, case):
    """restate_fast, which the frames of thousands of units need, against restate: the same retirement pass for every pixel, allowance 0
    and 8, one owner and three, decisions at 16 and 32."""
    key, W, H = CASES[case]
    sc = the_scenes[key]
    kw = dict(BUILDS["exact"], flags=0)
    _, records, _ = twin(sc, key, W, H, kw)
    slots = unit_slots_of(sc, W, H, **kw)
    target = median_target(records, W, H, slots)
    for allowance in (0, 8):
        for owners in (1, 3):
            slow = restate(records, W, H, owners, slots, target, allowance)
            assert np.array_equal(restate_fast(records, W, H, owners, slots, target, allowance), slow), (case, allowance, owners)
            assert np.array_equal(restate_fast(records, W, H, owners, slots, target, allowance, passes=16),
                                  restate(records, W, H, owners, slots, target, allowance, passes=16)), (case, allowance, owners)
            if allowance == 0:
                assert (slow == 16).any() and (slow == 0).any(), (case, np.unique(slow))


# The smallest frames, with one owner and the default tile, at which kajo_adapt_step's and kajo_adapt_passes' grids meet their cap
# (adapt_kernels.cpp KAJO_ADAPT_MAX_GROUPS) and a workgroup strides: more than 2048 x 256 slots, more than 2048 rectangles of 64x4.
MAX_GROUPS = 2048
STRIDED = [((9, 8200), "fast"), ((9, 8200), "exact"), ((9, 8200), "strict"), ((1001, 523), "exact")]


@pytest.mark.parametrize("size,build", STRIDED, ids=["%dx%d-%s" % (s + (b,)) for s, b in STRIDED])
def test_strided_launches_give_the_restatement_beyond_the_first_2048_workgroups(the_scenes, size, build):
    """20 passes cut (16, 4): one decision at 16, a step with retired units behind the second launch, a batch boundary at 20. The target is
    the lower median of the worst relative error at pass 16 of the units beyond slot 524 288 -- the image's last tile row -- so that one of
    them at least retires and one stays active there."""
    sc, (W, H), P = the_scenes["spheres"], size, 20
    kw = BUILDS[build]
    lay = TileLayout(W, H, 1)
    rects = ((W + 63) // 64) * ((H + 3) // 4)
    assert lay.slots_per_owner > MAX_GROUPS * 256 and rects > MAX_GROUPS, (size, lay.slots_per_owner, rects)
    with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, **kw) as t:
        frames, records = [np.zeros((H, W, 4), F32)], [t.noise_moments()]
        for _ in range(P // 4):
            frames.append(t.render(4).radiance().copy())
            records.append(t.noise_moments())
    slots = unit_slots_of(sc, W, H, **kw)
    ys, xs = np.mgrid[0:H, 0:W]
    beyond = lay.owner_and_slot(xs, ys)[1] >= MAX_GROUPS * 256
    _, unit, _ = unit_of(W, H, 1, slots)
    rel = rel32(records[4])
    assert beyond.any() and (records[4]["n"][beyond] >= 2).all()
    assert not np.isin(unit[~beyond], unit[beyond]).any()  # (a unit lies on one side)
    worst = np.sort([rel[beyond][unit[beyond] == u].max() for u in np.unique(unit[beyond])])
    target = float(worst[(len(worst) - 1) // 2])
    assert len(worst) >= 2 and target > 0 and worst[-1] > target, (size, build, worst)
    retired = restate_fast(records, W, H, 1, slots, target, 0, passes=P)
    assert (retired[beyond] == 16).any() and (retired[beyond] == 0).any() and (retired[~beyond] == 16).any() and (retired[~beyond] == 0).any()
    frame, rec, plane = expected(frames, records, retired, P=P)
    got = run(sc, W, H, (16, 4), 1, dict(target=target, floor=FLOOR, allowance=0), **kw)
    why = (size, build)
    for where, at in (("beyond slot 524 288", beyond), ("the whole frame", np.ones((H, W), bool))):
        assert np.array_equal(u32(got[0][at]), u32(frame[at])), (why, where)
        assert same_records(got[1][at], rec[at]), (why, where)
        assert np.array_equal(got[2][at], plane[at]), (why, where, np.argwhere((got[2] != plane) & at)[:4])
    s = got[3]
    active = int((retired == 0).sum())
    assert (s["pixels"], s["activePixels"], s["paths"], s["unitSlots"]) == (W * H, active, 4 * (16 * W * H + 4 * active), slots), (why, s)
    assert s["lastDecisionPass"] == 16 and s["activeUnits"] == len(np.unique(unit[retired == 0])), (why, s)


def test_retired_slots_are_extended_behind_every_launch_not_only_at_boundaries(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    frames, records, _ = twin(sc, "spheres", W, H, dict(exact=True))
    slots = unit_slots_of(sc, W, H, exact=True)
    target = median_target(records, W, H, slots)
    retired = restate(records, W, H, 1, slots, target, 0, passes=16)
    with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, exact=True) as t:
        at18 = t.render(18).radiance().copy()
    with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, exact=True, adaptive=dict(target=target)) as r:
        got = r.render(16).render(2).radiance()
        plane = r.adapt_passes()
        assert r.adapt_state()["lastDecisionPass"] == 16
    want = np.where((retired > 0)[..., None], frames[4] * F32(F64(18) / F64(16)), at18)
    assert (retired > 0).any() and (retired == 0).any()
    assert np.array_equal(u32(got), u32(want))
    assert np.array_equal(plane, np.where(retired > 0, 16, 18))


@pytest.mark.parametrize("nosplit", [False, True], ids=["split", "nosplit"])
def test_with_everything_retired_no_render_kernel_is_launched_and_the_image_stands(the_scenes, nosplit):
    sc, (W, H) = the_scenes["spheres"], (100, 75)
    kw = dict(exact=True, flags=capi.KAJO_FLAG_NO_SPLIT if nosplit else 0)
    with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, adaptive=dict(target=HUGE), **kw) as r:
        r.render(16)
        s = r.adapt_state()
        assert (s["activeUnits"], s["activePixels"], s["lastDecisionPass"]) == (0, 0, 16) and s["units"] > 0
        image, launches, frame = r.argb8().copy(), r.counters()["launches"], r.radiance().copy()
        assert launches == 4
        r.render(16)
        c = r.counters()
        assert (c["launches"], c["passes"]) == (launches, 32)
        after = r.argb8()
        channels = lambda a: np.stack([(a >> k) & 255 for k in (0, 8, 16, 24)], -1).astype(np.int64)
        assert np.abs(channels(after) - channels(image)).max() <= 1
        assert np.array_equal(u32(r.radiance()), u32(frame * F32(2)))
        assert (r.adapt_passes() == 16).all()
        s = r.adapt_state()
        assert (s["paths"], s["lastDecisionPass"]) == (4 * 16 * W * H, 16)
        # reset: every unit active again, and the rule may be given anew
        r.reset()
        s = r.adapt_state()
        assert (s["activeUnits"], s["activePixels"], s["paths"], s["lastDecisionPass"]) == (s["units"], W * H, 0, 0)
        r.set_adaptive(dict(target=TINY))
        r.render(16)
        assert np.array_equal(u32(r.radiance()), u32(frame))
        with pytest.raises(capi.KajoError) as e:
            r.set_adaptive(dict(target=HUGE))
        assert e.value.code == capi.KAJO_E_STATE
        with pytest.raises(capi.KajoError) as e:
            r.set_pass_count(8)
        assert e.value.code == capi.KAJO_E_STATE and r.counters()["passes"] == 16


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("rule", ["unmet", "unset"])
def test_a_target_nothing_meets_or_no_rule_at_all_is_the_noise_twin(the_scenes, build, rule):
    sc, (W, H) = the_scenes["spheres"], (100, 75)
    frames, records, launches = twin(sc, "spheres", W, H, BUILDS[build])
    with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, adaptive=dict(target=TINY) if rule == "unmet" else True, **BUILDS[build]) as r:
        for c in (4,) * 8:
            r.render(c)
        assert np.array_equal(u32(r.radiance()), u32(frames[8])) and same_records(r.noise_moments(), records[8])
        assert r.counters()["launches"] == launches
        s = r.adapt_state()
        assert s["activePixels"] == W * H and s["lastDecisionPass"] == (32 if rule == "unmet" else 0) and (r.adapt_passes() == 32).all()


def test_the_aov_buffers_are_those_of_a_plain_handle(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    frames, records, _ = twin(sc, "spheres", W, H, dict(exact=True))
    target = median_target(records, W, H, unit_slots_of(sc, W, H, exact=True))
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, aov=True) as plain:
        want = plain.render(32).aov()
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, aov=True, noise=True, adaptive=dict(target=target)) as r:
        got = r.render(32).aov()
        s = r.adapt_state()
        assert 0 < s["activeUnits"] < s["units"]
    assert np.array_equal(u32(got["raw"][0]), u32(want["raw"][0])) and np.array_equal(u32(got["raw"][1]), u32(want["raw"][1]))


def test_a_nan_in_the_accumulation_does_not_keep_its_unit_from_retiring(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    x, y = 17, 9
    hip = C.CDLL("libamdhip64.so")
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, noise=True, adaptive=dict(target=HUGE)) as r:
        r.render(8).wait()
        _, slot = TileLayout(W, H, 1).owner_and_slot(x, y)
        ptr, nbytes = r.tile_buffer()
        assert 0 <= int(slot) * 16 + 16 <= nbytes
        nan = np.full(4, np.nan, F32)
        assert hip.hipMemcpy(C.c_void_p(ptr + int(slot) * 16), nan.ctypes.data_as(C.c_void_p), C.c_size_t(16), C.c_int(1)) == 0
        r.render(8)
        rec = r.noise_moments()
        assert (rec["bad"][y, x], rec["n"][y, x]) == (2, 2)
        s = r.adapt_state()
        assert s["activeUnits"] == 0 and s["lastDecisionPass"] == 16
        assert r.adapt_passes()[y, x] == 8


# ---- the driver: hip::Scheduler's real gather path ------------------------------------------------------------------------------------

import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")


def driver(tmp_path, name, *extra):
    out = str(tmp_path / (name + ".png"))
    cmd = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--spp", "4", "-o", out, "--json", "--sample-map", str(tmp_path / (name + ".pfm")), *extra]
    p = subprocess.run(cmd + [os.path.join(ROOT, "kajo_amd", "data", "caustics.json")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1]), open(out, "rb").read(), open(str(tmp_path / (name + ".pfm")), "rb").read()


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_adaptive_one_gpu_and_three_owners_write_the_same_image_and_sample_map(tmp_path):
    # a target from the frame's own estimate: the 0.5 quantile of the relative error at 32 passes, so that some units retire and others do not
    # (--batch 16 everywhere: the scheduler's own refreshes follow measured time, and a run that ends because no unit is active ends at a
    # refresh; with fixed refreshes the pass a run ends at is the same for any number of owners)
    probe, _, _ = driver(tmp_path, "p", "--adaptive", "1e-30", "--max-passes", "32", "--noise-quantile", "0.5", "--batch", "16")
    E = probe["noise_quantile_value"]
    assert E > 0 and probe["passes"] == 32 and probe["adaptive_stopped_at_pass"] == 0 and probe["adaptive_units"] > 0
    one, png1, map1 = driver(tmp_path, "a", "--adaptive", repr(E), "--max-passes", "64", "--batch", "16")
    three, png3, map3 = driver(tmp_path, "b", "--adaptive", repr(E), "--max-passes", "64", "--batch", "16", "--gpus", "3", "--same-device")
    assert png1 == png3 and map1 == map3
    for k in ("passes", "adaptive_active_units", "adaptive_units", "adaptive_paths", "adaptive_stopped_at_pass"):
        assert one[k] == three[k], (k, one[k], three[k])
    # (the first holds for any target: at 96x54 the units the image does not reach retire at pass 16. The second is the one that shows a
    # retirement inside the image: fewer camera paths than pixels * n^2 * passes)
    assert one["adaptive_active_units"] < one["adaptive_units"] and 0 < one["adaptive_paths"] < 96 * 54 * 4 * one["passes"]
    plane = np.frombuffer(map1[-96 * 54 * 4:], "<f4")
    assert plane.max() == one["passes"] or one["adaptive_stopped_at_pass"] == one["passes"]
    assert (plane % 16 == 0).all() or plane.max() == one["passes"]
    # with a target everything meets the run ends at the first refresh behind the first decision; with --until-noise too, whichever rule ends first
    # (--batch 4: the scheduler looks at the states after every batch)
    done, _, _ = driver(tmp_path, "c", "--adaptive", "1e30", "--until-noise", "1e-30", "--batch", "4")
    assert (done["passes"], done["adaptive_stopped_at_pass"], done["adaptive_active_units"], done["noise_stopped_at_pass"]) == (16, 16, 0, 0)
