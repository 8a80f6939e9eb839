"""The noise estimate (KAJO_FLAG_NOISE; include/kajo_hip.h "The noise estimate", kajo_hip_noise, kajo_hip_read_noise_moments;
kajo_amd/csrc/noise.hip) on the GPU.

The definition is restated in numpy from the frames of a twin handle WITHOUT the flag, rendered four passes at a time (float32
differences and luminance, float64 moments): the records must be the same bits. The evaluation (m, se, rel) is held to 2 float32 ulp of
the float64 restatement -- the largest difference measured over every case below, FAST / EXACT / STRICT, both scenes, all five frames:
0.5 ulp, that is, the float32 nearest to the float64 value -- and the histogram to the restatement's bins wherever rel is further than that from a bin edge. Then: the records do not
depend on how the passes are cut into calls, launches or owners; the flag leaves the frame, the AOVs and the image alone; a NaN in the
accumulation marks its own pixel and no other; reset / set_pass_count / fewer than two batches; the driver's stop rule; and two frames
large enough for both kernels to stride beyond their 2048 workgroups. Other tile shapes: tests/test_hip_noise_tile_shapes.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import read_pfm
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, NOISE_MOMENTS, noise_evaluate
from kajo_amd.tiles import TileLayout
from scenes_extra import dense_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
SEED = 0o715517
F32, F64 = np.float32, np.float64
BUILDS = {"fast": {}, "exact": dict(exact=True), "strict": dict(strict=True)}
SIZES = [(1, 1), (7, 5), (41, 23), (65, 9), (100, 75)]
BINS, BASE = 514, (127 - 16) << 4
ULPS = 2  # the evaluation against the float64 restatement, in float32 ulp
FLOOR = 1e-2


@pytest.fixture(scope="module")
def the_scenes(scenes):
    return {"spheres": scenes["spheres_a43"], "grid60": dense_scene(scenes["spheres_a169"], 60, 3, seed=11)}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_records(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in ("s1", "s2", "n", "bad"))


def restate_moments(frames, base=None):
    """frames: the accumulation (H, W, 4) float32 after every batch, in order; base: the one in front of the first (None: T_0 = 0) -> the
    records of include/kajo_hip.h"""
    shape = frames[0].shape[:2]
    rec = np.zeros(shape, NOISE_MOMENTS)
    base = np.zeros(frames[0].shape, F32) if base is None else base
    with np.errstate(invalid="ignore", over="ignore"):
        for T in frames:
            D = T - base
            y = F32(0.2126) * D[..., 0] + F32(0.7152) * D[..., 1] + F32(0.0722) * D[..., 2]
            assert y.dtype == F32
            ok = np.isfinite(y)
            d = np.where(ok, y.astype(F64), 0.0)
            rec["n"] += ok
            rec["s1"] = np.where(ok, rec["s1"] + d, rec["s1"])
            rec["s2"] = np.where(ok, rec["s2"] + d * d, rec["s2"])
            rec["bad"] += ~ok
            base = T
    return rec


def restate_evaluation(rec, floor=FLOOR):
    """-> m, se, rel in float64 (se = rel = -1 where n < 2)"""
    n = rec["n"].astype(F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(n > 0, rec["s1"] / (4.0 * n), 0.0)
        v = np.maximum(rec["s2"] - rec["s1"] * rec["s1"] / n, 0.0) / (n - 1.0)
        se = np.sqrt(v / n) / 4.0
        rel = se / (np.maximum(m, 0.0) + F64(F32(floor)))
    known = rec["n"] >= 2
    return m, np.where(known, se, -1.0), np.where(known, rel, -1.0)


def bin_of(rel32):
    k = (u32(rel32.astype(F32)) & 0x7fffffff) >> 19
    return np.where(k < BASE, 0, np.minimum(k.astype(np.int64) - BASE + 1, BINS - 1))


def ulps(got32, want64):
    """|got - want| in units of the float32 ulp at want"""
    want32 = want64.astype(F32)
    ulp = np.spacing(np.abs(want32)).astype(F64)
    return np.abs(got32.astype(F64) - want64) / ulp


def twin_frames(sc, W, H, batches, **kw):
    with HipRenderer(sc, W, H, spp=4, seed=SEED, **kw) as t:
        assert t.counters()["launches"] == 0
        return [t.render(4).radiance().copy() for _ in range(batches)]


WORST = {"ulp": 0.0}


def check_map(out, want, W, H, rows=slice(None)):
    """noise()'s planes, histogram and counts against the restatement of the records `want`; `rows`: the planes of these rows alone (the
    histogram and the counts are the whole frame's either way) -> the largest difference of the planes in float32 ulp"""
    m, se, rel = restate_evaluation(want)
    worst = max(ulps(out["mean"][rows], m[rows]).max(), ulps(out["stderr"][rows], se[rows]).max(), ulps(out["relative"][rows], rel[rows]).max())
    assert worst <= ULPS, (W, H, rows, worst)
    assert np.array_equal(out["batches"][rows], want["n"][rows].astype(np.uint32))
    # the histogram: the device's own rel plane binned gives its words; its bins are the restatement's away from the bin edges
    rel32 = rel.astype(F32)
    lo, hi = rel32.copy(), rel32.copy()
    for _ in range(ULPS):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
    known = want["n"] >= 2
    near_edge = known & (bin_of(np.maximum(lo, 0)) != bin_of(hi))
    assert near_edge.sum() <= 0.001 * W * H, (near_edge.sum(), W * H)
    assert np.array_equal(np.bincount(bin_of(out["relative"][known]), minlength=BINS), out["hist"][:BINS])
    at = np.zeros((H, W), bool)
    at[rows] = True
    at &= known & ~near_edge
    assert np.array_equal(bin_of(out["relative"])[at], bin_of(rel32)[at])
    assert out["hist"][BINS] == (~known).sum() and out["hist"][BINS + 1] == (want["bad"] > 0).sum()
    assert (out["pixels"], out["known"], out["unknown"], out["bad"]) == (W * H, known.sum(), (~known).sum(), (want["bad"] > 0).sum())
    assert out["quantile_value"] == noise_evaluate(out["hist"], 0.95) and (out["quantile_value"] > 0) == bool(known.any())
    return worst


@pytest.mark.parametrize("scene", ["spheres", "grid60"])
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_records_are_the_restatement_bit_for_bit_and_the_map_within_two_ulp(the_scenes, scene, build, size):
    sc, (W, H) = the_scenes[scene], size
    want = restate_moments(twin_frames(sc, W, H, 4, **BUILDS[build]))
    with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, **BUILDS[build]) as r:
        r.render(16)
        got = r.noise_moments()
        out = r.noise(floor=FLOOR, quantile=0.95)
    assert (want["n"] + want["bad"] == 4).all() and (want["n"] == 4).mean() > 0.99
    assert same_records(got, want), (scene, build, size)
    worst = check_map(out, want, W, H)
    WORST["ulp"] = max(WORST["ulp"], worst)
    print("%s %s %dx%d: largest difference %.3g ulp (largest so far %.3g)" % (scene, build, W, H, worst, WORST["ulp"]))


# The smallest frames, with one owner and the default tile, at which both kernels' grids meet their cap (noise.hip KAJO_NOISE_MAX_GROUPS) and
# a workgroup strides: more than 2048 x 256 slots for the update, more than 2048 rectangles of 64x4 for the map. 9x8200 is one tile wide
# (1 x 513 tiles); 1001x523 is 16 x 33 tiles, ragged on both axes. Every frame below those sizes -- all the others of this module -- runs
# each loop once.
MAX_GROUPS = 2048
STRIDED = [((9, 8200), "fast"), ((9, 8200), "exact"), ((9, 8200), "strict"), ((1001, 523), "exact")]


def strided_sizes(W, H):
    """-> (slots of the one owner's buffer, rectangles of the map kernel), both held above the caps"""
    slots, rects = TileLayout(W, H, 1).slots_per_owner, ((W + 63) // 64) * ((H + 3) // 4)
    assert slots > MAX_GROUPS * 256 and rects > MAX_GROUPS, (W, H, slots, rects)
    return slots, rects


@pytest.mark.parametrize("size,build", STRIDED, ids=["%dx%d-%s" % (s + (b,)) for s, b in STRIDED])
def test_strided_launches_give_the_restatement_beyond_the_first_2048_workgroups(the_scenes, size, build):
    """8 passes, two batches: se and rel are known. The slots beyond the first 524 288 and the rectangles beyond the first 2 048 are the
    image's last tile row, the last 16 rows at the most: they are compared once more on their own, so that a failure there is named."""
    sc, (W, H) = the_scenes["spheres"], size
    slots, rects = strided_sizes(W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    beyond = TileLayout(W, H, 1).owner_and_slot(xs, ys)[1] >= MAX_GROUPS * 256
    last = slice(H - 16, H)
    assert beyond.any() and not beyond[:H - 16].any()
    assert 4 * (MAX_GROUPS // ((W + 63) // 64)) >= H - 16  # (rectangle 2048, row-major in rows of four, starts in the last 16 rows too)
    want = restate_moments(twin_frames(sc, W, H, 2, **BUILDS[build]))
    with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, **BUILDS[build]) as r:
        r.render(8)
        got = r.noise_moments()
        out = r.noise(floor=FLOOR, quantile=0.95)
    assert (want["n"] + want["bad"] == 2).all() and (want["n"] == 2).mean() > 0.99 and (want["n"][last] == 2).any()
    assert same_records(got[last], want[last]), (size, build, "the last 16 rows")
    assert same_records(got, want), (size, build)
    worst = check_map(out, want, W, H, rows=last)
    worst = max(worst, check_map(out, want, W, H))
    print("%s %dx%d: %d slots, %d rectangles, largest difference %.3g ulp" % (build, W, H, slots, rects, worst))


def run_cuts(sc, W, H, cuts, ppl, owners, **kw):
    parts = [HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, passes_per_launch=ppl, tile_index=i, tile_count=owners, **kw)
             for i in range(owners)]
    try:
        rec, hist, planes, pixels = np.zeros((H, W), NOISE_MOMENTS), np.zeros(capi.KAJO_NOISE_HIST_WORDS, np.uint64), None, 0
        rec["n"] = 99  # (every pixel has one owner: nothing of this is left)
        for p in parts:
            for c in cuts:
                p.render(c)
            p.noise_moments(out=rec)
            planes = p.noise(out=planes)
            hist += planes["hist"]
            pixels += planes["pixels"]
        assert pixels == W * H
        return rec, hist, planes["relative"].copy()
    finally:
        for p in parts:
            p.close()


@pytest.mark.parametrize("build", list(BUILDS))
def test_any_cut_into_calls_launches_and_owners_gives_the_same_records_and_histogram(the_scenes, build):
    sc, (W, H) = the_scenes["spheres"], (100, 75)
    want = run_cuts(sc, W, H, (16,), 16, 1, **BUILDS[build])
    assert (want[0]["n"] + want[0]["bad"] == 4).all() and want[1][:BINS + 1].sum() == W * H
    for owners in (1, 3):
        for ppl in (3, 16):
            for cuts in ((16,), (4, 12), (1, 2, 13), (3, 5, 8), (1,) * 16):
                got = run_cuts(sc, W, H, cuts, ppl, owners, **BUILDS[build])
                assert same_records(got[0], want[0]), (build, owners, ppl, cuts)
                assert np.array_equal(got[1], want[1]) and np.array_equal(u32(got[2]), u32(want[2])), (build, owners, ppl, cuts)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("size", [(41, 23), (100, 75)], ids=lambda s: "%dx%d" % s)
def test_the_flag_leaves_the_frame_the_aovs_and_the_image_alone(the_scenes, build, size):
    sc, (W, H) = the_scenes["spheres"], size
    got = {}
    for noise in (False, True):
        for ppl in (0, 3):
            with HipRenderer(sc, W, H, spp=4, seed=SEED, aov=True, noise=noise, passes_per_launch=ppl, **BUILDS[build]) as r:
                r.render(16)
                a = r.aov()
                got[noise, ppl] = (r.radiance().copy(), a["raw"][0].copy(), a["raw"][1].copy(), r.argb8().copy(), r.counters()["launches"])
                if not noise:
                    with pytest.raises(capi.KajoError) as e:
                        r.noise()
                    assert e.value.code == capi.KAJO_E_STATE
                    with pytest.raises(capi.KajoError) as e:
                        r.noise_moments()
                    assert e.value.code == capi.KAJO_E_STATE
    for ppl in (0, 3):
        for a, b in zip(got[False, ppl][:4], got[True, ppl][:4]):
            assert np.array_equal(u32(a), u32(b)), (build, size, ppl)
    # an unflagged handle launches what it did: 16 passes in one launch, or in six of three at the most; a flagged one never crosses a
    # multiple of four: four launches, or [1-3] [4] [5-7] [8] ...
    assert [got[k][4] for k in ((False, 0), (False, 3), (True, 0), (True, 3))] == [1, 6, 4, 8]


def test_a_nan_in_the_accumulation_marks_its_pixel_and_no_other(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    x, y = 17, 9
    hip = C.CDLL("libamdhip64.so")
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, noise=True) as clean:
        want = clean.render(12).noise_moments()
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, noise=True) as r:
        r.render(8).wait()
        _, slot = TileLayout(W, H, 1).owner_and_slot(x, y)
        ptr, nbytes = r.tile_buffer()
        assert 0 <= int(slot) * 16 + 16 <= nbytes
        nan = np.full(4, np.nan, F32)
        assert hip.hipMemcpy(C.c_void_p(ptr + int(slot) * 16), nan.ctypes.data_as(C.c_void_p), C.c_size_t(16), C.c_int(1)) == 0
        got = r.render(4).noise_moments()
        out = r.noise()
    assert want["bad"][y, x] == 0 and want["n"][y, x] == 3
    assert (got["bad"][y, x], got["n"][y, x]) == (1, 2)
    others = np.ones((H, W), bool)
    others[y, x] = False
    assert same_records(got[others], want[others])
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, noise=True) as two:
        first = two.render(8).noise_moments()
    assert all(got[k][y, x] == first[k][y, x] for k in ("s1", "s2", "n"))  # the pixel keeps the two batches it had
    already = int((want["bad"] > 0).sum())
    assert (out["bad"], out["known"] + out["unknown"]) == (already + 1, W * H) and out["hist"][BINS + 1] == already + 1


def test_reset_set_pass_count_and_unknown_pixels(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (65, 9)
    frames = twin_frames(sc, W, H, 4, exact=True)
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, noise=True) as r:
        # nothing rendered, then one batch: every pixel unknown
        for passes, n in ((0, 0), (4, 1), (3, 1)):
            r.render(passes)
            out = r.noise()
            assert (out["batches"] == n).all() and (out["stderr"] == -1).all() and (out["relative"] == -1).all()
            assert (out["unknown"], out["known"], out["quantile_value"]) == (W * H, 0, -1.0)
            assert out["hist"][BINS] == W * H and out["hist"][:BINS].sum() == 0
        assert np.array_equal(u32(out["mean"]), u32(restate_evaluation(restate_moments(frames[:1]))[0].astype(F32)))
        r.render(9)
        assert same_records(r.noise_moments(), restate_moments(frames))
        # reset clears the records and the baseline
        r.reset()
        zero = r.noise_moments()
        assert not zero["n"].any() and not zero["bad"].any() and not zero["s1"].any() and not zero["s2"].any()
        r.render(16)
        assert same_records(r.noise_moments(), restate_moments(frames))
        # set_pass_count(6) and ten passes: batch 2 is not this session's; batches 3 and 4 count, from the buffer at pass 8
        r.reset()
        r.render(6).wait()
        r.set_pass_count(6)
        assert not r.noise_moments()["n"].any()
        got = r.render(10).noise_moments()
        with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True) as t:
            t.render(6).wait()
            t.set_pass_count(6)
            at = [t.render(k).radiance().copy() for k in (2, 4, 4)]
        assert (got["n"] == 2).all() and same_records(got, restate_moments(at[1:], base=at[0]))
        # set_pass_count to a multiple of four: the baseline is the buffer in front of the next launch
        r.set_pass_count(16)
        before = r.radiance().copy()
        got = r.render(8).noise_moments()
        with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True) as t:
            t.render(6).wait()
            t.set_pass_count(6)
            at = [t.render(k).radiance().copy() for k in (10, 4, 4)]
        assert np.array_equal(u32(before), u32(at[0]))
        assert (got["n"] == 2).all() and same_records(got, restate_moments(at[1:], base=at[0]))


def driver(tmp_path, *extra, passes=None):
    out = str(tmp_path / "o.png")
    cmd = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--spp", "4", "-o", out, "--json", *extra]
    if passes:
        cmd += ["--passes", str(passes)]
    p = subprocess.run(cmd + [os.path.join(ROOT, "kajo_amd", "data", "caustics.json")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_stops_on_the_rule_runs_out_for_zero_and_maps_any_number_of_owners(tmp_path):
    fixed = driver(tmp_path, "--noise-map", str(tmp_path / "a.pfm"), passes=32)
    assert fixed["passes"] == 32 and fixed["noise_stopped_at_pass"] == 0 and fixed["noise_known_px"] == 96 * 54
    E = fixed["noise_quantile_value"]
    assert E > 0
    # the quantile a fixed run of 32 passes reports is met after 32 passes at the latest (--batch 4: the rule is looked at every batch)
    stop = driver(tmp_path, "--until-noise", repr(E), "--max-passes", "64", "--batch", "4")
    assert stop["passes"] % 4 == 0 and 8 <= stop["passes"] <= 32 and stop["noise_stopped_at_pass"] == stop["passes"]
    assert stop["noise_quantile_value"] <= E and stop["noise_known_px"] == 96 * 54
    # ... with the driver's own batches: a multiple of four below 64
    auto = driver(tmp_path, "--until-noise", repr(E), "--max-passes", "64")
    assert auto["passes"] % 4 == 0 and auto["passes"] < 64 and auto["noise_stopped_at_pass"] == auto["passes"] and auto["noise_quantile_value"] <= E
    never = driver(tmp_path, "--until-noise", "0", "--max-passes", "64")
    assert never["passes"] == 64 and never["noise_stopped_at_pass"] == 0 and never["noise_quantile_value"] > 0
    three = driver(tmp_path, "--noise-map", str(tmp_path / "b.pfm"), "--gpus", "3", "--same-device", passes=32)
    a, b = read_pfm(str(tmp_path / "a.pfm")), read_pfm(str(tmp_path / "b.pfm"))
    assert a.shape == (54, 96, 3) and np.array_equal(u32(a), u32(b)) and (a[..., 2] >= 0).all()
    assert three["noise_quantile_value"] == E and three["noise_known_px"] == 96 * 54
