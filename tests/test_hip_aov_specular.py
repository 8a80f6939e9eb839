"""AOVs at the first non-delta hit (KAJO_FLAG_AOV_SPECULAR; include/kajo_hip.h under kajo_hip_read_aov; aovFollow in
kajo_amd/csrc/aov.inc.hip) on the GPU.

The definition is replayed one sample at a time in numpy from the oracle's camera rays, closest hits and delta-lobe directions
(tests/aov_specular_replay.py; pinned against the first-hit replay by tests/test_aov_specular_cpu.py). The STRICT and EXACT handles'
buffers must be that replay's sums bit for bit; the FAST handles' within a measured bound of the STRICT buffers."""
import os
import subprocess

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import stress_scene
from oraclelib import available

from aov_specular_replay import describe, replay_specular, with_delta_balls, without_delta
from framelib import read_pfm
from test_hip_aov import crowded_scene, open_floor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not available("oracle"), reason="oracle not built")]
SEED = 0o715517
W, H, S, P = 48, 32, 32, 3  # n = 5: 25 strata per pass
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
BUILDS = [dict(exact=True), dict(strict=True), dict()]
_REPLAYS = {}


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def replay(sc, passes, w=W, h=H, spp=S):
    key = (sc.name, sc.n_spheres, sc.n_planes, tuple(passes), w, h, spp)
    if key not in _REPLAYS:
        _REPLAYS[key] = replay_specular(sc, passes, w, h, spp, SEED)
    return _REPLAYS[key]


def _scenes(scenes):
    """name -> (scene, flags, kernel instance). The grid scenes are tests/test_hip_aov.py's with every fifth or seventh ball turned into glass
    or an ideal mirror (their room keeps spheres.json's mirror wall), so every one of the five instances follows chains."""
    base = scenes["spheres_a169"]
    grid60, grid1000, grid2000 = (with_delta_balls(stress_scene(base, 60, 4), 5), with_delta_balls(stress_scene(base, 1000, 16)),
                                  with_delta_balls(crowded_scene(base)))
    return {
        "spheres_a169": (base, 0, "kajo_aov_{}_spec"),
        "caustics_a169": (scenes["caustics_a169"], 0, "kajo_aov_{}_spec"),
        "test_a1": (scenes["test_a1"], 0, "kajo_aov_{}_spec"),
        "open_floor": (open_floor(base), 0, "kajo_aov_{}_spec"),
        "grid_lds": (grid60, 0, "kajo_aov_{}_spec_biglist_lg"),
        "grid_lds_nolists": (grid60, capi.KAJO_FLAG_NO_SHADOW_LISTS, "kajo_aov_{}_spec_big_lg"),
        "stress1000": (grid1000, 0, "kajo_aov_{}_spec_biglist_lg"),
        "stress1000_nolists": (grid1000, capi.KAJO_FLAG_NO_SHADOW_LISTS, "kajo_aov_{}_spec_big_lg"),
        "grid_global": (grid2000, 0, "kajo_aov_{}_spec_biglist"),
        "grid_global_nolists": (grid2000, capi.KAJO_FLAG_NO_SHADOW_LISTS, "kajo_aov_{}_spec_big"),
    }


NAMES = ["spheres_a169", "caustics_a169", "test_a1", "open_floor", "grid_lds", "grid_lds_nolists", "stress1000", "stress1000_nolists",
         "grid_global", "grid_global_nolists"]


@pytest.mark.parametrize("name", NAMES)
def test_equal_the_replay_strict_and_exact(scenes, name):
    sc, flags, kernel = _scenes(scenes)[name]
    A, B, stats = replay(sc, range(1, P + 1))
    print(name, describe(stats))
    if name != "test_a1":  # (the built-in test scene has no delta material: there the flag must change nothing, and the replay says so)
        assert stats["followed"] > 0
    if name.startswith(("grid_", "stress")):  # chains off the balls too, not only off the room's mirror wall
        assert stats["longest"] >= 2
    for kw in (dict(strict=True), dict(exact=True)):
        with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, aov_specular=True, flags=flags, **kw) as r:
            assert r.aov_kernel() == kernel.format("strict"), (name, kw, r.aov_kernel())
            got = r.render(P).aov()
        assert got["samples"] == 25 * P
        for k, want in enumerate((A, B)):
            assert bits_equal(got["raw"][k], want), (name, kw, k, np.argwhere(got["raw"][k] != want)[:4])
    if name == "open_floor":  # chains that end in a miss take T * background
        assert (A[..., 3] < 25 * P).any() and (A[..., 3] > 0).any()


RAGGED = [(1, 1), (7, 5), (41, 23), (65, 9)]
RAGGED_S, RAGGED_P = 16, 2


@pytest.mark.parametrize("name", ["spheres_a169", "grid_lds"])
def test_ragged_frames(scenes, name):
    sc, flags, kernel = _scenes(scenes)[name]
    followed = 0
    for w, h in RAGGED:
        A, B, stats = replay(sc, range(1, RAGGED_P + 1), w, h, RAGGED_S)
        followed += stats["followed"]
        for kw in (dict(strict=True), dict(exact=True)):
            with HipRenderer(sc, w, h, spp=RAGGED_S, seed=SEED, aov=True, aov_specular=True, flags=flags, **kw) as r:
                assert r.aov_kernel() == kernel.format("strict")
                got = r.render(RAGGED_P).aov()
            assert got["samples"] == 16 * RAGGED_P
            for k, want in enumerate((A, B)):
                assert bits_equal(got["raw"][k], want), (name, (w, h), kw, k, np.argwhere(got["raw"][k] != want)[:4])
    assert followed > 0


@pytest.mark.parametrize("build", BUILDS)
def test_cut_invariance(scenes, build):
    """render(1); render(2), render(3), and launches of 1 or 3 passes: one pair of buffers, bit for bit."""
    for name in ("spheres_a169", "grid_lds"):
        sc, flags, _ = _scenes(scenes)[name]
        got = []
        for ppl, cuts in ((0, (1, 2)), (0, (3,)), (1, (3,)), (3, (3,))):
            with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, aov_specular=True, passes_per_launch=ppl, flags=flags, **build) as r:
                for c in cuts:
                    r.render(c)
                got.append(r.aov())
        for g in got[1:]:
            assert g["samples"] == got[0]["samples"] == 75
            assert bits_equal(g["raw"][0], got[0]["raw"][0]) and bits_equal(g["raw"][1], got[0]["raw"][1]), (name, build)


@pytest.mark.parametrize("build", BUILDS)
def test_without_delta_materials_the_flag_changes_nothing(scenes, build):
    base = scenes["spheres_a169"]
    for sc in (scenes["test_a1"], without_delta(base), without_delta(stress_scene(base, 60, 4))):
        raws = []
        for spec in (False, True):
            with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, aov_specular=spec, **build) as r:
                assert ("_spec" in r.aov_kernel()) == spec
                raws.append(r.render(P).aov()["raw"])
        assert raws[0][0].any()
        assert bits_equal(raws[0][0], raws[1][0]) and bits_equal(raws[0][1], raws[1][1]), (sc.name, build)


@pytest.mark.parametrize("build", BUILDS)
def test_beauty_unchanged_by_the_flag(scenes, build):
    for name in ("spheres_a169", "stress1000"):
        sc, flags, _ = _scenes(scenes)[name]
        with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, flags=flags, **build) as a, \
                HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, aov_specular=True, flags=flags, **build) as b:
            ra = a.render(3).radiance()
            rb = b.render(3).radiance()
            ca, cb = a.counters(), b.counters()
        assert bits_equal(ra, rb), (name, build)
        assert ca["launches"] == cb["launches"] and ca["passes"] == cb["passes"]


# FAST against STRICT on the same frame, by tests/test_hip_aov.py's rule: the share of pixels whose every channel of the means (albedo,
# normal, depth, hit count) is within 1e-4 relative (floor 1). A chain passes FAST's rounding through up to nine walks and a hit flipped
# behind a mirror moves a whole sample, so the shares are lower than the first-hit ones. The bound is the share MEASURED on one MI355X
# at 48 x 32 x 32 spp x 3 passes less 0.03 (the first-hit test's margin, for the same reason: a handful of grazing rays). Measured:
# spheres_a169 0.99544 (7 pixels of 1536 outside: all by the normal, 6 by the depth, 1 by the albedo, none by the hit count),
# caustics_a169 0.99479 (8), 60 spheres 0.98177 (28: 27 by the normal), 1000 spheres 0.80859 (294: 292 by the normal, 76 by the depth,
# 36 by the albedo), 2000 spheres 0.75846 (371: 368 / 85 / 44). The first-hit shares of the same scenes without edited balls are 1.0,
# 1.0, 0.984, 0.915, 0.906: the small balls' normals (radius 0.1, FAST's cancelling discriminant) are now also seen in the mirror wall
# and through the glass balls, and a reflected ray that starts on such a normal carries its error on.
FAST_MEASURED = {"spheres_a169": 0.99544, "caustics_a169": 0.99479, "grid_lds": 0.98177, "stress1000": 0.80859, "grid_global": 0.75846}


def _means(a):
    return np.concatenate([a["albedo"], a["normal"], a["depth"][..., None], a["hits"][..., None]], -1)


def test_fast_close_to_strict(scenes):
    failures = []
    for name, measured in FAST_MEASURED.items():
        sc, flags, _ = _scenes(scenes)[name]
        means = []
        for kw in (dict(strict=True), dict()):
            with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, aov_specular=True, flags=flags, **kw) as r:
                means.append(_means(r.render(P).aov()))
        s, f = means
        close = np.abs(f - s) <= 1e-4 * np.maximum(np.abs(s), 1.0)
        ok = close.all(-1)
        print("FAST vs STRICT AOVs (first non-delta hit), %s: %.5f of pixels within 1e-4 (%d of %d outside); outside by albedo %d, normal %d, "
              "depth %d, hits %d" % (name, ok.mean(), (~ok).sum(), ok.size, (~close[..., 0:3].all(-1)).sum(), (~close[..., 3:6].all(-1)).sum(),
                                     (~close[..., 6]).sum(), (~close[..., 7]).sum()))
        if measured is None or ok.mean() < measured - 0.03:
            failures.append((name, ok.mean(), measured))
    assert not failures, failures


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_writes_the_means_and_a_denoised_image(scenes, tmp_path):
    sc = scenes["spheres_a169"]
    pod = str(tmp_path / "scene.pod")
    sc.write_pod(pod)
    prefix = str(tmp_path / "frame")
    common = [BIN, "-w", str(W), "-h", str(H), "--passes", "3", "--spp", str(S), "--gpus", "1", "-o", "", "--scene-pod", pod]
    p = subprocess.run(common + ["--strict", "--aov", prefix, "--aov-specular"], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    with HipRenderer(sc, W, H, spp=S, seed=SEED, strict=True, aov=True, aov_specular=True) as r:
        want = r.render(3).aov()
    with HipRenderer(sc, W, H, spp=S, seed=SEED, strict=True, aov=True) as r:
        first = r.render(3).aov()
    assert not bits_equal(want["depth"], first["depth"])  # (the flag reached the handle)
    albedo, normal, depth = (read_pfm("%s_%s.pfm" % (prefix, k)) for k in ("albedo", "normal", "depth"))
    assert bits_equal(albedo, want["albedo"]) and bits_equal(normal, want["normal"]) and bits_equal(depth[..., 0], want["depth"])
    png = str(tmp_path / "denoised.png")
    p = subprocess.run(common + ["--denoise", png, "--aov-specular"], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(png) > 100 and open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"


def _rmse(img, ref, mask):
    return float(np.sqrt(np.mean((np.clip(img, 0, 1) - np.clip(ref, 0, 1))[mask] ** 2)))


def test_denoise_quality_with_the_new_guides(scenes):
    """tests/test_hip_denoise.py::test_quality_against_a_converged_frame's setup (EXACT, spheres.json 16:9 at 320x180, truth = 64 spp x 40
    passes seed 12345, noisy = 4 spp x 1 pass, the denoiser's defaults), with first-hit guides and with the guides of the first non-delta
    hit in the same run. M = the pixels whose mean depth differs between the two kinds of guides by more than 1e-3 relative: the pixels
    that see a chain. Measured on one MI355X: M = 30.6 % of the frame; blur over M 0.0401 with first-hit guides, 0.0381 with the new ones;
    denoised 4-spp frame over M 0.0937 -> 0.0887 (raw 0.2041); whole frame raw 0.2727, denoised 0.0880 -> 0.0868 (ratio 0.318), the
    reference moved by 0.0391 -> 0.0389 (0.143 x raw)."""
    sc = scenes["spheres_a169"]
    w, h = 320, 180
    out = {}
    for spec in (False, True):
        with HipRenderer(sc, w, h, spp=64, exact=True, aov=True, aov_specular=spec, seed=12345) as ref:
            ref.render(40)
            truth = ref.radiance()[..., :3] / ref.passes
            ref_dn = ref.denoise()["radiance"][..., :3] / ref.passes
            depth = ref.aov()["depth"]
        with HipRenderer(sc, w, h, spp=4, exact=True, aov=True, aov_specular=spec) as r:
            r.render(1)
            raw = r.radiance()[..., :3] / r.passes
            dn = r.denoise()["radiance"][..., :3] / r.passes
        out[spec] = dict(truth=truth, ref_dn=ref_dn, depth=depth, raw=raw, dn=dn)
    a, b = out[False], out[True]
    assert bits_equal(a["truth"], b["truth"]) and bits_equal(a["raw"], b["raw"])  # (the beauty frames do not depend on the flag)
    truth, raw = b["truth"], b["raw"]
    finite = np.isfinite(truth).all(-1) & np.isfinite(raw).all(-1)
    M = (np.abs(b["depth"] - a["depth"]) > 1e-3 * np.maximum(np.abs(a["depth"]), 1e-30)) & finite
    print("M: %.1f %% of the frame" % (100.0 * M.mean()))
    assert M.mean() >= 0.20, M.mean()
    assert np.isfinite(b["dn"]).all() and np.isfinite(b["ref_dn"][np.isfinite(truth).all(-1)]).all()
    e_raw, e_dn, e_ref = _rmse(raw, truth, finite), _rmse(b["dn"], truth, finite), _rmse(b["ref_dn"], truth, finite)
    e_dn0, e_ref0 = _rmse(a["dn"], truth, finite), _rmse(a["ref_dn"], truth, finite)
    blur0, blur1 = _rmse(a["ref_dn"], truth, M), _rmse(b["ref_dn"], truth, M)
    noisy0, noisy1, raw_m = _rmse(a["dn"], truth, M), _rmse(b["dn"], truth, M), _rmse(raw, truth, M)
    print("whole frame: raw %.4f; denoised first-hit %.4f, new %.4f (ratio %.3f); reference moved by first-hit %.4f, new %.4f (%.3f x raw)" %
          (e_raw, e_dn0, e_dn, e_dn / e_raw, e_ref0, e_ref, e_ref / e_raw))
    print("over M: raw %.4f; blur (denoised truth against truth) first-hit %.4f, new %.4f; denoised noisy frame first-hit %.4f, new %.4f" %
          (raw_m, blur0, blur1, noisy0, noisy1))
    assert blur1 < blur0, (blur0, blur1)
    assert e_dn <= 0.5 * e_raw, (e_raw, e_dn)
    assert e_ref <= 0.25 * e_raw, (e_raw, e_ref)
    assert noisy1 <= 1.05 * noisy0, (noisy0, noisy1)
