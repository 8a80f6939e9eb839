"""First-hit AOVs (KAJO_FLAG_AOV; include/kajo_hip.h kajo_hip_read_aov; kajo_amd/csrc/aov.inc.hip) on the GPU.

The definition is replayed sample by sample by the oracle (koracle_aov): every camera ray of the frame (the same stream key and jitter
as Renderer.cpp:51-64), its closest hit from the oracle's trace, and the two float4 sums built by a sequential float32 loop in the
defined order -- pass order, then stratum sy * n + sx. tests/test_aov_oracle_cpu.py pins that replay to a numpy one, one ray at a time.
The STRICT and EXACT handles' buffers must be those sums bit for bit; the FAST handles' within a measured bound of them."""
import os
import subprocess

import numpy as np
import pytest

from framelib import read_pfm
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import Scene, stress_scene
from oraclelib import OracleLib, available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not available("oracle"), reason="oracle not built")]
SEED = 0o715517
W, H, S, P = 48, 32, 32, 3  # n = 5: 25 strata per pass
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
_REPLAYS = {}
THREADS = max(1, min(16, os.cpu_count() or 1))


def open_floor(base):
    """spheres.json's spheres over its floor alone: rays above the horizon miss everything and take the background."""
    return Scene(base.background, base.view, base.proj, base.spheres, base.planes[[0]], "open_floor")


def crowded_scene(base):
    """Two thousand spheres: the stress scene's thousand (and its 16 lights) and a second thousand from another seed. The hot records
    and the grid's cell lists no longer fit what the grid may take of LDS (capi.cpp: 40 KiB), so the cell lists stay in global memory
    -- the home the 1000-sphere scene does not reach (its cell lists fit LDS)."""
    a = stress_scene(base, 1000, 16)
    b = stress_scene(base, 1000, 0, seed=4321)
    return Scene(a.background, a.view, a.proj, np.concatenate([a.spheres, b.spheres]), a.planes, "crowded2000")


def replay(sc, passes, w=W, h=H, spp=S, seed=SEED, rect=None):
    """(A, B) of include/kajo_hip.h for the passes numbered `passes` (over `rect` = (x0, y0, rw, rh) of the w x h frame if given), from
    the oracle's batched replay (koracle_aov; pinned to the per-sample definition by tests/test_aov_oracle_cpu.py)."""
    key = (sc.name, sc.n_spheres, sc.n_planes, tuple(passes), w, h, spp, seed, rect)
    if key in _REPLAYS:
        return _REPLAYS[key]
    o = OracleLib("oracle").create(sc, 1)
    sums = None
    for p in passes:  # (one call per pass continues the sums: the passes need not be consecutive)
        sums = o.aov(w, h, spp, passes=1, seed=seed, first_pass=p, rect=rect, sums=sums, threads=THREADS)
    _REPLAYS[key] = sums
    return sums


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _scenes(scenes):
    base = scenes["spheres_a169"]
    return {
        "spheres_a169": (scenes["spheres_a169"], 0, "kajo_aov_{}"),
        "caustics_a169": (scenes["caustics_a169"], 0, "kajo_aov_{}"),
        "test_a1": (scenes["test_a1"], 0, "kajo_aov_{}"),
        "open_floor": (open_floor(base), 0, "kajo_aov_{}"),
        # ~60 spheres: the grid's cell lists fit LDS; a closed room of (centre, radius) spheres, so visibility lists too
        "grid_lds": (stress_scene(base, 60, 4), 0, "kajo_aov_{}_biglist_lg"),
        "grid_lds_nolists": (stress_scene(base, 60, 4), capi.KAJO_FLAG_NO_SHADOW_LISTS, "kajo_aov_{}_big_lg"),
        # the 1000-sphere stress scene (BASELINE configs[4]): hot records and cell lists fit LDS
        "stress1000": (stress_scene(base, 1000, 16), 0, "kajo_aov_{}_biglist_lg"),
        "stress1000_nolists": (stress_scene(base, 1000, 16), capi.KAJO_FLAG_NO_SHADOW_LISTS, "kajo_aov_{}_big_lg"),
        # two thousand spheres: the cell lists in global memory
        "grid_global": (crowded_scene(base), 0, "kajo_aov_{}_biglist"),
        "grid_global_nolists": (crowded_scene(base), capi.KAJO_FLAG_NO_SHADOW_LISTS, "kajo_aov_{}_big"),
    }


@pytest.mark.parametrize("name", ["spheres_a169", "caustics_a169", "test_a1", "open_floor", "grid_lds", "grid_lds_nolists", "stress1000",
                                  "stress1000_nolists", "grid_global", "grid_global_nolists"])
def test_aov_equal_the_oracle_replay_strict_and_exact(scenes, name):
    sc, flags, kernel = _scenes(scenes)[name]
    want = replay(sc, range(1, P + 1))
    for kw in (dict(strict=True), dict(exact=True)):
        with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, flags=flags, **kw) as r:
            # the instance of the scene's class (EXACT runs the STRICT one), so that the coverage of each cannot disappear silently
            assert r.aov_kernel() == kernel.format("strict"), (name, kw, r.aov_kernel())
            got = r.render(P).aov()
        assert got["samples"] == 25 * P
        for k in (0, 1):
            assert bits_equal(got["raw"][k], want[k]), (name, kw, k, np.argwhere(got["raw"][k] != want[k])[:4])
    A, B = want
    assert (A[..., 3] > 0).any()
    if name == "open_floor":  # the construction does what it is for: misses that take the background
        assert (A[..., 3] < 25 * P).any() and (A[..., 3] > 0).any()
    if name.startswith(("grid_", "stress")):
        assert (A[..., 3] == 25 * P).all()  # (a closed room: every camera ray hits something)


def test_means_follow_the_sums(scenes):
    sc = scenes["spheres_a169"]
    with HipRenderer(sc, W, H, spp=S, seed=SEED, exact=True, aov=True) as r:
        a = r.render(2).aov()
    A, B = a["raw"]
    s = np.float32(a["samples"])
    assert a["samples"] == 50
    assert bits_equal(a["albedo"], A[..., :3] / s) and bits_equal(a["normal"], B[..., :3] / s) and bits_equal(a["hits"], A[..., 3])
    hit = A[..., 3] > 0
    assert bits_equal(a["depth"][hit], B[..., 3][hit] / A[..., 3][hit]) and (a["depth"][~hit] == 0).all()
    assert np.all((a["albedo"] >= 0) & (a["albedo"] <= 1))


@pytest.mark.parametrize("build", [dict(exact=True), dict(strict=True), dict()])
def test_cut_invariance(scenes, build):
    """render(1); render(2), render(3), and launches of 1 or 3 passes: one pair of buffers, bit for bit."""
    for sc in (scenes["spheres_a169"], stress_scene(scenes["spheres_a169"], 60, 4)):
        got = []
        for ppl, cuts in ((0, (1, 2)), (0, (3,)), (1, (3,)), (3, (3,)), (1, (2, 1))):
            with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, passes_per_launch=ppl, **build) as r:
                for c in cuts:
                    r.render(c)
                got.append(r.aov())
        for g in got[1:]:
            assert g["samples"] == got[0]["samples"] == 75
            assert bits_equal(g["raw"][0], got[0]["raw"][0]) and bits_equal(g["raw"][1], got[0]["raw"][1]), (sc.name, build)


def test_set_pass_count_moves_the_streams_not_the_buffers(scenes):
    """set_pass_count(k) then P passes: the buffers hold passes k+1 .. k+P of the oracle's replay, and n^2 x P samples."""
    sc = scenes["spheres_a169"]
    k = 5
    with HipRenderer(sc, W, H, spp=S, seed=SEED, strict=True, aov=True) as r:
        r.set_pass_count(k)
        got = r.render(2).aov()
    assert got["samples"] == 50
    want = replay(sc, [k + 1, k + 2])
    assert bits_equal(got["raw"][0], want[0]) and bits_equal(got["raw"][1], want[1])
    # ... and set_pass_count after passes were summed leaves the sums alone
    with HipRenderer(sc, W, H, spp=S, seed=SEED, strict=True, aov=True) as r:
        r.render(1)
        r.set_pass_count(k)
        r.render(1)
        got = r.aov()
    want = replay(sc, [1, k + 1])
    assert got["samples"] == 50 and bits_equal(got["raw"][0], want[0]) and bits_equal(got["raw"][1], want[1])


@pytest.mark.parametrize("build", [dict(), dict(exact=True), dict(strict=True)])
def test_beauty_unchanged_by_the_flag(scenes, build):
    for sc in (scenes["spheres_a169"], stress_scene(scenes["spheres_a169"], 1000, 16)):
        with HipRenderer(sc, W, H, spp=S, seed=SEED, **build) as a, HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, **build) as b:
            ra = a.render(3).radiance()
            rb = b.render(3).radiance()
            ca, cb = a.counters(), b.counters()
        assert bits_equal(ra, rb), (sc.name, build)
        assert ca["launches"] == cb["launches"] and ca["passes"] == cb["passes"]


# FAST against STRICT on the same frame. FAST's walk and normal round differently: on small spheres seen from across the room the
# discriminant h^2 - a c cancels (|O - c| ~ 10, r ~ 0.1), so a normal (o + d t) / r carries that rounding over the radius, and a few
# grazing rays meet another sphere. Share of pixels whose every channel of the means (albedo, normal, depth, hit count) is within 1e-4
# relative (floor 1: absolute below 1), measured on MI355X at 48 x 32 x 32 spp x 3 passes: spheres_a169 1.0000, caustics_a169 1.0000
# (largest normal difference 3.3e-5), 60 spheres 0.9837 (25 pixels, all by the normal; 5.0e-3), 1000 spheres 0.9147 (131: normals;
# 16 also by albedo and depth, no hit count), 2000 spheres 0.9063 (144). The issue's estimate, 99.9 %, holds for the small scenes; the
# bounds below are the measured shares less a margin of about 0.03 for the scenes of small spheres. The decisions alone (albedo, depth,
# hit count within 1e-4): 0.9896 .. 1.0 measured, 0.98 asserted.
FAST_BOUND = {"spheres_a169": 0.999, "caustics_a169": 0.999, "grid_lds": 0.95, "stress1000": 0.88, "grid_global": 0.87}


def test_fast_close_to_strict(scenes):
    for name, bound in FAST_BOUND.items():
        sc, flags, _ = _scenes(scenes)[name]
        means = []
        for kw in (dict(strict=True), dict()):
            with HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, flags=flags, **kw) as r:
                a = r.render(P).aov()
            means.append(np.concatenate([a["albedo"], a["normal"], a["depth"][..., None], a["hits"][..., None]], -1))
        s, f = means
        close = np.abs(f - s) <= 1e-4 * np.maximum(np.abs(s), 1.0)
        ok = close.all(-1)
        decided = close[..., [0, 1, 2, 6, 7]].all(-1)
        print("FAST vs STRICT AOVs, %s: %.5f of pixels within 1e-4 (%d of %d outside); outside by albedo %d, normal %d, depth %d, hits %d; "
              "largest normal difference %.2e" % (name, ok.mean(), (~ok).sum(), ok.size, (~close[..., 0:3].all(-1)).sum(), (~close[..., 3:6].all(-1)).sum(),
                                                 (~close[..., 6]).sum(), (~close[..., 7]).sum(), np.abs(f - s)[..., 3:6].max()))
        assert ok.mean() >= bound, (name, ok.mean(), bound)
        assert decided.mean() >= 0.98, (name, decided.mean())


def test_state_and_errors(scenes):
    sc = scenes["spheres_a169"]
    with HipRenderer(sc, W, H, spp=S, seed=SEED, exact=True, aov=True) as r:
        a = r.aov()
        assert a["samples"] == 0 and not a["raw"][0].any() and not a["raw"][1].any()
        r.render(2)
        a = r.aov()
        assert a["samples"] == 50 and a["raw"][0].any()
        r.reset()
        a = r.aov()
        assert a["samples"] == 0 and not a["raw"][0].any() and not a["raw"][1].any()
        r.render(1)
        assert r.aov()["samples"] == 25
        # either pointer may be NULL
        import ctypes as C
        n = C.c_int64()
        capi.check(r._L.kajo_hip_read_aov(r._h, None, None, C.byref(n)))
        assert n.value == 25
    with HipRenderer(sc, W, H, spp=16, seed=SEED, exact=True, aov=True) as r:
        assert r.render(3).aov()["samples"] == 16 * 3
    with HipRenderer(sc, W, H, spp=S, seed=SEED, exact=True) as r:
        assert r.aov_kernel() is None
        with pytest.raises(capi.KajoError) as e:
            r.aov()
        assert e.value.code == capi.KAJO_E_STATE
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(sc, W, H, spp=S, seed=SEED, aov=True, tile_index=1, tile_count=2)
    assert e.value.code == capi.KAJO_E_INVALID


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_writes_the_means(scenes, tmp_path):
    sc = scenes["spheres_a169"]
    pod = str(tmp_path / "scene.pod")
    sc.write_pod(pod)
    prefix = str(tmp_path / "frame")
    cmd = [BIN, "-w", str(W), "-h", str(H), "--passes", "3", "--spp", str(S), "--strict", "--gpus", "1", "-o", "", "--aov", prefix,
           "--scene-pod", pod]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    with HipRenderer(sc, W, H, spp=S, seed=SEED, strict=True, aov=True) as r:
        want = r.render(3).aov()
    albedo, normal, depth = (read_pfm("%s_%s.pfm" % (prefix, k)) for k in ("albedo", "normal", "depth"))
    assert albedo.shape == (H, W, 3) and normal.shape == (H, W, 3) and depth.shape == (H, W, 1)
    assert bits_equal(albedo, want["albedo"]) and bits_equal(normal, want["normal"]) and bits_equal(depth[..., 0], want["depth"])


def _means(a):
    return np.concatenate([a["albedo"], a["normal"], a["depth"][..., None], a["hits"][..., None]], -1).reshape(-1, 8)


# 1x1 .. 65x9: frames narrower than a block, one column, one row, and ragged right and bottom blocks. 41x23 has 6 x 3 = 18 blocks: the
# last of its five workgroups holds two waves past the frame (the early return); every shape has lanes outside the frame, which trace
# nothing through the grid and still take part in the wave's votes.
RAGGED = [(1, 1), (7, 5), (1, 37), (37, 1), (41, 23), (65, 9)]
RAGGED_S, RAGGED_P = 16, 2


@pytest.mark.parametrize("name", ["spheres_a169", "grid_lds", "grid_lds_nolists", "stress1000", "stress1000_nolists", "grid_global",
                                  "grid_global_nolists"])
def test_ragged_and_degenerate_frames(scenes, name):
    """STRICT and EXACT equal the replay bit for bit at every shape; FAST within the FAST_BOUND rule over the 1638 pixels of all shapes.
    Measured on one MI355X (S = 16, 2 passes), share within 1e-4: small scene 1.0, 60 spheres 0.968, 1000 spheres 0.899, 2000 spheres
    0.910, with and without visibility lists alike; decisions 0.994 .. 1.0."""
    sc, flags, kernel = _scenes(scenes)[name]
    strict_means, fast_means = [], []
    for w, h in RAGGED:
        want = replay(sc, range(1, RAGGED_P + 1), w, h, RAGGED_S)
        for kw in (dict(strict=True), dict(exact=True), dict()):
            with HipRenderer(sc, w, h, spp=RAGGED_S, seed=SEED, aov=True, flags=flags, **kw) as r:
                assert r.aov_kernel() == kernel.format("fast" if not kw else "strict"), (name, kw, r.aov_kernel())
                got = r.render(RAGGED_P).aov()
            assert got["samples"] == 16 * RAGGED_P
            if kw:
                for k in (0, 1):
                    assert bits_equal(got["raw"][k], want[k]), (name, (w, h), kw, k, np.argwhere(got["raw"][k] != want[k])[:4])
                if "strict" in kw:
                    strict_means.append(_means(got))
            else:
                fast_means.append(_means(got))
        assert (want[0][..., 3] > 0).all() or name == "spheres_a169"
    s, f = np.concatenate(strict_means), np.concatenate(fast_means)
    close = np.abs(f - s) <= 1e-4 * np.maximum(np.abs(s), 1.0)
    ok, decided = close.all(-1), close[..., [0, 1, 2, 6, 7]].all(-1)
    print("FAST vs STRICT AOVs on the ragged frames, %s: %.5f of %d pixels within 1e-4, decisions %.5f" % (name, ok.mean(), ok.size,
                                                                                                        decided.mean()))
    assert ok.mean() >= FAST_BOUND[name.replace("_nolists", "")], (name, ok.mean())
    assert decided.mean() >= 0.98, (name, decided.mean())


@pytest.mark.parametrize("build", [dict(strict=True), dict(exact=True)])
def test_pass_numbers_across_two_to_the_sixteen_and_the_last_pass(scenes, build):
    """Passes 65535, 65536, 65537 -- the stream key's pass >> 16 word goes from 0 to 1 -- and the last renderable pass, 2^31 - 2
    (tests/test_hip_edge_cases.py test_maximum_sizes), bit for bit the replay's."""
    sc = scenes["spheres_a169"]
    for w, h in ((W, H), (41, 23)):
        with HipRenderer(sc, w, h, spp=S, seed=SEED, aov=True, **build) as r:
            r.set_pass_count(65534)
            got = r.render(3).aov()
        want = replay(sc, [65535, 65536, 65537], w, h)
        assert got["samples"] == 75 and bits_equal(got["raw"][0], want[0]) and bits_equal(got["raw"][1], want[1]), (w, h)
        with HipRenderer(sc, w, h, spp=S, seed=SEED, aov=True, **build) as r:
            r.set_pass_count(2 ** 31 - 3)
            got = r.render(1).aov()
            with pytest.raises(capi.KajoError):
                r.render(1)
        want = replay(sc, [2 ** 31 - 2], w, h)
        assert got["samples"] == 25 and bits_equal(got["raw"][0], want[0]) and bits_equal(got["raw"][1], want[1]), (w, h)


@pytest.mark.parametrize("name", ["spheres_a169", "stress1000"])
def test_full_hd_frame(scenes, name):
    """One whole 1920x1080 frame at spp = 1, STRICT and EXACT, bit for bit the replay's (the 1000-sphere replay is the slow part)."""
    sc, flags, kernel = _scenes(scenes)[name]
    w, h = 1920, 1080
    want = replay(sc, [1], w, h, 1)
    for kw in (dict(strict=True), dict(exact=True)):
        with HipRenderer(sc, w, h, spp=1, seed=SEED, aov=True, flags=flags, **kw) as r:
            assert r.aov_kernel() == kernel.format("strict")
            got = r.render(1).aov()
        assert got["samples"] == 1
        for k in (0, 1):
            assert bits_equal(got["raw"][k], want[k]), (name, kw, k, np.argwhere(got["raw"][k] != want[k])[:4])
    assert (want[0][..., 3] > 0).mean() > 0.5


def test_4k_bottom_right_corner(scenes):
    """3840x2160 (BASELINE configs[2] size), STRICT: the bottom-right 96x48 pixels -- the last blocks and workgroups -- against the replay
    of that rectangle, bit for bit."""
    sc = scenes["spheres_a169"]
    w, h, rect = 3840, 2160, (3744, 2112, 96, 48)
    want = replay(sc, [1], w, h, 4, rect=rect)
    with HipRenderer(sc, w, h, spp=4, seed=SEED, aov=True, strict=True) as r:
        got = r.render(1).aov()
    x0, y0, rw, rh = rect
    for k in (0, 1):
        g = got["raw"][k][y0:y0 + rh, x0:x0 + rw]
        assert bits_equal(g, want[k]), (k, np.argwhere(g != want[k])[:4])
    assert (want[0][..., 3] > 0).any()
