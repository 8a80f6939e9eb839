"""First-hit AOVs (KAJO_FLAG_AOV; include/kajo_hip.h kajo_hip_read_aov; kajo_amd/csrc/aov.inc.hip) on the GPU.

The definition is replayed sample by sample against the oracle: every camera ray of the frame from oraclelib.camera_ray (the same
stream key and jitter as Renderer.cpp:51-64), its closest hit from the oracle's trace, and the two float4 sums built in numpy by a
sequential float32 loop in the defined order -- pass order, then stratum sy * n + sx (np.sum would add pairwise: not that order).
The STRICT and EXACT handles' buffers must be those sums bit for bit; the FAST handles' within a measured bound of them."""
import os
import subprocess

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import Scene, stress_scene
from oraclelib import OracleLib, available, camera_ray

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not available("oracle"), reason="oracle not built")]
SEED = 0o715517
W, H, S, P = 48, 32, 32, 3  # n = 5: 25 strata per pass
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
_REPLAYS = {}


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


def replay(sc, passes, w=W, h=H, spp=S, seed=SEED):
    """(A, B) of include/kajo_hip.h for the passes numbered `passes`, from the oracle, one sample at a time in the defined order."""
    key = (sc.name, sc.n_spheres, sc.n_planes, tuple(passes), w, h, spp, seed)
    if key in _REPLAYS:
        return _REPLAYS[key]
    o = OracleLib("oracle").create(sc, 1)
    n = int(np.sqrt(float(spp)))
    mats = np.concatenate([sc.planes[:, 16:38], sc.spheres[:, 16:38]]).astype(np.float32)  # by object id - 1: planes first
    diffuse, specular, transparency = mats[:, 4:7], mats[:, 8:11], mats[:, 16:19]
    lobes = np.minimum(np.maximum((diffuse + specular) + transparency, np.float32(0)), np.float32(1))
    bg = sc.background[:3].astype(np.float32)
    A = np.zeros((h * w, 4), np.float32)
    B = np.zeros((h * w, 4), np.float32)
    for p in passes:
        for s in range(n * n):
            O = np.empty((h * w, 3), np.float32)
            D = np.empty((h * w, 3), np.float32)
            for y in range(h):
                for x in range(w):
                    O[y * w + x], D[y * w + x], _ = camera_ray(o, w, h, spp, x, y, s, npass=p, seed=seed)
            t = o.trace(O, D)
            hit = t["idx"] != 0
            albedo = np.where(hit[:, None], lobes[np.maximum(t["idx"], 1) - 1], bg[None, :]).astype(np.float32)
            normal = np.where(hit[:, None], t["normal"], np.float32(0)).astype(np.float32)
            depth = np.where(hit, t["t"], np.float32(0)).astype(np.float32)
            # one float32 addition per word and sample (a miss adds zeros), in pass and stratum order
            A[:, :3] += albedo
            A[:, 3] += hit.astype(np.float32)
            B[:, :3] += normal
            B[:, 3] += depth
    out = (A.reshape(h, w, 4), B.reshape(h, w, 4))
    _REPLAYS[key] = out
    return out


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


def read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4")
    c = 3 if kind == b"PF" else 1
    assert kind in (b"PF", b"Pf") and data.size == w * h * c
    return data.reshape(h, w, c)[::-1]  # (rows are stored bottom to top)


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
