"""Which of the EXACT build's two one-light small-scene kernels a scene runs. Nothing observable says which kernel a handle launched, so the
condition kajo_amd/csrc/launch.inc.hip reads -- coldInLds && nLights == 1, then allTranslated && planesRigid: kajo_render_exact_simple, else
kajo_render_exact -- is pinned here from the host's own staging (tools/host_san.cpp `plan sizes` and `plan lds` over kajo_amd/csrc/stage.cpp
and launch_plan.h), for every one-light scene of tests/golden/scenes.npz and every builder of tests/one_light_scenes.py. If stage.cpp's rule
or a builder moves, the GPU modules that render these scenes (tests/test_hip_simple_instance.py, tests/test_hip_one_light_general.py) fail
here by the scene's name instead of quietly covering one kernel twice.

The golden set's one-light scenes are spheres_a1 / _a43 / _a169 and test_a1, all (allTranslated, planesRigid, nLights) = (1, 1, 1): the simple
kernel; and dialect_a1, whose first two spheres carry a rotation and a non-uniform scale: (0, 1, 1), the general kernel already."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from kajo_amd.scene import Scene, material, plane_record, sphere_record, translate
from one_light_scenes import GRID_THRESHOLD, both_twin, general_ids, general_scene, scaled_plane_twin, turned_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMPLE_GOLDEN = ("spheres_a1", "spheres_a43", "spheres_a169", "test_a1")
GENERAL_SEEDS = (2, 4)  # tests/test_hip_one_light_general.py's


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(scene) -> the fields of `plan sizes` and, under "exact", of `plan lds`'s line for the EXACT build without flags. A plain build of
    the tool: the sanitised one runs in tests/test_sanitize_cpu.py."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("routing")
    exe = str(d / "host_plan")
    src = [os.path.join(ROOT, "tools", "host_san.cpp"), os.path.join(ROOT, "kajo_amd", "csrc", "stage.cpp"),
           os.path.join(ROOT, "kajo_amd", "host", "scene", "SceneLoader.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "kajo_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "kajo_amd", "host"), *src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def fields(line):
        return {k: int(v) for k, v in (kv.split("=") for kv in line.split(": ", 1)[1].split())}

    def run(sc):
        pod = str(d / "scene.pod")
        sc.write_pod(pod)
        got = fields(subprocess.run([exe, "plan", "sizes", pod], capture_output=True, text=True, check=True).stdout)
        lds = subprocess.run([exe, "plan", "lds", pod], capture_output=True, text=True, check=True).stdout.splitlines()
        got["exact"] = fields([l for l in lds if l.split(": ", 1)[0].endswith(" plain exact")][0])
        got["exact no_grid"] = q = fields([l for l in lds if l.split(": ", 1)[0].endswith(" no_grid exact")][0])  # as KAJO_FLAG_NO_GRID stages
        # (launch_plan.h ldsTotal() restated, as tests/test_scene_sizes_cpu.py does)
        q["ldsTotal"] = ((q["ldsBytes"] + 15) & ~15) + q["wavesPerBlock"] * (q["helpBytes"] + q["accBytes"] + 64 * 16 * q["stealWindow"])
        return got

    return run


def triple(p):
    return p["allTranslated"], p["planesRigid"], p["nLights"]


def kernel_of(p):
    """launch.inc.hip's choice for an EXACT handle without KAJO_FLAG_NO_ONE_LIGHT, restated over the plan's fields"""
    assert p["exact"]["coldInLds"] == 1
    if p["nLights"] != 1:
        return "kajo_render_exact_lights"
    return "kajo_render_exact_simple" if p["allTranslated"] and p["planesRigid"] else "kajo_render_exact"


def test_the_golden_one_light_scenes(plan, scenes):
    one_light = sorted(k for k, s in scenes.items() if s.n_lights == 1)
    assert one_light == sorted(SIMPLE_GOLDEN + ("dialect_a1",))
    for k in SIMPLE_GOLDEN:
        p = plan(scenes[k])
        assert triple(p) == (1, 1, 1) and kernel_of(p) == "kajo_render_exact_simple", (k, p)
    p = plan(scenes["dialect_a1"])
    assert triple(p) == (0, 1, 1) and kernel_of(p) == "kajo_render_exact", p


@pytest.mark.parametrize("name", SIMPLE_GOLDEN)
def test_the_twins_of_every_simple_golden_scene(plan, scenes, name):
    base = scenes[name]
    b = plan(base)
    assert b["roomClosed"] == 1 and b["grid"] == 0
    for build, want in ((turned_twin, (0, 1, 1)), (scaled_plane_twin, (1, 0, 1)), (both_twin, (0, 0, 1))):
        sc, ids = build(base)
        p = plan(sc)
        assert sc.n_lights == 1 and sc.n_spheres < GRID_THRESHOLD
        assert triple(p) == want and kernel_of(p) == "kajo_render_exact", (sc.name, p)
        # the room and the grid decision are the base's, the whole scene is staged in LDS
        assert (p["roomClosed"], p["grid"], p["lists"]) == (b["roomClosed"], b["grid"], b["lists"]), (sc.name, p)
        # the id map: every old object keeps its record, the last sphere is still the last
        assert ids.size == 1 + base.n_planes + base.n_spheres and ids[0] == 0 and len(set(ids.tolist())) == ids.size
        for old in range(1, ids.size):
            new = int(ids[old])
            if old <= base.n_planes:
                assert np.array_equal(sc.planes[new - 1], base.planes[old - 1])
            else:
                assert np.array_equal(sc.spheres[new - 1 - sc.n_planes], base.spheres[old - 1 - base.n_planes])
        assert ids[-1] == sc.n_planes + sc.n_spheres


@pytest.mark.parametrize("seed", GENERAL_SEEDS)
def test_general_scenes(plan, scenes, seed):
    base = scenes["spheres_a169"]
    for planes, want in (("rigid", (0, 1, 1)), ("scaled", (0, 0, 1))):
        sc = general_scene(base, seed, planes)
        p = plan(sc)
        assert sc.n_lights == 1 and 9 <= sc.n_spheres <= 21 and general_ids(sc) == (7, 7 + sc.n_spheres)
        assert triple(p) == want and kernel_of(p) == "kajo_render_exact", (sc.name, p)
        assert p["roomClosed"] == 1 and p["grid"] == 0
        m = sc.spheres[:, 16:38]
        light = (m[:, 12:16] != 0).any(1)
        assert light.sum() == 1 and light[-1]
        glass, diffuse, spec, mirror = (m[:, 16:19] != 0).any(1), (m[:, 4:7] != 0).any(1), (m[:, 8:11] != 0).any(1), m[:, 20] == 0
        # the five classes of scenes_extra.mixed_scene: diffuse, Phong, ideal reflector, glass, diffuse + Phong
        for k, has in enumerate((diffuse & ~spec, spec & ~diffuse & ~glass & ~mirror, spec & mirror & ~light, glass, diffuse & spec)):
            assert has.any(), (sc.name, k)
        # every sphere carries a rotation
        assert not any(np.array_equal(r[:16].reshape(4, 4).T[:3, :3], np.eye(3, dtype=np.float32)) for r in sc.spheres)
    rigid, scaled = general_scene(base, seed, "rigid"), general_scene(base, seed, "scaled")
    assert np.array_equal(rigid.spheres, scaled.spheres)
    det = lambda r: float(np.linalg.det(r[:16].reshape(4, 4).astype(np.float64)))
    ratios = [det(b) / det(a) for a, b in zip(rigid.planes, scaled.planes)]
    assert sorted(set(np.round(ratios, 9))) == [0.125, 8.0], ratios  # (the room's own determinants are 1 to within 3e-7) both occur
    # ... of the same planes: row y of the inverse, which is all the walk reads of a plane beside the determinant, is the rigid scene's
    for a, b in zip(rigid.planes, scaled.planes):
        ra = np.linalg.inv(a[:16].reshape(4, 4).T.astype(np.float64))[1]
        rb = np.linalg.inv(b[:16].reshape(4, 4).T.astype(np.float64))[1]
        assert np.allclose(ra, rb, rtol=0, atol=1e-12)


def with_plane_determinant(base, z_scale):
    """`base` with one more plane far behind its first one: a pure translation with its z axis scaled, whose binary32 determinant (stage.cpp
    determinant: products with exact zeros and ones) is z_scale exactly"""
    M = np.eye(4, dtype=np.float32)
    M[1, 3] = 60.0
    M[2, 2] = np.float32(z_scale)
    assert base.planes[0, 13] == 1.0  # (spheres_a169's floor: y = 1 in a y-down world; the new plane lies under it)
    return Scene(base.background, base.view, base.proj, base.spheres, np.concatenate([base.planes, plane_record(M.T.reshape(16), material(diffuse=[.5] * 3))[None]]))


def test_the_boundary_of_the_rigid_plane_rule(plan, scenes):
    """stage.cpp stageScene: planesRigid = 0 unless |det - 1| <= 2^-20 for every plane. 1 + 2^-20 and 1 - 2^-20 are binary32 numbers and their
    differences from 1 are exact: rigid. One binary32 step farther from 1 on either side (2^-23 above 1, 2^-24 below) is not."""
    base = scenes["spheres_a169"]
    one, e = np.float32(1), np.float32(2.0 ** -20)
    up, down = one + e, one - e
    assert float(up) - 1 == 2.0 ** -20 and 1 - float(down) == 2.0 ** -20
    for z, rigid in ((up, 1), (down, 1), (np.nextafter(up, np.float32(2)), 0), (np.nextafter(down, np.float32(0)), 0), (one, 1)):
        p = plan(with_plane_determinant(base, z))
        assert triple(p) == (1, rigid, 1), (float(z), p)


def test_a_translated_sphere_is_general_only_by_its_matrix(plan, scenes):
    """stage.cpp: translated = isPureTranslation(M) && det == 1 && isPureTranslation(inverse). The issue's case "a pure translation whose
    determinant is not exactly 1" has no binary32 instance with finite entries and is left out: with columns 0-2 and element (3, 3) exactly
    those of the identity, every product of stage.cpp's cofactor expansion is x * 0 or x * 1, exact, and the sums are 1 + 0 or 0 + 0: the
    determinant is 1 and the inverse translate(-c) for ANY finite translation (only an infinite one makes inf * 0 = NaN, and kajo_hip_create
    refuses non-finite coordinates: stage.h coordinateRange). What is pinned instead is the rule's other side: translations at the extremes
    of binary32 stay (centre, radius) records, and the smallest departure from the identity in the 3 x 3 part makes a general one."""
    base = scenes["spheres_a169"]

    def with_sphere(M16):
        rec = sphere_record(M16, material(diffuse=[.5] * 3), 0.25)
        n = base.n_spheres
        return Scene(base.background, base.view, base.proj, np.concatenate([base.spheres[:n - 1], rec[None], base.spheres[n - 1:]]), base.planes)

    for c in ((1e-30, 3e4, -7.25), (0.1, 0.2, 0.3), (-16777217.0, 1e-38, 5e3)):
        assert triple(plan(with_sphere(translate(*c)))) == (1, 1, 1), c
    M = translate(0.0, 40.0, 0.0)
    M[0] = np.nextafter(np.float32(1), np.float32(2))  # element (0, 0): one step above 1
    assert triple(plan(with_sphere(M))) == (0, 1, 1)
    M = translate(0.0, 40.0, 0.0)
    M[1] = np.float32(2.0 ** -100)  # element (column 0, row 1): a shear far below the rounding of any product; the determinant is still 1
    assert triple(plan(with_sphere(M))) == (0, 1, 1)


def test_the_small_scene_that_reaches_the_lds_opt_in(plan, scenes):
    """capi.cpp kajo_hip_create calls setLds above 48 KiB, and for a scene staged whole in LDS launch.inc.hip's _set_lds passes the bytes on to
    kajo_render_exact_simple_set_lds. Under 48 spheres nothing comes near (46 + 1 light: 25 888 bytes); with KAJO_FLAG_NO_GRID a scene stays
    a small one while its records are within 40 KiB (launch_plan.h: big), and lds_opt_in_scene's 200 spheres + 1 light plan 52 992 bytes:
    tests/test_hip_simple_instance.py renders it. No small scene can pass the 64 KiB default limit of dynamic LDS itself: 40 KiB of records,
    the planes and the camera beside them and four waves' 4 KiB areas end below 59 KiB -- one more sphere than fits makes a large scene."""
    from one_light_scenes import lds_opt_in_scene
    sc = lds_opt_in_scene(scenes["spheres_a169"])
    p = plan(sc)
    q = p["exact no_grid"]
    assert triple(p) == (1, 1, 1) and q["coldInLds"] == 1 and q["wavesPerBlock"] == 4, (p, q)
    assert 48 * 1024 < q["ldsTotal"] <= 64 * 1024, q["ldsTotal"]
    assert p["exact"]["coldInLds"] == 0  # (without the flag it is a large scene: the grid)
    t = plan(turned_twin(sc)[0])
    assert triple(t) == (0, 1, 1) and t["exact no_grid"]["coldInLds"] == 1 and t["exact no_grid"]["ldsTotal"] > 48 * 1024
    # the largest small scene of this recipe: one sphere more than the last that is still staged whole is not
    from scenes_extra import dense_scene
    n = 200
    while plan(dense_scene(scenes["spheres_a169"], n + 8, 1, seed=1))["exact no_grid"]["coldInLds"]:
        n += 8
    top = plan(dense_scene(scenes["spheres_a169"], n, 1, seed=1))["exact no_grid"]
    print("largest ldsTotal of a small scene found: %d bytes at %d spheres + 1 light" % (top["ldsTotal"], n))
    assert top["coldInLds"] == 1 and top["ldsTotal"] < 64 * 1024
