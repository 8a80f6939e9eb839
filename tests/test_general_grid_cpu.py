"""What kajo_hip_create makes of tests/general_grid_scenes.py's entries, pinned from the host's own staging and plan (tools/host_san.cpp
`plan sizes` and `plan lds` over kajo_amd/csrc/stage.cpp and launch_plan.h; kajo_amd.renderer's host-only stage_info / stage_shadow_lists):
large scenes WITH the grid, WITHOUT visibility lists, allTranslated = 0 -- the kernels `_big_lg` / `_big` with general records, which
tests/test_hip_general_grid.py renders. The rule's other side as well: one record whose determinant is an ulp off 1, and the scene gets no
grid. And a condition on the inputs: in the oracle, a quarter and more of the frame's first hits are general spheres. If stage.cpp's rule or
launch_plan.h's thresholds move, the entry that no longer covers its path fails here by name. Run with -s for the plan lines and shares."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import general_grid_scenes as G
from kajo_amd.renderer import stage_info, stage_shadow_lists
from oraclelib import OracleLib, available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ("fast", "strict", "exact")
FRAME = (72, 40)  # tests/test_hip_general_grid.py's
NAMES = list(G.ENTRIES)
_SCENES = {}


def scene_of(scenes, name, **changes):
    key = (name, tuple(sorted(changes.items())))
    if key not in _SCENES:
        _SCENES[key] = G.entry(scenes["spheres_a169"], name, **changes)
    return _SCENES[key]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(scene) -> dict: "<staging> <numerics>" -> kajoLdsPlan's fields, "sizes" -> the fields of `plan sizes`. A plain build of the
    tool, as tests/test_scene_sizes_cpu.py's: the sanitised one runs in tests/test_sanitize_cpu.py."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("general_grid")
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
        got = {}
        for line in subprocess.run([exe, "plan", "lds", pod], capture_output=True, text=True, check=True).stdout.splitlines():
            got[" ".join(line.split(": ", 1)[0].split()[1:])] = fields(line)
        got["sizes"] = fields(subprocess.run([exe, "plan", "sizes", pod], capture_output=True, text=True, check=True).stdout)
        return got

    return run


def first_hits(handle, W, H):
    """the oracle's first-hit object id of the ray through every pixel's centre (tests/test_hip_one_light_general.py's)"""
    p1, p2, p3, o = handle.camera_basis().astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    d = p1 + ((xs + .5) / W)[..., None] * (p2 - p1) + ((ys + .5) / H)[..., None] * (p3 - p1) - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return handle.trace(np.broadcast_to(o, d.shape).reshape(-1, 3), d.reshape(-1, 3))["idx"].reshape(H, W)


def general_share(sc, ids):
    """the share of first-hit ids that are general spheres of `sc`"""
    sph = np.asarray(ids) - 1 - sc.n_planes
    return float(((sph >= 0) & G.general_mask(sc)[np.clip(sph, 0, None)]).mean())


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_is_what_it_is_named_for(plan, scenes, name):
    """(the table in general_grid_scenes' docstring: printed here, computed)"""
    sc = scene_of(scenes, name)
    n = G.ENTRIES[name][1]
    g = plan(sc)
    p, s = g["plain strict"], g["sizes"]
    print("%-14s %4d + %d lights  ldsTotal %6d  big %d gridInLds %d window %d  grid %dx%dx%d  items %4d  general %d" % (
        name, n, G.N_LIGHTS, s["ldsTotalStrict"], p["big"], p["gridInLds"], p["stealWindow"], s["gridDimX"], s["gridDimY"], s["gridDimZ"], s["gridItems"],
        int(G.general_mask(sc).sum())))
    assert s["nSpheres"] == n + G.N_LIGHTS == sc.n_spheres and s["nLights"] == G.N_LIGHTS
    assert (s["grid"], s["lists"], s["allTranslated"], s["planesRigid"], s["roomClosed"]) == (1, 0, 0, 1, 1), (name, s)
    in_lds, _ = G.CLASS[name]
    for b in BUILDS:
        q = g["plain " + b]
        assert (q["big"], q["coldInLds"], q["gridInLds"], q["fits"]) == (1, 0, in_lds, 1), (name, b, q)
        # the GPU module's other handles: without the grid (a large scene by its bytes or a small one, staged whole) and without lists
        assert g["no_grid " + b]["fits"] == 1 and g["no_shadow_lists " + b] == q, (name, b)
    info = stage_info(sc)
    assert info["closed_room"] and info["grid"] and not info["shadow_lists"], name
    assert stage_shadow_lists(sc) is None
    assert (G.staged_determinants(sc.spheres) == np.float32(1.0)).all()
    # the neighbour with one sphere fewer is not there yet
    down = plan(scene_of(scenes, name, n=n - 1))
    if n + G.N_LIGHTS == G.GRID_THRESHOLD:
        assert down["sizes"]["grid"] == 0 and down["plain strict"]["big"] == 0 and down["plain strict"]["coldInLds"] == 1, name
    else:
        assert down["sizes"]["grid"] == 1 and [down["plain " + b]["gridInLds"] for b in BUILDS] == [1, 1, 1], name


def test_mixed_l2_is_the_smallest_count_with_the_cell_lists_in_l2(plan, scenes):
    """(as tests/test_scene_sizes_cpu.py found its entries: every count below it, down to where the steal window is still 2, keeps gridInLds 1)"""
    n = G.ENTRIES["mixed_l2"][1]
    seen = []
    for m in range(n - 1, 0, -1):
        p = plan(scene_of(scenes, "mixed_l2", n=m))["plain strict"]
        seen.append((m, p["gridInLds"], p["stealWindow"]))
        assert p["gridInLds"] == 1, seen[-1]
        if p["stealWindow"] >= 2:  # the ladder of launch_plan.h gives up the window before the cell lists: from here down there is room
            break
    assert len(seen) >= 2, seen


def test_the_kinds_are_the_kinds(scenes):
    """every builder's records are the matrices its name says, each general; mixed interleaves one-word and four-word records and holds its
    constructed records"""
    I = np.eye(3, dtype=np.float32)
    mat3 = lambda sc: sc.spheres[:, :16].reshape(-1, 4, 4).transpose(0, 2, 1)[:, :3, :3]
    for name in ("quarter_turns", "shears", "ellipsoids", "rotations"):
        sc = scene_of(scenes, name)
        assert G.general_mask(sc).all(), name
        M = mat3(sc)[:-G.N_LIGHTS]
        if name == "quarter_turns":
            assert all(sorted(np.abs(m).ravel()) == [0] * 6 + [1] * 3 and not np.array_equal(m, I) for m in M)
            assert len({m.tobytes() for m in M}) == 23  # every turn other than the identity occurs
        elif name == "shears":
            assert all((np.diag(m) == 1).all() and np.count_nonzero(m - I) == 1 for m in M) and len({m.tobytes() for m in M}) == 36
        elif name == "ellipsoids":
            assert all(np.count_nonzero(m - np.diag(np.diag(m))) == 0 and np.diag(m).astype(np.float64).prod() == 1 for m in M)
            assert len({m.tobytes() for m in M}) == 12 and max(np.diag(m).max() / np.diag(m).min() for m in M) == 8
        else:
            assert all(np.abs(m.astype(np.float64) @ m.astype(np.float64).T - I).max() < 1e-6 and np.count_nonzero(m) == 9 for m in M)
    for name in ("mixed", "mixed_l2"):
        sc = scene_of(scenes, name)
        gm = G.general_mask(sc)
        assert 0.15 < (~gm).mean() < 0.25 and (gm[1:] != gm[:-1]).sum() >= (~gm).sum(), name  # plain balls among the general records, interleaved
        s, M = sc.spheres, mat3(sc)
        # the constructed tie: two records alike but for their material
        a, b = s[G.TIE_FIRST], s[G.TIE_SECOND]
        assert np.array_equal(a[:16], b[:16]) and a[38] == b[38] == G.TIE_RADIUS and not np.array_equal(a[16:38], b[16:38]) and gm[G.TIE_FIRST]
        c, r = s[:, 12:15].astype(np.float64), s[:, 38].astype(np.float64)
        ext = r[:, None] * np.sqrt((M.astype(np.float64) ** 2).sum(2))  # world half-extents (stage.cpp sphereBounds)
        others = np.ones(len(s), bool)
        others[[G.TIE_FIRST, G.TIE_SECOND]] = False
        # ... and nothing else within a unit of their surface along the axes, where the tie's rays start (a box test: conservative)
        gap = np.abs(c[others] - np.array(G.TIE_CENTRE)) - ext[others]
        assert (gap.max(1) > 1.0).all(), name
        # the sphere cut by the floor, the long ellipsoid against the spheres' x extent, the ball inside the glass ellipsoid
        assert c[G.CUT_BY_FLOOR, 1] < 1.0 < c[G.CUT_BY_FLOOR, 1] + ext[G.CUT_BY_FLOOR, 1]
        span = (c[:, 0] + ext[:, 0]).max() - (c[:, 0] - ext[:, 0]).min()
        assert 2 * ext[G.LONG_ELLIPSOID, 0] > span / 3, (ext[G.LONG_ELLIPSOID, 0], span)
        inner = (c[G.NEST_INNER] - c[G.NEST_OUTER]) / ext[G.NEST_OUTER]
        assert np.linalg.norm(np.abs(inner) + r[G.NEST_INNER] / ext[G.NEST_OUTER]) < 1 and s[G.NEST_OUTER, 16 + 16:16 + 19].any()


def test_a_determinant_an_ulp_off_one_gets_no_grid(plan, scenes):
    """The rule's other side (stage.cpp buildGrid: `!= 1.f`): the same scenes with ONE record nudged -- a scale (2, .5, 1.0000001), and a
    float32 rotation that rotations() drew and turned down -- are staged without a grid, in every build's plan."""
    sc = scene_of(scenes, "ellipsoids")
    twin = G.nudged(sc, 7, np.diag(np.array([2, .5, 1.0000001], np.float32)), "ellipsoids_nudged")
    report = {}
    rot = G.rotations(scenes["spheres_a169"], G.ENTRIES["rotations"][1], report=report)
    assert np.array_equal(rot.spheres, scene_of(scenes, "rotations").spheres)
    print("rotations: %d draws for %d records, %d turned down" % (report["draws"], G.ENTRIES["rotations"][1], len(report["rejected"])))
    assert report["draws"] == G.ENTRIES["rotations"][1] + len(report["rejected"]) and report["rejected"]
    twin2 = G.nudged(rot, 11, report["rejected"][0], "rotations_nudged")
    for base, t, k in ((sc, twin, 7), (rot, twin2, 11)):
        det = G.staged_determinants(t.spheres)
        off = np.flatnonzero(det != np.float32(1.0))
        assert off.tolist() == [k] and abs(float(det[k]) - 1.0) <= 2.0 ** -22, (t.name, off, det[k])  # one record, an ulp or two
        assert plan(base)["sizes"]["grid"] == 1
        g = plan(t)
        assert g["sizes"]["grid"] == 0 and g["sizes"]["lists"] == 0 and g["sizes"]["allTranslated"] == 0, t.name
        assert not stage_info(t)["grid"]
        for b in BUILDS:
            assert g["plain " + b] == g["no_grid " + b], (t.name, b)  # (the plan of the handle that was told to build none)


@pytest.mark.skipif(not available("oracle"), reason="oracle/libkajo_oracle.so not built (run __graft_entry__.build())")
@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_sees_the_general_records(scenes, name):
    """A condition on the inputs, met by the oracle alone: of the pixel-centre camera rays of the GPU module's frame at least 25 % first hit a
    general sphere. Measured (printed with -s): quarter_turns 0.332, shears 0.294, ellipsoids 0.321, rotations 0.332, mixed 0.270,
    mixed_l2 0.432. mixed's constructed records are among the hits."""
    sc = scene_of(scenes, name)
    ids = first_hits(OracleLib("oracle").create(sc, 1), *FRAME)
    share = general_share(sc, ids)
    print("%s: first hits on general spheres %.3f" % (name, share))
    assert share >= 0.25, (name, share)
    if name.startswith("mixed"):
        first = 1 + sc.n_planes
        seen = set(np.unique(ids).tolist())
        if name == "mixed":  # (in mixed_l2 the lattice's 488 stand in front of some of them)
            assert {first + G.CUT_BY_FLOOR, first + G.LONG_ELLIPSOID, first + G.NEST_OUTER, first + G.TIE_SECOND} <= seen, name
        assert first + G.TIE_FIRST not in seen  # (wherever the pair is met, the later record is the hit)
