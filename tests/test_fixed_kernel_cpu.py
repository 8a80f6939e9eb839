"""The EXACT build's one-light small-scene kernel instances with compile-time plane and sphere counts (kajo_amd/csrc/kernel_exact_fixed.cpp,
fixed_counts.h; integrator.inc.hip trace NP / NS), checked without a GPU: what the compiler made of each instance -- the budgets of
kajo_render_exact_simple (tests/test_simple_kernel_resources_cpu.py), whose arithmetic they repeat, but for the static instruction count,
which unrolling raises and which is pinned where it was measured so that drift shows --, that the Makefile compiles the unit with
kernel_exact.hip's flags and links it, that fixed_counts.h's table, the unit's kernels and the launcher's choice agree one to one, and which
kernel tools/host_san.cpp `plan kernel` names for scenes with and without a table entry. (That no kernel from before moved is
tests/test_noise_cpu.py's and tests/test_adaptive_cpu.py's digest comparison, and the simple kernel's own budgets its own test.)"""
import os
import re
import shutil
import subprocess

import pytest

import devicecode
from framelib import bits as _bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
# static vector instructions per instance as measured (the simple kernel: 1959; the walk of 6 planes and 5 spheres written out: 16
# correctly rounded divisions where the loops held 3), held within 3 % either way
VALU_MEASURED = {(6, 5): 2258}
VALU_SLACK = 0.03


def table():
    """fixed_counts.h's pairs, from its text: the X(planes, spheres) entries of KAJO_FIXED_COUNTS"""
    text = open(os.path.join(CSRC, "fixed_counts.h")).read()
    body = re.search(r"^#define KAJO_FIXED_COUNTS\(X\)(.*)$", text, re.M).group(1)
    pairs = [(int(p), int(s)) for p, s in re.findall(r"X\((\d+), (\d+)\)", body)]
    assert re.sub(r"X\(\d+, \d+\)", "", body).strip() == "", body
    return pairs


def name_of(pair):
    return "kajo_render_exact_p%ds%d" % pair


def _make_line(target_src):
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all"], capture_output=True, text=True, check=True).stdout
    return plan, next(l for l in plan.splitlines() if l.startswith("hipcc") and target_src in l and " -c " in l)


@pytest.fixture(scope="module")
def compiled():
    """(resource remarks per kernel, device assembly) of the unit, by the Makefile's own command"""
    b = devicecode.build("kernel_exact_fixed.cpp")
    return b.resources, b.asm


def test_the_table_is_small_and_holds_the_benchmarked_scene(scenes):
    pairs = table()
    assert 1 <= len(pairs) <= 3 and len(set(pairs)) == len(pairs) and sorted(VALU_MEASURED) == sorted(pairs)
    # taken from the golden set's simple one-light scenes (tests/test_one_light_routing_cpu.py SIMPLE_GOLDEN), all of them one room
    golden = {(scenes[k].n_planes, scenes[k].n_spheres) for k in ("spheres_a1", "spheres_a43", "spheres_a169", "test_a1")}
    assert golden == {(6, 5)} and golden <= set(pairs)


def test_the_unit_holds_exactly_the_tables_kernels_within_the_budgets(compiled):
    res, asm = compiled
    pairs = table()
    assert sorted(res) == sorted(name_of(p) for p in pairs), sorted(res)
    for pair in pairs:
        kernel = name_of(pair)
        r = res[kernel]
        assert r["Occupancy"] == 5 and r["VGPRs"] <= 96 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (kernel, r)
        body = devicecode.body(asm, kernel)
        assert not re.search(r"\n\s+flat_(load|store|atomic)", body) and not re.search(r"\n\s+scratch_", body), kernel
        assert "v_div_scale_f32" not in body and "v_div_fmas_f32" not in body and "v_div_fixup_f32" in body, kernel
        n = len(re.findall(r"\n\s+v_\w+", body))
        print("%s: %d static VALU instructions, %d v_div_fixup_f32" % (kernel, n, body.count("v_div_fixup_f32")))
        want = VALU_MEASURED[pair]
        assert (1 - VALU_SLACK) * want <= n <= (1 + VALU_SLACK) * want, "%s: %d VALU instructions, measured %d" % (kernel, n, want)


def test_the_walk_is_straight_line_code(compiled):
    """One correctly rounded division per plane and two per sphere are written out between the kernel's label and its end -- the loops held
    one and two -- beside the eight of the rest of the kernel (camera block 1, vertex and shadow result 3, light and BSDF 4: the blocks of
    tools/isa_blocks.sh, the same eight in kajo_render_exact_simple)."""
    _, asm = compiled
    elsewhere = 8
    for p, s in table():
        kernel = name_of((p, s))
        body = devicecode.body(asm, kernel)
        assert body.count("v_div_fixup_f32") == elsewhere + p + 2 * s, (kernel, body.count("v_div_fixup_f32"))


def test_the_makefile_compiles_it_with_the_exact_units_flags_and_links_it():
    devicecode.need_tools()
    plan, fixed = _make_line("kernel_exact_fixed.cpp")
    strip = lambda l, src, obj: [w for w in l.split() if w not in ("-x", "hip") and not w.endswith(src) and not w.endswith(obj)]
    exact = next(l for l in plan.splitlines() if l.startswith("hipcc") and l.rstrip().split()[-3].endswith("kernel_exact.hip"))
    assert strip(exact, "kernel_exact.hip", "kernel_exact.o") == strip(fixed, "kernel_exact_fixed.cpp", "kernel_exact_fixed.o")
    assert "-ffp-contract=off" in fixed.split()
    link = next(l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l and l.split()[l.split().index("-o") + 1].endswith("libkajo_hip.so"))
    assert any(w.endswith("kernel_exact_fixed.o") for w in link.split()) and any(w.endswith("kernel_exact_simple.o") for w in link.split())
    # the launcher of the EXACT unit, and of no other, is told of it
    for unit, told in (("kernel_exact.hip", True), ("kernel_strict.hip", False), ("kernel_fast.hip", False)):
        assert ("#define KAJO_FIXED_LAUNCH kajo_render_exact_fixed" in open(os.path.join(CSRC, unit)).read()) == told, unit


@pytest.fixture(scope="module")
def kernel_name(tmp_path_factory):
    """kernel_name(scene) -> what `host_san plan kernel` prints for it"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("fixed_routing")
    exe = str(d / "host_plan")
    src = [os.path.join(ROOT, "tools", "host_san.cpp"), os.path.join(CSRC, "stage.cpp"), os.path.join(ROOT, "kajo_amd", "host", "scene", "SceneLoader.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "kajo_amd", "host"), *src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(sc):
        pod = str(d / "scene.pod")
        sc.write_pod(pod)
        line = subprocess.run([exe, "plan", "kernel", pod], capture_output=True, text=True, check=True).stdout.strip()
        got = dict(kv.split("=") for kv in line.split(": ", 1)[1].split())
        assert (int(got["nPlanes"]), int(got["nSpheres"]), int(got["nLights"])) == (sc.n_planes, sc.n_spheres, sc.n_lights), line
        return got["kernel"]

    return run


def test_which_scenes_reach_a_fixed_instance(kernel_name, scenes):
    from fixed_instance_scenes import far_sphere_twin, without_a_sphere
    from one_light_scenes import scaled_plane_twin, turned_twin
    pairs = table()
    for k in ("spheres_a1", "spheres_a43", "spheres_a169", "test_a1"):
        assert kernel_name(scenes[k]) == "kajo_render_exact_p6s5", k
    base = scenes["spheres_a169"]
    # one sphere more, one sphere fewer: simple scenes still, of counts without an entry
    more, fewer = far_sphere_twin(base)[0], without_a_sphere(base)
    assert (more.n_planes, more.n_spheres) == (6, 6) and (fewer.n_planes, fewer.n_spheres) == (6, 4)
    assert (6, 6) not in pairs and (6, 4) not in pairs
    assert kernel_name(more) == "kajo_render_exact_simple" and kernel_name(fewer) == "kajo_render_exact_simple"
    # the counts alone do not send a scene there: a general record or a scaled plane goes where it went, whatever it counts
    turned = turned_twin(without_a_sphere(base))[0]
    assert (turned.n_planes, turned.n_spheres) == (6, 5) and kernel_name(turned) == "kajo_render_exact"
    assert kernel_name(scaled_plane_twin(base)[0]) == "kajo_render_exact"
    # ... nor do they for a scene of several lights
    assert kernel_name(scenes["caustics_a169"]) == "kajo_render_exact_lights"


def test_the_launcher_picks_by_the_function_the_printout_calls():
    """launch.inc.hip asks fixed_counts.h's kajoFixedKernelName inside the simple scenes' branch, before the simple kernel's launch; the unit's
    launcher and its LDS opt-in are stamped from the same table"""
    text = open(os.path.join(CSRC, "launch.inc.hip")).read()
    branch = text[text.index("args->scene.allTranslated && args->scene.planesRigid"):]
    pick, simple = branch.index("kajoFixedKernelName(args->scene.nPlanes, args->scene.nSpheres)"), branch.index("KAJO_CAT(KAJO_SIMPLE_LAUNCH, _launch)(args")
    assert 0 < pick < simple
    unit = open(os.path.join(CSRC, "kernel_exact_fixed.cpp")).read()
    assert unit.count("KAJO_FIXED_COUNTS(") == 2 and "#define KAJO_FIXED_KERNELS KAJO_FIXED_COUNTS" in unit
    # (the printed name and the kernel's symbol are spelled from the same two numbers: name_of() above restates both)
    header = open(os.path.join(CSRC, "fixed_counts.h")).read()
    assert 'return "kajo_render_exact_p" #P "s" #S;' in header and "#define KAJO_FIXED_NAME(P, S) kajo_render_exact_p##P##s##S" in header


# ---- the family of 6 + 5 scenes (tests/fixed_instance_scenes.py family) the instance is rendered on (tests/test_hip_fixed_instance.py) ----
FAMILY_FRAMES = [(64, 16), (72, 40)]
FAMILY_S, FAMILY_PASSES, FAMILY_SEED = 4, 5, 0o715517
FAMILY_NAMES = (["light_at_%d" % k for k in range(4)] + ["planes_reversed", "materials_1", "materials_2", "materials_19", "nested", "overlapping",
                "coincident", "touching_floor", "light_in_ceiling", "camera_in_glass", "test_a1", "spheres_a1"])


def test_the_family_is_what_it_says(scenes):
    """the members by name, none missing; what each is built to be, from its records"""
    import numpy as np
    from fixed_instance_scenes import NAMES, family
    fam = family(scenes)
    assert list(fam) == NAMES == FAMILY_NAMES
    base = scenes["spheres_a169"]
    emits = lambda sc: np.flatnonzero((sc.spheres[:, 28:32] != 0).any(1)).tolist()
    key = lambda recs: sorted(map(bytes, recs))
    for name, sc in fam.items():
        assert (sc.n_planes, sc.n_spheres, sc.n_lights) == (6, 5, 1), name
        # (centre, radius) spheres: the transform is a translation
        T = sc.spheres[:, :16].reshape(-1, 4, 4).copy()
        T[:, 3, :3] = 0
        assert (T == np.eye(4, dtype=np.float32)).all(), name
    for k in range(4):
        sc = fam["light_at_%d" % k]
        assert emits(sc) == [k] and key(sc.spheres) == key(base.spheres)
        assert np.array_equal(np.delete(sc.spheres, k, axis=0), base.spheres[:4])  # the other records in their order
    assert np.array_equal(fam["planes_reversed"].planes, base.planes[::-1]) and np.array_equal(fam["planes_reversed"].spheres, base.spheres)
    kinds = set()
    for name in FAMILY_NAMES:
        if name.startswith("materials_"):
            sc = fam[name]
            assert np.array_equal(sc.spheres[:, :16], base.spheres[:, :16]) and np.array_equal(sc.planes[:, :16], base.planes[:, :16]) and emits(sc) == [4]
            for m in np.concatenate([sc.planes[:, 16:38], sc.spheres[:4, 16:38]]):
                d, s, t, e = m[4:7].any(), m[8:11].any(), m[16:19].any(), m[20]
                assert not (t and e == 0), name  # no glass over exponent 0
                kinds.add((bool(d), bool(s), bool(t), bool(e == 0)))
    assert len(kinds) == 5, kinds  # the five classes all occur among the three seeds
    dist = lambda sc, i, j: float(np.linalg.norm(sc.spheres[i, 12:15].astype(np.float64) - sc.spheres[j, 12:15]))
    sc = fam["nested"]
    assert sc.spheres[0, 32:35].any() and sc.spheres[3, 20:23].any() and dist(sc, 0, 3) + sc.spheres[3, 38] < sc.spheres[0, 38]
    sc = fam["overlapping"]
    assert abs(sc.spheres[1, 38] - sc.spheres[2, 38]) < dist(sc, 1, 2) < sc.spheres[1, 38] + sc.spheres[2, 38]
    sc = fam["coincident"]
    assert dist(sc, 1, 3) == 0 and sc.spheres[1, 38] == sc.spheres[3, 38] and not np.array_equal(sc.spheres[1, 16:38], sc.spheres[3, 16:38])
    sc = fam["touching_floor"]
    cy, r, floor = sc.spheres[2, 13], sc.spheres[2, 38], sc.planes[0, 13]
    assert np.float64(cy) + np.float64(r) == np.float64(floor) and np.float32(cy + r) == floor and r != 1.0
    sc = fam["light_in_ceiling"]
    assert emits(sc) == [4] and abs(sc.spheres[4, 13] - sc.planes[5, 13]) < sc.spheres[4, 38]
    sc = fam["camera_in_glass"]
    eye = np.linalg.inv(sc.view.reshape(4, 4).T.astype(np.float64))[:3, 3]
    assert sc.spheres[0, 32:35].any() and np.linalg.norm(eye - sc.spheres[0, 12:15]) < sc.spheres[0, 38]
    assert fam["test_a1"] is scenes["test_a1"] and fam["spheres_a1"] is scenes["spheres_a1"]
    assert not np.array_equal(fam["test_a1"].proj, base.proj)


def test_the_twin_before_the_last_sphere(scenes):
    import numpy as np
    from fixed_instance_scenes import far_sphere_twin
    base = scenes["spheres_a169"]
    last, ids_last = far_sphere_twin(base)
    twin, ids = far_sphere_twin(base, before_last=True)
    assert np.array_equal(ids_last, np.arange(12)) and np.array_equal(last.spheres[:5], base.spheres)
    assert np.array_equal(ids, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12])
    assert np.array_equal(twin.spheres[[0, 1, 2, 3, 5]], base.spheres) and np.array_equal(twin.spheres[4], last.spheres[5])
    assert twin.n_lights == 1 and np.array_equal(twin.planes, base.planes)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_every_member_runs_the_instance_and_its_twin_the_simple_kernel(kernel_name, scenes, name):
    from fixed_instance_scenes import family, far_sphere_twin
    sc = family(scenes)[name]
    twin, _ = far_sphere_twin(sc, before_last=True)
    assert (twin.n_planes, twin.n_spheres, twin.n_lights) == (6, 6, 1)
    assert kernel_name(sc) == "kajo_render_exact_p6s5", name
    assert kernel_name(twin) == "kajo_render_exact_simple", name


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_the_oracle_renders_member_and_twin_alike(scenes, name):
    """The precondition of the comparison of the kernels (tests/test_hip_fixed_instance.py): in the oracle the twin's frame is the member's
    bit for bit, not-a-number where it is not a number -- no ray meets the far sphere, and a ray that is not a number ends on the same record
    in both. A condition every member meets, at both frame sizes."""
    import numpy as np
    from oraclelib import OracleLib, available
    from fixed_instance_scenes import family, far_sphere_twin
    if not available("oracle"):
        pytest.skip("oracle not built")
    lib = OracleLib("oracle")
    sc = family(scenes)[name]
    twin, _ = far_sphere_twin(sc, before_last=True)
    for w, h in FAMILY_FRAMES:
        a = lib.create(sc, 1).render(w, h, S=FAMILY_S, passes=FAMILY_PASSES, seed=FAMILY_SEED)
        b = lib.create(twin, 1).render(w, h, S=FAMILY_S, passes=FAMILY_PASSES, seed=FAMILY_SEED)
        same = ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all(-1)
        assert same.all(), "%s at %dx%d: %d pixels differ, first at %s" % (name, w, h, int((~same).sum()), np.argwhere(~same)[:4].tolist())
        assert np.isfinite(a[..., :3]).all(-1).mean() > 0.99, (name, w, h)  # (a frame, not a field of NaN: there is something to compare)


def test_every_sphere_id_is_some_pixels_first_hit(scenes):
    """From the oracle's own first-hit ids (camera_ray and trace: tests/test_aov_oracle_cpu.py's path), pass 1 at 72 x 40: over the family every
    sphere id 7 .. 11 is the first hit of some pixel, so no literal sphere id of the unrolled walk goes unexercised -- and the light is seen
    as every one of them; the twin meets, ray for ray, the member's object under the twin's id map."""
    import numpy as np
    from oraclelib import OracleLib, available, camera_ray
    from fixed_instance_scenes import family, far_sphere_twin
    if not available("oracle"):
        pytest.skip("oracle not built")
    lib = OracleLib("oracle")
    w, h = FAMILY_FRAMES[1]
    seen, light_seen_as = set(), set()
    for name, sc in family(scenes).items():
        o = lib.create(sc, 1)
        rays = [camera_ray(o, w, h, FAMILY_S, x, y, s, npass=1, seed=FAMILY_SEED)[:2] for y in range(h) for x in range(w) for s in range(FAMILY_S)]
        O, D = np.array([r[0] for r in rays], np.float32), np.array([r[1] for r in rays], np.float32)
        idx = o.trace(O, D)["idx"]
        twin, ids = far_sphere_twin(sc, before_last=True)
        assert np.array_equal(lib.create(twin, 1).trace(O, D)["idx"], ids[idx]), name
        seen |= set(np.unique(idx).tolist())
        light = 7 + int(np.flatnonzero((sc.spheres[:, 28:32] != 0).any(1))[0])
        if (idx == light).any():
            light_seen_as.add(light)
    assert seen >= set(range(7, 12)) and seen >= set(range(1, 7)), sorted(seen)
    assert light_seen_as == set(range(7, 12)), sorted(light_seen_as)
