"""Which scene reaches which path of kajo_hip_create: tests/scenes_extra.py SIZES against the host's own plan (tools/host_san.cpp `plan lds`
and `plan sizes`: kajo_amd/csrc/launch_plan.h kajoLdsPlan over stage.cpp's staging) and kajo_amd.renderer's host-only stage_info /
stage_shadow_lists. If a threshold of launch_plan.h or stage.cpp moves, the entry that no longer covers its path fails here by name, and
tests/test_hip_scene_sizes.py, which renders the entries, never quietly stops covering it. Run with -s for the plan line of every entry."""
import os
import shutil
import subprocess

import pytest

from kajo_amd.renderer import stage_info, stage_shadow_lists
from scenes_extra import SIZES, sized_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ("fast", "strict", "exact")
KIB = 1024


@pytest.fixture(scope="module")
def plan(tmp_path_factory, scenes):
    """plan(name, **changes) -> dict: "<staging> <numerics>" -> kajoLdsPlan's fields (+ ldsTotal: its ldsTotal(), `plan sizes`), "sizes" ->
    the fields of `plan sizes`. A plain build of the tool: the sanitised one runs in tests/test_sanitize_cpu.py."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("sizes")
    exe = str(d / "host_plan")
    src = [os.path.join(ROOT, "tools", "host_san.cpp"), os.path.join(ROOT, "kajo_amd", "csrc", "stage.cpp"),
           os.path.join(ROOT, "kajo_amd", "host", "scene", "SceneLoader.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "kajo_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "kajo_amd", "host"), *src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    base, cache = scenes["spheres_a169"], {}

    def fields(line):
        return {k: int(v) for k, v in (kv.split("=") for kv in line.split(": ", 1)[1].split())}

    def run(name, **changes):
        key = (name, tuple(sorted(changes.items())))
        if key not in cache:
            pod = str(d / "scene.pod")
            sized_scene(base, name, **changes).write_pod(pod)
            got = {}
            for line in subprocess.run([exe, "plan", "lds", pod], capture_output=True, text=True, check=True).stdout.splitlines():
                got[" ".join(line.split(": ", 1)[0].split()[1:])] = fields(line)
            got["sizes"] = s = fields(subprocess.run([exe, "plan", "sizes", pod], capture_output=True, text=True, check=True).stdout)
            for b in BUILDS:
                p = got["plain " + b]
                p["ldsTotal"] = s["ldsTotal" + b.capitalize()]
                # (launch_plan.h ldsTotal() restated: the scene copy and four waves' mailbox + helper areas)
                assert p["ldsTotal"] == ((p["ldsBytes"] + 15) & ~15) + p["wavesPerBlock"] * (p["helpBytes"] + p["accBytes"] + 64 * 16 * p["stealWindow"])
                assert p["fits"] == s["fits" + b.capitalize()] == (p["ldsTotal"] <= 160 * KIB)
            cache[key] = got
        return cache[key]

    return run


def one_down(name):
    return dict(n_spheres=SIZES[name]["n_spheres"] - 1)


def test_every_entry_has_its_plan_line(plan, scenes):
    """(the table above SIZES: printed here, computed, for every entry)"""
    for name, args in SIZES.items():
        g = plan(name)
        p, s = g["plain strict"], g["sizes"]
        assert s["nSpheres"] == args["n_spheres"] + args["n_lights"] and s["nLights"] == args["n_lights"]
        print("%-10s %5d + %3d lights  ldsTotal %6d  fits %d  big %d gridInLds %d window %d  grid %dx%dx%d (wanted %dx%dx%d)  bins %d  longest row %d" % (
            name, args["n_spheres"], args["n_lights"], p["ldsTotal"], p["fits"], p["big"], p["gridInLds"], p["stealWindow"], s["gridDimX"], s["gridDimY"],
            s["gridDimZ"], s["gridWantX"], s["gridWantY"], s["gridWantZ"], s["shadowN"], s["shadowMaxRow"]))
        # every entry is a large scene with its grid and its visibility lists: the classes _biglist_lg / _biglist, in all three builds alike
        assert s["grid"] == 1 and s["lists"] == 1, name
        for b in BUILDS:
            q = g["plain " + b]
            assert q["big"] == 1 and q["coldInLds"] == 0 and q["helpBytes"] == 512 and q["accBytes"] == 0, (name, b)
            assert {k: q[k] for k in ("gridInLds", "stealWindow", "ldsTotal", "fits")} == {k: p[k] for k in ("gridInLds", "stealWindow", "ldsTotal", "fits")}
            if name != "too_large":  # what the GPU module's other two handles per entry need: they fit as well
                assert g["no_grid " + b]["fits"] == 1 and g["no_shadow_lists " + b]["fits"] == 1, (name, b)
        info = stage_info(sized_scene(scenes["spheres_a169"], name))
        assert info["closed_room"] and info["grid"] and info["shadow_lists"], name


@pytest.mark.parametrize("name,window,below", [("window4", 4, None), ("window2", 2, 4), ("window1", 1, 2)])
def test_grid_ladder_in_lds(plan, name, window, below):
    """the grid's cell lists in LDS at each steal window of kajoLdsPlan's ladder; one sphere fewer is still on the rung above"""
    for b in BUILDS:
        p = plan(name)["plain " + b]
        assert (p["gridInLds"], p["stealWindow"]) == (1, window), (name, b, p)
        q = plan(name, **one_down(name))
        if below is None:  # stage.cpp buildGrid: no grid below 48 spheres, the lights among them: one fewer is no large scene at all
            assert SIZES[name]["n_spheres"] + SIZES[name]["n_lights"] == 48 and q["sizes"]["grid"] == 0 and q["plain " + b]["big"] == 0
        else:
            assert (q["plain " + b]["gridInLds"], q["plain " + b]["stealWindow"]) == (1, below), (name, b)


def test_grid_in_l2_by_size(plan):
    for b in BUILDS:
        p = plan("grid_in_l2")["plain " + b]
        assert (p["big"], p["gridInLds"], p["stealWindow"]) == (1, 0, 4) and plan("grid_in_l2")["sizes"]["lists"] == 1
        q = plan("grid_in_l2", **one_down("grid_in_l2"))["plain " + b]
        assert (q["gridInLds"], q["stealWindow"]) == (1, 1)
        # (and the rungs lie in the order the table gives them)
    assert SIZES["window4"]["n_spheres"] < SIZES["window2"]["n_spheres"] < SIZES["window1"]["n_spheres"] < SIZES["grid_in_l2"]["n_spheres"]


@pytest.mark.parametrize("name,bound", [("over48k", 48 * KIB), ("over64k", 64 * KIB)])
def test_lds_total_just_above(plan, name, bound):
    """capi.cpp kajo_hip_create calls setLds above 48 KiB (launch.inc.hip _set_lds, the coldInLds == 0 arm); 64 KiB is the default limit of
    dynamic LDS. One sphere (a 16-byte hot record) fewer is not above."""
    for b in BUILDS:
        p = plan(name)["plain " + b]
        assert bound < p["ldsTotal"] <= bound + 16 and p["coldInLds"] == 0, (name, b, p["ldsTotal"])
        assert plan(name, **one_down(name))["plain " + b]["ldsTotal"] <= bound
    # the entries below 48 KiB never reach the opt-in; the one the GPU module opens its process-order test with is `over64k`
    for small in ("window4", "window2", "window1", "grid_in_l2", "needle", "lights17", "lights33", "lights64", "lights171"):
        assert plan(small)["plain strict"]["ldsTotal"] <= 48 * KIB, small


def test_largest_and_too_large(plan):
    """one sphere is one 16-byte hot record: `largest` is the last count that fits, `too_large` the next, in each numerics build (large
    scenes carry no accBytes and the same helpBytes: the three builds share the limit)"""
    assert SIZES["too_large"] == dict(SIZES["largest"], n_spheres=SIZES["largest"]["n_spheres"] + 1)
    for b in BUILDS:
        p, q = plan("largest")["plain " + b], plan("too_large")["plain " + b]
        assert p["fits"] == 1 and 160 * KIB - 16 < p["ldsTotal"] <= 160 * KIB, (b, p["ldsTotal"])
        assert q["fits"] == 0 and q["ldsTotal"] == p["ldsTotal"] + 16
        assert p["hotBytes"] > 64 * KIB  # the known-answer trace and the AOV kernel stage this much: beyond the default as well


def test_needle_meets_the_clamp(plan):
    s = plan("needle")["sizes"]
    assert s["gridDimX"] == 128 and s["gridWantX"] > 128, s  # stage.cpp buildGrid: d > 128 ? 128
    assert s["gridDimY"] == s["gridWantY"] <= 8 and s["gridDimZ"] == s["gridWantZ"] <= 8
    assert s["gridMaxCell"] >= 8  # cells that hold many items each


@pytest.mark.parametrize("name,bins", [("lights17", 64), ("lights33", 64), ("lights64", 64), ("lights171", 32)])
def test_light_counts_and_bins(plan, scenes, name, bins):
    """stage.cpp buildShadowLists: N = 64 bins per face axis halves once nL * 6 * N * N > 2^22, from 171 lights on"""
    sc = sized_scene(scenes["spheres_a169"], name)
    lists = stage_shadow_lists(sc)
    assert lists is not None and lists["n"] == bins == plan(name)["sizes"]["shadowN"]
    assert len(lists["lights"]) == SIZES[name]["n_lights"] == sc.n_lights and SIZES[name]["n_lights"] > 16
    assert lists["start"].size == sc.n_lights * 6 * bins * bins + 1
    assert (SIZES[name]["n_lights"] * 6 * 64 * 64 > 1 << 22) == (bins == 32)
    if name == "lights171":
        assert 170 * 6 * 64 * 64 <= 1 << 22  # 171 is the first count that halves the bins


def test_cluster_rows_and_the_16_bit_offsets(plan):
    """stage.cpp buildShadowLists, "if (out.shadowStart[b0 + N] - base > 65535u) return;": a row of N bins whose items would not fit the
    16-bit offsets (shadowOff16 against shadowRowBase) drops the lists of the whole scene, and the grid answers its shadow rays. What is
    pinned here is the other side: the offsets of the longest rows a lattice scene has hold their row's length exactly. A sphere enters
    at most the N = 64 bins of a row, so a row passes 65 535 items only with 1 024 spheres or more whose cone of directions spans a
    whole row of one light -- spheres that touch or hold the light itself. Lattice spheres two units around a light do not come near:
    the longest row of `cluster` (3 000 spheres) has 2 597 items, of the same lattice at `largest`'s 9 036 spheres 7 419, a ninth of the
    limit. The fallback is not rendered: a scene that reaches it stages tens of millions of items, seconds per handle."""
    s = plan("cluster")["sizes"]
    assert s["lists"] == 1 and s["shadowN"] == 64
    assert s["shadowMaxOff16"] == s["shadowMaxRow"] <= 65535
    room = plan("cluster", shape="room")["sizes"]  # the same spheres spread over the room: the cluster's rows are the longer ones
    assert s["shadowMaxRow"] > 2 * room["shadowMaxRow"], (s["shadowMaxRow"], room["shadowMaxRow"])
    for name in SIZES:
        t = plan(name)["sizes"]
        assert t["shadowMaxOff16"] == t["shadowMaxRow"] <= 65535, name
