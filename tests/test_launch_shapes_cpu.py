"""Which render kernel every case of tests/test_hip_adaptive_launch_shapes.py launches, from the host's own plan: tools/host_san.cpp
`plan shape` stages the case's scene as kajo_hip_create does and prints kajo_amd/csrc/launch_plan.h's kajoLdsPlan / kajoLaunchShape for
each launch kajo_hip_render cuts the case's calls into, one owner and three. No threshold is restated here: a case says which path it is
there for (tests/adaptive_shape_cases.py `paths`), and if launch_plan.h moves a threshold the case that no longer covers its path fails
here by name, so that the GPU module never quietly stops covering it. Run with -s for the plan line of every case.

Not reached at these frames: chunks 2. kajoLaunchShape takes the LARGEST divisor q of n * n with now * q <= 16 whose table fits 48 KiB
unless an earlier one already fills the chip's 4096 wave slots (pixelBlocks * now * q >= 4096). With the 32 pixel blocks of 41x23, and
the 96 of 72x40, no q does, so S = 4 takes q = 4 at every launch length

    spheres-S4-ppl16 now=4 passesDone=16: split=4 chunks=4 ... wavesPerBlock=1 coldInLds=1 home=1 grouped=1 n=2 gridBlocks=32 pixelBlocks=32

and S = 16 takes 8 or 16 at two passes and one, and at three and four passes has no q whose table fits (3 * 16 * 64 * 16 bytes + the
scene copy is over 48 KiB). q = 2 needs an even n * n and a frame of at least 4096 / (2 * now) pixel blocks: 512 blocks (32 768 pixels)
at four passes. test_chunks_2_needs_a_frame_of_512_pixel_blocks pins that from the plan itself; the existing 1001x523 case of
tests/test_hip_adaptive.py is the only short-grid render beyond that size."""
import os
import shutil
import subprocess

import pytest

from adaptive_shape_cases import CASES, CUTS, OWNERS, case_scene, launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = (64, 16)


@pytest.fixture(scope="module")
def shape(tmp_path_factory, scenes):
    """shape(case dict, pairs, owner, owners) -> one dict of `plan shape`'s fields per (now, passesDone) pair. A plain build of the tool."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("shapes")
    exe = str(d / "host_plan")
    src = [os.path.join(ROOT, "tools", "host_san.cpp"), os.path.join(ROOT, "kajo_amd", "csrc", "stage.cpp"),
           os.path.join(ROOT, "kajo_amd", "host", "scene", "SceneLoader.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "kajo_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "kajo_amd", "host"), *src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    pods, cache = {}, {}

    def run(case, pairs, owner=0, owners=1, size=None):
        if case["scene"] not in pods:
            pods[case["scene"]] = str(d / (case["scene"] + ".pod"))
            case_scene(scenes, case["scene"]).write_pod(pods[case["scene"]])
        W, H = size or case["size"]
        args = [exe, "plan", "shape", pods[case["scene"]], W, H, TILE[0], TILE[1], case["spp"], case["build"], case["create"].get("flags", 0), owner, owners]
        args = tuple(str(a) for a in args) + tuple(str(v) for p in pairs for v in p)
        if args not in cache:  # (a large scene is staged anew by every call of the tool)
            cache[args] = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
        out = cache[args]
        assert len(out) == len(pairs)
        rows = [{k: int(v) for k, v in (kv.split("=") for kv in line.replace(":", "").split())} for line in out]
        for row, line, (now, done) in zip(rows, out, pairs):
            assert (row["now"], row["passesDone"]) == (now, done)
            row["line"] = line
        return rows

    run.exe = exe
    return run


def path_of(row):
    """the branch of kajo_hip_render a launch of this shape takes"""
    if row["chunks"] > 1:
        return "chunks%d" % row["chunks"]
    if row["split"] > 1:
        return "split%d" % row["split"]
    return "unsplit-w%d" % row["wavesPerBlock"]


def rows_of(shape, case, cuts, owners):
    """the launches of an adaptive handle of the case: [(row, short grid?)], every owner that has a tile"""
    pairs = launches(cuts, case["create"].get("passes_per_launch", 0))
    out = []
    for o in range(owners):
        rows = shape(case, pairs, o, owners)
        if rows[0]["gridBlocks"]:
            out += [(r, r["passesDone"] >= 16) for r in rows]
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_every_launch_of_the_case_takes_the_path_the_case_is_named_for(shape, name):
    """before pass 16 (whole grids: the noise handle's launches) and behind it (short grids, once a unit has retired at 16: the condition
    the GPU test asserts of every case), for every cut, one owner and three"""
    case = CASES[name]
    seen = {False: set(), True: set()}
    for cuts in CUTS:
        for owners in OWNERS:
            for row, short in rows_of(shape, case, cuts, owners):
                assert path_of(row) == case["paths"].get(row["now"]), (name, cuts, owners, "short grid" if short else "whole grid", row["line"])
                assert row["launchGroups"] <= 1 and not row["parted"], (name, row["line"])  # (a noise handle's launches: one group at the most)
                seen[short].add(row["now"])
    # every length the case names is launched with a short grid
    assert seen[True] == set(case["paths"]), (name, seen)
    row = shape(case, [(4, 16)])[0]
    print("%-34s %s" % (name, row["line"]))
    # what the case's name says of its plan
    assert row["n"] * row["n"] <= case["spp"] < (row["n"] + 1) ** 2
    assert row["grouped"] == (row["coldInLds"] and case["build"] != "strict")
    assert (row["home"] == 2) == ("no-one-light" in name)
    if case["scene"] in ("spheres", "w4"):
        assert row["coldInLds"] == 1 and row["wavesPerBlock"] == (4 if case["scene"] == "w4" else 1), (name, row["line"])
    else:
        assert row["coldInLds"] == 0 and row["wavesPerBlock"] == (1 if case["scene"] == "window4" else 4), (name, row["line"])
    if case["scene"] == "over48k":
        assert row["ldsTotal"] > 48 * 1024, (name, row["line"])  # (the large-LDS opt-in of kajo_hip_create)


def test_the_table_covers_every_path_with_a_short_grid(shape):
    """each of the issue's paths, by the cases that reach it behind the first retirement"""
    reached = {}

    def note(what, name):
        reached.setdefault(what, set()).add(name)

    for name, case in CASES.items():
        for cuts in CUTS:
            for owners in OWNERS:
                for row, short in rows_of(shape, case, cuts, owners):
                    if not short:
                        continue
                    p = path_of(row)
                    note(p if not p.startswith("chunks") or row["chunks"] <= 4 else "chunks above 4", name)
                    if row["coldInLds"] == 0:
                        note("coldInLds == 0", name)
                    if row["home"] == 2:
                        note("home == 2", name)
                    if not row["grouped"]:
                        note("not grouped", name)
                    if not row["grouped"] and row["coldInLds"]:
                        note("STRICT, small scene", name)
                    if row["startsInside"] or row["endsInside"]:
                        note("a group handed over through carry", name)
                    if row["wavesPerBlock"] == 4 and row["coldInLds"] and p.startswith(("chunks", "split")):
                        note("SPLIT kernels over units of four pixel blocks", name)
    for what in sorted(reached):
        print("%-48s %3d cases, e.g. %s" % (what, len(reached[what]), sorted(reached[what])[0]))
    wanted = ("split2", "split4", "chunks3", "chunks4", "chunks above 4", "unsplit-w1", "unsplit-w4", "coldInLds == 0", "home == 2", "not grouped",
              "STRICT, small scene", "a group handed over through carry", "SPLIT kernels over units of four pixel blocks")
    missing = [w for w in wanted if w not in reached]
    assert not missing, missing
    assert "chunks2" not in reached  # (the module's docstring; a case that reaches it belongs in `wanted`)


def test_chunks_2_needs_a_frame_of_512_pixel_blocks(shape):
    """the docstring's claim, from the plan: S = 4 at four passes takes chunks 2 from 512 pixel blocks on and 4 below"""
    case = CASES["spheres-S4-ppl16"]
    at = lambda size: shape(case, [(4, 16)], size=size)[0]
    big, below = at((256, 128)), at((256, 112))
    assert (big["pixelBlocks"], big["chunks"]) == (512, 2), big["line"]
    assert (below["pixelBlocks"], below["chunks"]) == (448, 4), below["line"]
    assert all(at(size)["chunks"] == 4 for size in ((41, 23), (72, 40)))


@pytest.mark.parametrize("noise", [True, False], ids=["noise", "plain"])
@pytest.mark.parametrize("ppl", [0, 1, 2, 3, 16])
def test_the_cuts_of_kajo_hip_render_are_the_ones_this_table_is_built_from(shape, ppl, noise):
    """launches() (tests/adaptive_shape_cases.py) restates the cut rule; `host_san plan cuts` prints kajoLaunchPasses, which kajo_hip_render
    calls: for every entry of CUTS, from pass 0 and from pass 5"""
    for cuts in CUTS:
        for done in (0, 5):
            args = [shape.exe, "plan", "cuts", ppl, int(noise), done, *cuts]
            out = subprocess.run([str(a) for a in args], capture_output=True, text=True, check=True).stdout.split()
            got = list(zip(map(int, out[0::2]), map(int, out[1::2])))
            assert got == launches(cuts, ppl, noise, done), (cuts, ppl, noise, done)
            assert sum(now for now, _ in got) == sum(cuts)


def test_the_tool_refuses_what_create_refuses(shape):
    with pytest.raises(subprocess.CalledProcessError):
        shape(dict(CASES["spheres-S4-ppl16"], build="quick"), [(4, 16)])
