"""The cases of tests/test_hip_adaptive_launch_shapes.py (GPU) and tests/test_launch_shapes_cpu.py (the host's proof of which render kernel
each of them launches): not a test module. A case is a scene, a frame, S, a numerics build, create keywords and `paths`: for every length
of launch the case's cuts produce, the path kajo_hip_render takes for it --

  "split2", "split4"    the pass-split kernel behind the [pass][pixel] term table (KajoLaunchShape.split > 1, chunks == 1)
  "chunks3", ...        the sample-chunks kernel behind the [pass][sample][pixel] table (chunks > 1)
  "unsplit-w1", "-w4"   the unsplit kernel, a workgroup of one wave or of four (the plan's wavesPerBlock)

-- as tests/test_launch_shapes_cpu.py reads it from kajo_amd/csrc/launch_plan.h through `host_san plan shape`. Nothing here decides a
path: the table only says what each case is there for, and the CPU test fails by the case's name when the header no longer agrees."""
from kajo_amd import capi

SMALL, LARGE = (41, 23), (72, 40)  # ragged against the 64x16 tile on both axes; LARGE for scenes_extra.SIZES entries
CUTS = ((32,), (16, 2, 14), (16, 3, 13), (1,) * 32)
OWNERS = (1, 3)
PASSES = 32
BUILDS = {"fast": {}, "exact": dict(exact=True), "strict": dict(strict=True)}
W4_SPHERES, W4_LIGHTS, W4_SEED = 30, 3, 11  # scenes_extra.dense_scene: a small scene (no grid: fewer than 48 spheres) planned with four waves per block

NOSPLIT = dict(flags=capi.KAJO_FLAG_NO_SPLIT)
UNSPLIT1 = {4: "unsplit-w1", 3: "unsplit-w1", 2: "unsplit-w1", 1: "unsplit-w1"}
UNSPLIT4 = {4: "unsplit-w4", 3: "unsplit-w4", 2: "unsplit-w4", 1: "unsplit-w4"}
CHUNKS4 = {4: "chunks4", 3: "chunks4", 2: "chunks4", 1: "chunks4"}
# spheres_a169 with the SPLIT kernels allowed, by S (n = floor(sqrt(S)))
BY_S = {
    1: {4: "split4", 3: "unsplit-w1", 2: "split2", 1: "unsplit-w1"},  # n = 1: nothing to chunk
    3: {4: "split4", 3: "unsplit-w1", 2: "split2", 1: "unsplit-w1"},
    9: {4: "chunks3", 3: "chunks3", 2: "chunks3", 1: "chunks9"},
    16: {4: "split4", 3: "unsplit-w1", 2: "chunks8", 1: "chunks16"},  # four passes of 16 samples: the chunk table alone is 64 KiB
    31: {4: "split4", 3: "unsplit-w1", 2: "split2", 1: "chunks5"},  # n = 5
}


def _case(scene, size, spp, build, paths, **create):
    return dict(scene=scene, size=size, spp=spp, build=build, create=create, paths=paths)


def _cases():
    c = {}
    for S in (1, 3, 9, 16, 31):
        for b in ("fast", "exact"):
            c["spheres-S%d-%s-split" % (S, b)] = _case("spheres", SMALL, S, b, BY_S[S])
            c["spheres-S%d-%s-nosplit" % (S, b)] = _case("spheres", SMALL, S, b, UNSPLIT1, **NOSPLIT)
    for S in (1, 16):
        c["spheres-S%d-strict-split" % S] = _case("spheres", SMALL, S, "strict", BY_S[S])
        c["spheres-S%d-strict-nosplit" % S] = _case("spheres", SMALL, S, "strict", UNSPLIT1, **NOSPLIT)
    c["spheres-S4-no-one-light"] = _case("spheres", SMALL, 4, "exact", CHUNKS4, flags=capi.KAJO_FLAG_NO_ONE_LIGHT)
    c["spheres-S4-no-one-light-nosplit"] = _case("spheres", SMALL, 4, "exact", UNSPLIT1, flags=capi.KAJO_FLAG_NO_ONE_LIGHT | capi.KAJO_FLAG_NO_SPLIT)
    # (depth 0 sees the light's disc and nothing else: at 41x23 two units of eighteen have a pixel with any error, the median of the units'
    # worst error is 0 and no target can be set. 13x7 is two units, the light's edge in one: the median is half its worst error, the dark
    # unit retires at 16 and the other is still active at 32)
    c["spheres-S4-depth0"] = _case("spheres", (13, 7), 4, "exact", CHUNKS4, depth_limit=0)
    c["spheres-S4-ppl1"] = _case("spheres", SMALL, 4, "exact", {1: "chunks4"}, passes_per_launch=1)
    c["spheres-S4-ppl2"] = _case("spheres", SMALL, 4, "exact", {2: "chunks4", 1: "chunks4"}, passes_per_launch=2)
    c["spheres-S4-ppl3"] = _case("spheres", SMALL, 4, "exact", {3: "chunks4", 2: "chunks4", 1: "chunks4"}, passes_per_launch=3)
    c["spheres-S4-ppl16"] = _case("spheres", SMALL, 4, "exact", CHUNKS4, passes_per_launch=16)
    c["w4-S4-fast-split"] = _case("w4", SMALL, 4, "fast", CHUNKS4)
    c["w4-S4-fast-nosplit"] = _case("w4", SMALL, 4, "fast", UNSPLIT4, **NOSPLIT)
    c["w4-S16-exact-split"] = _case("w4", SMALL, 16, "exact", {**BY_S[16], 3: "unsplit-w4"})
    c["w4-S4-strict-nosplit"] = _case("w4", SMALL, 4, "strict", UNSPLIT4, **NOSPLIT)
    for name, paths in (("window4", UNSPLIT1), ("lights17", UNSPLIT4), ("over48k", UNSPLIT4)):
        for S in (4, 16):
            for b in BUILDS:
                c["%s-S%d-%s" % (name, S, b)] = _case(name, LARGE, S, b, paths)
    return c


CASES = _cases()
# the two cases of the legs "flags that must not move a bit" and "the readers know nothing of the flag"
FLAG_CASES = ("spheres-S16-exact-split", "window4-S4-exact")


def case_scene(scenes, key):
    """the scene of a case from the session's golden scenes"""
    from scenes_extra import dense_scene, sized_scene
    base = scenes["spheres_a169"]
    if key == "spheres":
        return base
    if key == "w4":
        return dense_scene(base, W4_SPHERES, W4_LIGHTS, seed=W4_SEED)
    return sized_scene(base, key)


def create_keywords(case):
    """HipRenderer's keywords of a case (without spp)"""
    return dict(BUILDS[case["build"]], **case["create"])


def launches(cuts, passes_per_launch=0, noise=True, done=0):
    """(now, passesDone) of every launch kajo_hip_render cuts the calls `cuts` into: passes_per_launch at the most (0: 16) and, on a handle
    with KAJO_FLAG_NOISE, none across an absolute multiple of four passes"""
    out = []
    for c in cuts:
        left = c
        while left > 0:
            now = min(left, passes_per_launch or 16)
            if noise:
                now = min(now, 4 - done % 4)
            out.append((now, done))
            done, left = done + now, left - now
    return out
