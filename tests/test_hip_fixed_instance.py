"""The EXACT build's fixed-count instance against its twin, bit for bit. kajo_render_exact_p6s5 (kajo_amd/csrc/kernel_exact_fixed.cpp) is
kajo_render_exact_simple with the walk compiled for 6 planes and 5 spheres: the same operations on the same operands in the same order, so a
scene that runs it must give, in every reader, what the simple kernel gives. The base is the golden scene spheres_a169 (6 planes, 5 spheres: an
entry of fixed_counts.h's table); the twin is the base with one more (centre, radius) sphere appended last, far outside the room
(tests/fixed_instance_scenes.py far_sphere_twin): 6 planes and 6 spheres, no entry, the simple kernel. Which kernel each runs is asserted from
`host_san plan kernel`, the launcher's own choice printed; that the new sphere is never hit and never shadows the light -- and that no ray that
is not a number ends on it where the base ends it on its own last sphere -- is checked on the CPU oracle first: its frames of base and twin
must be bit-identical, or the comparison of the kernels would mean nothing. KAJO_FLAG_NO_SPLIT, as tests/test_hip_one_light_general.py sets it:
small frames would otherwise run the split kernel, which has no fixed instance. The render kernels expose no generator state; what a
handle keeps of a render is compared whole instead, through the digests of its planes (kajo_hip_digest)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from framelib import bits
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from fixed_instance_scenes import far_sphere_twin, without_a_sphere

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0o715517
NOSPLIT = capi.KAJO_FLAG_NO_SPLIT
S = 4
PASSES = 5  # crosses the boundary of the group of passes 1-4
FRAMES = [(64, 16), (16, 16), (72, 40)]  # one block row; less than a tile; a height that is no multiple of 16, several blocks
frames = pytest.mark.parametrize("size", FRAMES, ids=["%dx%d" % f for f in FRAMES])


@pytest.fixture(scope="module")
def pair(scenes):
    """(base, twin, ids): spheres_a169 and its far-sphere twin, after the checks that make the comparison mean something"""
    from oraclelib import OracleLib, available
    base = scenes["spheres_a169"]
    twin, ids = far_sphere_twin(base)
    assert base.n_lights == twin.n_lights == 1 and (twin.n_planes, twin.n_spheres) == (base.n_planes, base.n_spheres + 1)
    assert np.array_equal(ids, np.arange(ids.size))
    if not available("oracle"):
        pytest.skip("oracle not built")
    lib = OracleLib("oracle")
    for w, h in FRAMES:
        a = lib.create(base, 1).render(w, h, S=S, passes=PASSES, seed=SEED)
        b = lib.create(twin, 1).render(w, h, S=S, passes=PASSES, seed=SEED)
        assert np.array_equal(bits(a), bits(b)), "the oracle meets the far sphere at %dx%d" % (w, h)
    return base, twin, ids


@pytest.fixture(scope="module")
def kernel_name(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("fixed_plan")
    exe = str(d / "host_plan")
    csrc = os.path.join(ROOT, "kajo_amd", "csrc")
    src = [os.path.join(ROOT, "tools", "host_san.cpp"), os.path.join(csrc, "stage.cpp"), os.path.join(ROOT, "kajo_amd", "host", "scene", "SceneLoader.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "-I" + os.path.join(ROOT, "kajo_amd", "host"), *src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(sc):
        pod = str(d / "scene.pod")
        sc.write_pod(pod)
        line = subprocess.run([exe, "plan", "kernel", pod], capture_output=True, text=True, check=True).stdout.strip()
        return dict(kv.split("=") for kv in line.split(": ", 1)[1].split())["kernel"]

    return run


def test_the_base_runs_the_instance_and_its_neighbours_the_simple_kernel(pair, kernel_name):
    """one case per table entry (there is one), and the counts on either side of it"""
    base, twin, _ = pair
    assert kernel_name(base) == "kajo_render_exact_p6s5"
    assert (twin.n_planes, twin.n_spheres) == (6, 6) and kernel_name(twin) == "kajo_render_exact_simple"
    fewer = without_a_sphere(base)
    assert (fewer.n_planes, fewer.n_spheres) == (6, 4) and kernel_name(fewer) == "kajo_render_exact_simple"
    # ... and both neighbours render: finite frames, the twin's the base's (below), the smaller scene's another
    with HipRenderer(fewer, 64, 16, spp=S, seed=SEED, exact=True, flags=NOSPLIT) as r:
        f = r.render(PASSES).radiance()[..., :3].copy()
    with HipRenderer(base, 64, 16, spp=S, seed=SEED, exact=True, flags=NOSPLIT) as r:
        b = r.render(PASSES).radiance()[..., :3].copy()
    assert np.isfinite(f).all(-1).mean() > 0.99 and not np.array_equal(bits(f), bits(b))


@frames
def test_radiance_counters_and_digests(pair, size):
    base, twin, _ = pair
    W, H = size

    def run(sc, cuts):
        with HipRenderer(sc, W, H, spp=S, seed=SEED, exact=True, flags=NOSPLIT, counters=True) as r:
            for c in cuts:
                r.render(c).wait()
            return r.radiance().copy(), r.counters(), r.digest()
    a, ca, da = run(base, (PASSES,))
    assert np.isfinite(a[..., :3]).all(-1).mean() > 0.99 and ca["passes"] == PASSES and ca["paths"] == PASSES * S * W * H
    for sc, cuts in ((twin, (PASSES,)), (twin, (4, 1)), (base, (4, 1))):
        b, cb, db = run(sc, cuts)
        assert np.array_equal(bits(a), bits(b)), (sc.name, cuts, np.argwhere((bits(a) != bits(b)).any(-1))[:4].tolist())
        for k in ("paths", "traversals", "vertices", "passes"):
            assert ca[k] == cb[k], (sc.name, cuts, k, ca[k], cb[k])
        # (the COUNTERS plane holds the number of launches too: it is compared between handles that were driven alike)
        drop = () if cuts == (PASSES,) else ("COUNTERS",)
        assert {k: v for k, v in da.items() if k not in drop} == {k: v for k, v in db.items() if k not in drop}, (sc.name, cuts)


@pytest.mark.parametrize("specular", [False, True], ids=["first-hit", "specular-following"])
@frames
def test_raw_aovs_and_matte_tables(pair, size, specular):
    base, twin, ids = pair
    W, H = size

    def run(sc):
        with HipRenderer(sc, W, H, spp=S, seed=SEED, exact=True, flags=NOSPLIT, aov=True, aov_specular=specular, matte=True) as r:
            r.render(PASSES).wait()
            aov, matte = r.aov(), r.matte()
            return aov["raw"], aov["samples"], matte, r.radiance().copy()
    (A, B), n, m, f = run(base)
    assert n > 0 and A[..., 3].max() > 0 and (m["ids"] > base.n_planes).any()
    (A2, B2), n2, m2, f2 = run(twin)
    assert n2 == n and np.array_equal(bits(f), bits(f2))
    assert np.array_equal(bits(A), bits(A2)) and np.array_equal(bits(B), bits(B2))
    assert np.array_equal(m["ids"], m2["ids"]) and np.array_equal(m["counts"], m2["counts"])  # (the id map is the identity)


@frames
def test_three_tile_owners_gathered(pair, size):
    from test_hip_pass_cuts import render_cuts
    base, twin, _ = pair
    W, H = size
    kw = dict(exact=True, flags=NOSPLIT, spp=S)
    whole, _ = render_cuts(base, W, H, (PASSES,), **kw)
    want, _ = render_cuts(base, W, H, (PASSES,), owners=3, **kw)
    assert np.array_equal(bits(want), bits(whole))
    for cuts in ((PASSES,), (4, 1)):
        got, _ = render_cuts(twin, W, H, cuts, owners=3, **kw)
        assert np.array_equal(bits(got), bits(want)), cuts


@frames
def test_reset_and_render_again_on_the_same_handle(pair, size):
    base, twin, _ = pair
    W, H = size
    kw = dict(spp=S, seed=SEED, exact=True, flags=NOSPLIT, counters=True)
    with HipRenderer(twin, W, H, **kw) as r:
        want = r.render(PASSES).radiance().copy()
    with HipRenderer(base, W, H, **kw) as r:
        r.render(3).wait()  # (leaves a group in progress behind)
        r.reset()
        assert r.counters()["passes"] == 0
        got = r.render(PASSES).radiance().copy()
        assert r.counters()["passes"] == PASSES
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("first", ["base-first", "twin-first"])
def test_a_fixed_handle_and_a_simple_handle_alive_together(pair, first):
    """both kernels' handles in one process, created and rendered in either order, their launches interleaved"""
    base, twin, _ = pair
    W, H = FRAMES[0]
    kw = dict(spp=S, seed=SEED, exact=True, flags=NOSPLIT)
    with HipRenderer(twin, W, H, **kw) as r:
        want = r.render(PASSES).radiance().copy()
    order = [base, twin] if first == "base-first" else [twin, base]
    handles = [HipRenderer(sc, W, H, **kw) for sc in order]
    try:
        for cut in (2, 3):
            for h in handles:
                h.render(cut)
        for h in reversed(handles):
            assert np.array_equal(bits(h.radiance()), bits(want)), (first, h.scene.name)
    finally:
        for h in handles:
            h.close()


def test_the_base_against_the_oracle(pair):
    """STRICT equals the oracle and EXACT -- the fixed instance -- stays within its stated tolerance of it (include/kajo_hip.h
    KAJO_EXACT_REL_TOL), on the base at 64x16: this file's own plumbing, no new tolerance"""
    from exact_tol import assert_exact_within_tolerance
    from oraclelib import OracleLib
    base, _, _ = pair
    W, H = FRAMES[0]
    want = OracleLib("oracle").create(base, 1).render(W, H, S=S, passes=PASSES, seed=SEED, depth_limit=8)
    with HipRenderer(base, W, H, spp=S, seed=SEED, strict=True, flags=NOSPLIT) as r:
        got = r.render(PASSES).radiance().copy()
    assert np.array_equal(bits(got[..., :3]), bits(want[..., :3]))
    with HipRenderer(base, W, H, spp=S, seed=SEED, exact=True, flags=NOSPLIT) as r:
        got = r.render(PASSES).radiance().copy()
    print(assert_exact_within_tolerance(got, want, PASSES, "spheres_a169, the fixed instance"))


# ---- the family of 6 + 5 scenes (tests/fixed_instance_scenes.py family) -----------------------------------------------------------------
# spheres_a169 is ONE shape of scene: the light the last sphere record, the glass the first, one wall order, spheres apart, the camera
# outside everything. A walk written out with literal hit ids and record reads at constant offsets differs from the counted loop in which id
# a hit gets, which record the light's shadow test compares against, which object a ray that is not a number ends on (the last) and which of
# two equal distances wins (the later): the family moves each of these. Every member runs kajo_render_exact_p6s5 and its twin -- the far
# sphere put in front of the LAST record, so that the last object is the member's own -- kajo_render_exact_simple; that, and that the
# oracle renders both alike, tests/test_fixed_kernel_cpu.py holds for every member (the oracle's part is asserted again here, on the
# frames used). (Measured on a copy of the tree whose fixed sphere walk visited its records last to first -- the same candidates, another
# winner among equal distances: every case of this file from before passed; of the cases below those of `coincident` failed.)
from fixed_instance_scenes import NAMES, family as _family

FAMILY_FRAMES = [(64, 16), (72, 40)]  # FRAMES' one block row, and its several blocks with a ragged height
family_frames = pytest.mark.parametrize("size", FAMILY_FRAMES, ids=["%dx%d" % f for f in FAMILY_FRAMES])
members = pytest.mark.parametrize("name", NAMES)


@pytest.fixture(scope="module")
def fam(scenes):
    """get(name, size) -> (member, twin, ids, the oracle's frame of the member): built and rendered once per member and size, shared and
    left unchanged"""
    from oraclelib import OracleLib, available
    if not available("oracle"):
        pytest.skip("oracle not built")
    lib = OracleLib("oracle")
    built = _family(scenes)
    cache = {}

    def get(name, size):
        if (name, size) not in cache:
            sc = built[name]
            twin, ids = far_sphere_twin(sc, before_last=True)
            assert sc.n_lights == twin.n_lights == 1 and (sc.n_planes, sc.n_spheres, twin.n_planes, twin.n_spheres) == (6, 5, 6, 6)
            w, h = size
            a = lib.create(sc, 1).render(w, h, S=S, passes=PASSES, seed=SEED)
            b = lib.create(twin, 1).render(w, h, S=S, passes=PASSES, seed=SEED)
            assert (((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)))).all(), "%s: the oracle's frames of member and twin differ at %dx%d" % (name, w, h)
            a.setflags(write=False)
            cache[name, size] = sc, twin, ids, a
        return cache[name, size]

    return get


def same_bits(a, b):
    """(H, W) bool: every word of the pixel the same, or not a number in both"""
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all(-1)


@members
@family_frames
def test_family_member_against_twin(fam, name, size):
    """radiance(), counters() and every plane of digest(): the instance's, on the member, are the simple kernel's, on the twin"""
    sc, twin, _, _ = fam(name, size)
    W, H = size

    def run(s):
        with HipRenderer(s, W, H, spp=S, seed=SEED, exact=True, flags=NOSPLIT, counters=True) as r:
            r.render(PASSES).wait()
            return r.radiance().copy(), r.counters(), r.digest()
    a, ca, da = run(sc)
    b, cb, db = run(twin)
    assert ca["passes"] == PASSES and ca["paths"] == PASSES * S * W * H and ca["vertices"] > 0
    assert np.array_equal(bits(a), bits(b)), (name, np.argwhere((bits(a) != bits(b)).any(-1))[:4].tolist())
    for k in ("paths", "traversals", "vertices", "passes"):
        assert ca[k] == cb[k], (name, k, ca[k], cb[k])
    assert set(da) >= {"SUM", "COUNTERS"} and da == db, (name, da, db)


@pytest.mark.parametrize("specular", [False, True], ids=["first-hit", "specular-following"])
@members
def test_family_raw_aovs_and_matte_tables(fam, name, specular):
    """the raw AOV sums bit for bit, and the matte tables through the twin's id map (the member's last sphere is one id up in the twin)"""
    size = FAMILY_FRAMES[1]
    sc, twin, ids, _ = fam(name, size)
    W, H = size

    def run(s):
        with HipRenderer(s, W, H, spp=S, seed=SEED, exact=True, flags=NOSPLIT, aov=True, aov_specular=specular, matte=True) as r:
            r.render(PASSES).wait()
            aov, matte = r.aov(), r.matte()
            return aov["raw"], aov["samples"], matte, r.radiance().copy()
    (A, B), n, m, f = run(sc)
    assert n > 0 and A[..., 3].max() > 0 and (m["ids"] > 0).any()
    (A2, B2), n2, m2, f2 = run(twin)
    assert n2 == n and np.array_equal(bits(f), bits(f2))
    assert np.array_equal(bits(A), bits(A2)) and np.array_equal(bits(B), bits(B2))
    assert ids[11] == 12 and not (m2["ids"] == 11).any()  # no sample sees the far sphere
    mapped = np.where(m["ids"] >= 0, ids[np.maximum(m["ids"], 0)], -1)
    assert np.array_equal(mapped, m2["ids"]) and np.array_equal(m["counts"], m2["counts"])


@members
@family_frames
def test_family_strict_is_the_oracle_and_exact_within_its_tolerance(fam, name, size):
    """STRICT on the member is the oracle bit for bit, not a number on the same pixels; EXACT -- the instance -- has the same pixels not
    finite and is elsewhere within its stated tolerance (include/kajo_hip.h KAJO_EXACT_REL_TOL through tests/exact_tol.py: no new number)"""
    from exact_tol import assert_exact_within_tolerance
    sc, _, _, want = fam(name, size)
    W, H = size
    nan_w = ~np.isfinite(want[..., :3]).all(-1)
    with HipRenderer(sc, W, H, spp=S, seed=SEED, strict=True, flags=NOSPLIT) as r:
        got = r.render(PASSES).radiance().copy()
    same = same_bits(got[..., :3], want[..., :3])
    assert same.all(), "%s: %d of %d pixels differ, first at %s" % (name, int((~same).sum()), same.size, np.argwhere(~same)[:4].tolist())
    assert np.array_equal(~np.isfinite(got[..., :3]).all(-1), nan_w) and np.array_equal(np.isnan(got[..., :3]), np.isnan(want[..., :3]))
    with HipRenderer(sc, W, H, spp=S, seed=SEED, exact=True, flags=NOSPLIT) as r:
        ex = r.render(PASSES).radiance().copy()
    nan_e = ~np.isfinite(ex[..., :3]).all(-1)
    assert np.array_equal(nan_e, nan_w), "%s: EXACT has %d not-finite pixels, the oracle %d" % (name, int(nan_e.sum()), int(nan_w.sum()))
    f = assert_exact_within_tolerance(ex, want, PASSES, name)
    print("%s %dx%d: EXACT max rel %.3g, %d not-finite px on both sides" % (name, W, H, f["max_rel"], f["nan_px"]))


@pytest.mark.parametrize("name", ["light_at_0", "nested"])
@family_frames
def test_family_cut_and_resumed_on_one_handle(fam, name, size):
    """5 passes in one render against 2 + 3 on the same handle: the instance's reads of the group's state (the cut falls inside the group of
    passes 1-4) with a light that is not the last record, and with a sphere inside the glass. The digests of every plane the handle keeps
    (no COUNTERS plane: it holds the number of launches) and the frame."""
    sc, _, _, _ = fam(name, size)
    W, H = size

    def run(cuts):
        with HipRenderer(sc, W, H, spp=S, seed=SEED, exact=True, flags=NOSPLIT) as r:
            for c in cuts:
                r.render(c).wait()
            return r.radiance().copy(), r.digest()
    a, da = run((PASSES,))
    b, db = run((2, 3))
    assert "SUM" in da and da == db, (name, da, db)
    assert np.array_equal(bits(a), bits(b))
