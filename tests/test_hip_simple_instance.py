"""The EXACT build has two one-light kernels for small scenes (integrator.inc.hip trace SIMPLE; launch.inc.hip picks): kajo_render_exact_simple
(kernel_exact_simple.cpp) for scenes of rigid planes and (centre, radius) spheres, without the loops for general records, and
kajo_render_exact for every other scene. Both must take the oracle's decisions. A (centre, radius) sphere walked by the general loop is,
operation for operation, the record's own arithmetic with a determinant of exactly 1: so the one-light scene with ONE sphere far
outside the room turned -- which no ray meets, but which sends the whole scene to the kernel of general scenes -- must give the simple
kernel's frame bit for bit, at frames of one and of several blocks and in the unsplit kernel too.

The same holds for a scene with one SCALED plane no ray meets first (every real plane then goes through the loop of scaled planes, where
t * det with |det - 1| <= 2^-20 and the second sign test give what the rigid loop gives), and for both together
(tests/one_light_scenes.py; tests/test_one_light_routing_cpu.py pins from the host's staging that each base runs kajo_render_exact_simple and
each twin kajo_render_exact). The suite's AOV, matte, noise, adaptive, pass-cut, tile-owner and reset tests render one-light scenes of the
simple kind only: here the two kernels, as separate code objects with their own register allocation, are held to the same bits in every
one of those readers, with KAJO_FLAG_NO_SPLIT so that it is these two kernels that run. Object ids are compared through the builders'
id maps."""
import numpy as np
import pytest

from framelib import bits
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from adaptive_shape_cases import CASES as SHAPE_CASES, PASSES as ADAPT_PASSES, create_keywords
from one_light_scenes import both_twin, lds_opt_in_scene, scaled_plane_twin, turned_twin

pytestmark = pytest.mark.gpu

SEED = 0o715517
NOSPLIT = capi.KAJO_FLAG_NO_SPLIT
BASES = ["spheres_a169", "spheres_a1"]  # spheres_a1: the golden one-light scene with glass and an ideal-reflector wall under another projection
TWINS = {"turned": turned_twin, "scaled-plane": scaled_plane_twin, "both": both_twin}
FRAMES = [(72, 40), (130, 70)]
frames_and_bases = lambda f: pytest.mark.parametrize("size", FRAMES, ids=["72x40", "130x70"])(pytest.mark.parametrize("base", BASES)(f))


def twins(scenes, base):
    """[(name, twin scene, id map)] of a base scene"""
    assert scenes[base].n_lights == 1
    return [(k,) + f(scenes[base]) for k, f in TWINS.items()]


@pytest.mark.parametrize("shape", [(64, 16, 3), (16, 16, 2), (72, 40, 5)])
def test_the_general_kernel_gives_the_simple_kernels_frame(scenes, shape):
    base = scenes["spheres_a169"]
    assert base.n_lights == 1
    gen, _ = turned_twin(base)
    w, h, passes = shape
    for flags in (0, capi.KAJO_FLAG_NO_SPLIT):
        frames = []
        for sc in (base, gen):
            with HipRenderer(sc, w, h, spp=16, seed=SEED, exact=True, flags=flags, counters=True) as r:
                frames.append((r.render(passes).radiance()[..., :3].copy(), r.counters()))
        (a, ca), (b, cb) = frames
        assert np.isfinite(a).all(-1).mean() > 0.99
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (shape, flags)
        assert (ca["traversals"], ca["vertices"]) == (cb["traversals"], cb["vertices"])


@frames_and_bases
def test_radiance_and_counters(scenes, base, size):
    W, H = size

    def run(sc):
        with HipRenderer(sc, W, H, spp=16, seed=SEED, exact=True, flags=NOSPLIT, counters=True) as r:
            return r.render(5).radiance().copy(), r.counters()
    a, ca = run(scenes[base])
    assert np.isfinite(a[..., :3]).all(-1).mean() > 0.99 and ca["passes"] == 5 and ca["paths"] == 5 * 16 * W * H
    for name, sc, _ in twins(scenes, base):
        b, cb = run(sc)
        assert np.array_equal(bits(a), bits(b)), (name, np.argwhere((bits(a) != bits(b)).any(-1))[:4].tolist())
        for k in ("traversals", "vertices", "paths", "passes"):
            assert ca[k] == cb[k], (name, k, ca[k], cb[k])


@pytest.mark.parametrize("specular", [False, True], ids=["first-hit", "specular-following"])
@frames_and_bases
def test_raw_aovs_and_matte_tables(scenes, base, size, specular):
    """albedo, normal, depth and hit counts as summed (kajo_hip_read_aov's raw pair), first-hit and following mirrors and glass; the matte
    tables with the base's ids sent through the twin's id map (both maps are increasing: the ranking of ties by id stands)"""
    W, H = size

    def run(sc):
        with HipRenderer(sc, W, H, spp=16, seed=SEED, exact=True, flags=NOSPLIT, aov=True, aov_specular=specular, matte=True) as r:
            r.render(3).wait()
            aov, matte = r.aov(), r.matte()
            return aov["raw"], aov["samples"], matte, r.radiance().copy()
    (A, B), n, m, f = run(scenes[base])
    assert n > 0 and A[..., 3].max() > 0 and (m["ids"] > scenes[base].n_planes).any()  # (spheres among the ids: the map is exercised)
    for name, sc, ids in twins(scenes, base):
        (A2, B2), n2, m2, f2 = run(sc)
        assert n2 == n and np.array_equal(bits(f), bits(f2)), name
        assert np.array_equal(bits(A), bits(A2)) and np.array_equal(bits(B), bits(B2)), name
        mapped = np.where(m["ids"] >= 0, ids[np.maximum(m["ids"], 0)], -1)
        assert np.array_equal(mapped, m2["ids"]) and np.array_equal(m["counts"], m2["counts"]), name


@pytest.mark.parametrize("base", BASES)
def test_noise_map_and_adaptive_render(scenes, base):
    """tests/adaptive_shape_cases.py's case spheres-S16-exact-nosplit (41x23, S = 16, 32 passes, the unsplit kernel) on each base and its twins:
    the noise map and the raw moments of a KAJO_FLAG_NOISE handle, then frame, records, pass plane and state of an adaptive handle under
    the base's own median target -- under which some unit retires and some stays active, so the set of retired blocks is compared."""
    from test_hip_adaptive import FLOOR, median_target, run, same_records, twin, unit_slots_of
    case = SHAPE_CASES["spheres-S16-exact-nosplit"]
    (W, H), S, kw = case["size"], case["spp"], create_keywords(case)
    assert kw == dict(exact=True, flags=NOSPLIT)

    def noise_of(sc):
        with HipRenderer(sc, W, H, spp=S, seed=SEED, noise=True, **kw) as r:
            r.render(ADAPT_PASSES).wait()
            return r.noise(), r.noise_moments()
    sc0 = scenes[base]
    n0, m0 = noise_of(sc0)
    assert n0["known"] > 0.99 * W * H
    _, records, _ = twin(sc0, "one-light:" + base, W, H, kw, spp=S)
    slots = unit_slots_of(sc0, W, H, spp=S, **kw)
    target = median_target(records, W, H, slots)
    rule = dict(target=target, floor=FLOOR, allowance=0)
    want = run(sc0, W, H, (ADAPT_PASSES,), 1, rule, spp=S, **kw)
    state = want[3]
    assert target > 0 and 0 < state["activeUnits"] < state["units"] and (want[2] < ADAPT_PASSES).any() and (want[2] == ADAPT_PASSES).any(), state
    for name, sc, _ in twins(scenes, base):
        n1, m1 = noise_of(sc)
        for k in ("mean", "stderr", "relative", "batches", "hist"):
            assert np.array_equal(bits(n0[k]), bits(n1[k])), (name, k)
        assert (n0["known"], n0["unknown"], n0["bad"], n0["quantile_value"]) == (n1["known"], n1["unknown"], n1["bad"], n1["quantile_value"]), name
        assert same_records(m0, m1), name
        got = run(sc, W, H, (ADAPT_PASSES,), 1, rule, spp=S, **kw)
        assert np.array_equal(bits(got[0]), bits(want[0])), name
        assert same_records(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3], (name, got[3], want[3])


@frames_and_bases
def test_render_in_cuts_with_launches_that_end_inside_a_group(scenes, base, size):
    """five passes as calls of 1 + 3 + 1 with at most two passes per launch: launches (1 | 2, 1 | 1) of which three end inside the group of
    passes 1-4 (include/kajo_hip.h kajo_hip_render: the group in progress is carried from launch to launch). One call is the reference."""
    from test_hip_pass_cuts import render_cuts
    W, H = size
    kw = dict(exact=True, flags=NOSPLIT, spp=16)
    want, _ = render_cuts(scenes[base], W, H, (5,), **kw)
    got, _ = render_cuts(scenes[base], W, H, (1, 3, 1), passes_per_launch=2, **kw)
    assert np.array_equal(bits(got), bits(want))
    for name, sc, _ in twins(scenes, base):
        got, _ = render_cuts(sc, W, H, (1, 3, 1), passes_per_launch=2, **kw)
        assert np.array_equal(bits(got), bits(want)), name
        got, _ = render_cuts(sc, W, H, (5,), **kw)
        assert np.array_equal(bits(got), bits(want)), name


@pytest.mark.parametrize("tile", [(8, 32), (64, 16)], ids=["tiles-8x32", "tiles-64x16"])
@frames_and_bases
def test_three_tile_owners_gathered(scenes, base, size, tile):
    from test_hip_pass_cuts import render_cuts
    W, H = size
    kw = dict(exact=True, flags=NOSPLIT, spp=16, tile=tile)
    whole, _ = render_cuts(scenes[base], W, H, (5,), **kw)
    want, _ = render_cuts(scenes[base], W, H, (5,), owners=3, **kw)
    assert np.array_equal(bits(want), bits(whole))
    for name, sc, _ in twins(scenes, base):
        got, _ = render_cuts(sc, W, H, (5,), owners=3, **kw)
        assert np.array_equal(bits(got), bits(want)), name


@frames_and_bases
def test_reset_and_render_again_on_the_same_handle(scenes, base, size):
    W, H = size
    kw = dict(spp=16, seed=SEED, exact=True, flags=NOSPLIT, counters=True)
    with HipRenderer(scenes[base], W, H, **kw) as r:
        want = r.render(5).radiance().copy()
    for name, sc, _ in twins(scenes, base):
        with HipRenderer(sc, W, H, **kw) as r:
            r.render(3).wait()  # (leaves a group in progress behind)
            r.reset()
            assert r.counters()["passes"] == 0
            got = r.render(5).radiance().copy()
            assert r.counters()["passes"] == 5
        assert np.array_equal(bits(got), bits(want)), name


@pytest.mark.parametrize("first", ["base-first", "twin-first"])
@pytest.mark.parametrize("base", BASES)
def test_a_base_handle_and_a_twin_handle_alive_together(scenes, base, first):
    """both kernels' handles in one process, created and rendered in either order, their launches interleaved"""
    W, H = FRAMES[0]
    kw = dict(spp=16, seed=SEED, exact=True, flags=NOSPLIT)
    with HipRenderer(scenes[base], W, H, **kw) as r:
        want = r.render(5).radiance().copy()
    order = [scenes[base], both_twin(scenes[base])[0]]
    if first == "twin-first":
        order.reverse()
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


def test_the_lds_opt_in_of_both_kernels(scenes):
    """A small scene whose LDS plan is above 48 KiB: kajo_hip_create opts the kernels in to more dynamic LDS, through launch.inc.hip's
    _set_lds and, from there, kajo_render_exact_simple_set_lds (kernel_exact_simple.cpp: its own per-device high-water table). 200 spheres +
    1 light with KAJO_FLAG_NO_GRID: 52 992 bytes, four waves per workgroup (tests/test_one_light_routing_cpu.py pins the plan, and that no
    scene staged whole in LDS can pass the 64 KiB default limit itself: the largest plans 57 216 bytes). The twin is created FIRST, so
    that the simple kernel's table is still empty when the base's handle raises it; a smaller handle in between must not lower either.
    Simple kernel == general kernel bit for bit, and both within EXACT's stated tolerance of the oracle where it is built."""
    from exact_tol import assert_exact_within_tolerance
    from oraclelib import OracleLib, available
    base = lds_opt_in_scene(scenes["spheres_a169"])
    W, H = FRAMES[0]
    kw = dict(spp=16, seed=SEED, exact=True, flags=NOSPLIT | capi.KAJO_FLAG_NO_GRID)
    with HipRenderer(turned_twin(base)[0], W, H, **kw) as g, HipRenderer(base, W, H, **kw) as s:
        with HipRenderer(scenes["spheres_a169"], W, H, **kw) as small:
            small.render(1).wait()
        a, b = s.render(3).radiance().copy(), g.render(3).radiance().copy()
    with HipRenderer(base, W, H, **kw) as s:  # (at the high-water mark: nothing to raise)
        again = s.render(3).radiance().copy()
    assert np.isfinite(a[..., :3]).all(-1).mean() > 0.99
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(again))
    if available("oracle"):
        want = OracleLib("oracle").create(base, 1).render(W, H, S=16, passes=3, seed=SEED, depth_limit=8)
        assert_exact_within_tolerance(a, want, 3, "200 spheres + 1 light, no grid")
