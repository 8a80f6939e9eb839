"""Scenes for the EXACT build's fixed-count kernel instances (kajo_amd/csrc/fixed_counts.h, kernel_exact_fixed.cpp), built where they are used
(tests/test_fixed_kernel_cpu.py pins which kernel each runs; tests/test_hip_fixed_instance.py renders them). A simple one-light scene whose
(planes, spheres) are in the table runs its instance; the same scene with one (centre, radius) sphere more runs kajo_render_exact_simple, the
kernel the instance was stamped from -- and gives the same frame if no ray meets the new sphere.

family() is the set of 6 + 5 scenes the instance is held to its twin on: the golden scenes of these counts all have one shape (the light the
last record, the glass the first, one wall order, spheres apart, the camera outside everything), and a walk written out with literal hit ids
and record reads at constant offsets can be wrong exactly where that shape never looks."""
import numpy as np

from kajo_amd.scene import Scene, material, sphere_record, translate

_EMISSION = slice(16 + 12, 16 + 16)  # the emission colour inside a sphere record (kajo_amd/scene.py)
# family()'s materials_<seed>: the first two seeds, and the first whose oracle frames hold pixels that are not a number at both of the frame
# sizes the tests render (64 x 16, 72 x 40; S = 4, 5 passes): found on the CPU oracle, which is all that chose them
MATERIAL_SEEDS = (1, 2, 19)
# family()'s members, for the tests that are parametrised over them
NAMES = (["light_at_%d" % k for k in range(4)] + ["planes_reversed"] + ["materials_%d" % s for s in MATERIAL_SEEDS] +
         ["nested", "overlapping", "coincident", "touching_floor", "light_in_ceiling", "camera_in_glass", "test_a1", "spheres_a1"])


def far_sphere_twin(base, before_last=False):
    """(`base` plus a dark (centre, radius) sphere far outside the room; ids): a pure translation, so the scene stays one of rigid planes and
    (centre, radius) spheres (allTranslated = 1), with one sphere more than `base`. ids[old object id] = new object id. In a closed room every
    ray meets a wall first, and no ray of the wave reaches the new sphere's line, so the walk skips it as a wave.

    before_last=False: the new record is appended LAST and ids is the identity: nothing in front of it moves. Being the last record it IS what
    a ray that is not a number ends on in STRICT and EXACT (integrator.inc.hip trace) where `base` ends such a ray on its own last sphere: the
    callers check on the oracle that base and twin give one frame before they compare kernels.

    before_last=True: the new record is put in front of the last sphere record, as one_light_scenes.turned_twin puts its own: the last sphere
    of `base` stays the last object, one id up, and a ray that is not a number ends on it in base and twin alike."""
    rec = sphere_record(translate(0.0, 500.0, 0.0), material(diffuse=[0.5, 0.5, 0.5]), 0.25)  # (the world is y-down: far below the floor plane)
    ids = np.arange(1 + base.n_planes + base.n_spheres, dtype=np.int32)
    if not before_last:
        spheres = np.concatenate([base.spheres, rec[None]])
    else:
        n = base.n_spheres
        assert n >= 1
        spheres = np.concatenate([base.spheres[:n - 1], rec[None], base.spheres[n - 1:]])
        ids[base.n_planes + n] += 1  # the last sphere moved one up
    return Scene(base.background, base.view, base.proj, spheres, base.planes, base.name + "+far_sphere"), ids


def without_a_sphere(base):
    """`base` without its first sphere that is not a light: another image, one sphere fewer, still one light"""
    light = (base.spheres[:, 16:38][:, 12:16] != 0).any(1)
    k = int(np.flatnonzero(~light)[0])
    return Scene(base.background, base.view, base.proj, np.delete(base.spheres, k, axis=0), base.planes, base.name + "-sphere%d" % k)


def _with(base, name, spheres=None, planes=None, view=None):
    return Scene(base.background, base.view if view is None else view, base.proj, base.spheres if spheres is None else spheres,
                 base.planes if planes is None else planes, name)


def _materials(base, seed):
    """the room and the sphere positions of `base`; the walls and the spheres that are no light draw from the five classes of
    scenes_extra.mixed_scene's some_material (restated: it is local there), glass over exponent 0 excluded as it is there"""
    rng = np.random.default_rng(seed)
    lin = lambda c: np.float32(c) ** np.float32(2.2)
    col = lambda lo=.1, hi=.9: [lin(rng.uniform(lo, hi)) for _ in range(3)]

    def some_material():
        k = rng.integers(5)
        if k == 0:
            return material(diffuse=col())
        if k == 1:
            return material(specular=col(), exponent=float(rng.choice([2, 10, 50, 100, 400])))
        if k == 2:
            return material(specular=col(.5, .9), exponent=0.0)  # ideal reflector
        if k == 3:  # (glass over an ideal reflector, exponent 0, is NaN over whole regions in the reference: nothing to compare there)
            return material(specular=col(.2, .6), transparency=col(.7, 1.0), exponent=float(rng.choice([20, 100])), ior=float(rng.choice([1.1, 1.5, 2.0, 2.4])))
        return material(diffuse=col(.1, .5), specular=col(.1, .5), exponent=float(rng.choice([5, 30])))

    planes, spheres = base.planes.copy(), base.spheres.copy()
    for i in range(len(planes)):
        planes[i, 16:38] = some_material()
    for i in range(len(spheres)):
        if not (spheres[i, _EMISSION] != 0).any():
            spheres[i, 16:38] = some_material()
    return _with(base, "materials_%d" % seed, spheres, planes)


def radius_touching(cy, coordinate=1.0):
    """(cy', r): the float32 nearest `cy` from above, and a float32 radius, for which cy' + r is `coordinate` EXACTLY -- the sum of the two
    binary32 numbers formed without rounding is the coordinate itself, so it is in every precision --, searched and not assumed (as
    tests/test_hip_kat.py test_trace_origin_exactly_on_a_surface searches its points): the sphere touches the plane y = coordinate in one
    point"""
    cy = np.float32(cy)
    for _ in range(64):
        r = np.float32(np.float64(coordinate) - np.float64(cy))
        if np.float64(cy) + np.float64(r) == np.float64(coordinate) and np.float32(cy + r) == np.float32(coordinate) and r > 0:
            return cy, r
        cy = np.nextafter(cy, np.float32(np.inf))
    raise AssertionError("no float32 radius makes centre + radius the plane's coordinate exactly")


def family(scenes):
    """{name: scene}: every member has exactly 6 planes, 5 (centre, radius) spheres, rigid planes and one light, so every member runs
    kajo_render_exact_p6s5 (tests/test_fixed_kernel_cpu.py asserts it, and that its far_sphere_twin(before_last=True) runs the simple kernel
    and is the same frame in the oracle).

    The room of spheres_a169 (the world is y-down): the floor y = 1 (plane 0), the mirror wall z = -2, the walls x = 10, x = -8, z = 6 and
    the ceiling y = -2 (plane 5); the glass sphere is record 0, the light record 4, the camera at (-6, -0.8, 4)."""
    base = scenes["spheres_a169"]
    assert (base.n_planes, base.n_spheres, base.n_lights) == (6, 5, 1)
    light = int(np.flatnonzero((base.spheres[:, _EMISSION] != 0).any(1))[0])
    others = [i for i in range(base.n_spheres) if i != light]
    assert light == 4 and base.spheres[0, 16 + 16:16 + 19].any()  # the light last, the glass first
    out = {}
    # the emitter as record k, the other records in their order
    for k in range(4):
        out["light_at_%d" % k] = _with(base, "light_at_%d" % k, base.spheres[others[:k] + [light] + others[k:]])
    out["planes_reversed"] = _with(base, "planes_reversed", planes=base.planes[::-1].copy())
    for seed in MATERIAL_SEEDS:
        out["materials_%d" % seed] = _materials(base, seed)
    small = material(diffuse=[.6, .3, .1])
    # a small diffuse sphere wholly inside the glass sphere (centre (-2, 0, 0), radius 1): 0.28 from its centre, radius 0.4
    s = base.spheres.copy()
    s[3] = sphere_record(translate(-2.0, .2, .2), small, .4)
    assert np.linalg.norm(s[3, 12:15] - s[0, 12:15]) + s[3, 38] < s[0, 38]
    out["nested"] = _with(base, "nested", s)
    # record 2 moved until its surface cuts record 1's (centres 1.24 apart, radii 1 and 1)
    s = base.spheres.copy()
    s[2, :16] = translate(2.2, 0.0, .8)
    assert abs(s[1, 38] - s[2, 38]) < np.linalg.norm(s[2, 12:15] - s[1, 12:15]) < s[1, 38] + s[2, 38]
    out["overlapping"] = _with(base, "overlapping", s)
    # record 3 laid over record 1, centre on centre and radius on radius, with its own material: every ray that meets one meets the other at
    # the same distance, and the walk keeps the LATER record of equal distances (integrator.inc.hip trace: `!(th > tMax)`)
    s = base.spheres.copy()
    s[3, :16], s[3, 38] = s[1, :16], s[1, 38]
    assert not np.array_equal(s[3, 16:38], s[1, 16:38])
    out["coincident"] = _with(base, "coincident", s)
    # record 2 smaller and lower, its lowest point ON the floor: centre.y + radius is the floor's y exactly
    floor_y = base.planes[0, 13]
    assert floor_y == 1.0 and np.array_equal(base.planes[0, :16], translate(0, 1, 0))
    cy, r = radius_touching(.3, float(floor_y))
    s = base.spheres.copy()
    s[2, :16] = translate(4.0, cy, 1.0)
    s[2, 38] = r
    assert s[2, 13] + s[2, 38] == floor_y and np.float64(s[2, 13]) + np.float64(s[2, 38]) == np.float64(floor_y) and (cy, r) != (0.0, 1.0)
    out["touching_floor"] = _with(base, "touching_floor", s)
    # the emitter's ball cut by the ceiling y = -2: its centre 0.1 under it, its radius 0.3
    s = base.spheres.copy()
    s[light, :16] = translate(-1.0, -1.9, 2.0)
    assert abs(s[light, 13] - (-2.0)) < s[light, 38]
    out["light_in_ceiling"] = _with(base, "light_in_ceiling", s)
    # the view moved (its rotation kept) until the camera lies inside the glass sphere, 0.37 from its centre
    V = base.view.reshape(4, 4).T.astype(np.float64)
    eye = np.array([-2.3, -.1, .2])
    V[:3, 3] = -V[:3, :3] @ eye
    view = V.T.reshape(16).astype(np.float32)
    at = np.linalg.inv(view.reshape(4, 4).T.astype(np.float64))[:3, 3]
    assert np.linalg.norm(at - base.spheres[0, 12:15]) < .5 * base.spheres[0, 38]
    out["camera_in_glass"] = _with(base, "camera_in_glass", view=view)
    # two golden scenes as they are: another projection (test_a1, whose four spheres also overlap), another aspect (spheres_a1)
    out["test_a1"] = scenes["test_a1"]
    out["spheres_a1"] = scenes["spheres_a1"]
    for name, sc in out.items():
        assert (sc.n_planes, sc.n_spheres, sc.n_lights) == (6, 5, 1), name
    assert list(out) == NAMES
    return out
