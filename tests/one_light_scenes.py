"""One-light small scenes for the EXACT build's two one-light kernels (kajo_amd/csrc/launch.inc.hip): kajo_render_exact_simple takes the scenes
of rigid planes and (centre, radius) spheres (StagedScene allTranslated = planesRigid = 1), kajo_render_exact every other one. Not fixtures: built
where they are used (tests/test_one_light_routing_cpu.py pins which kernel each builder's scene runs; tests/test_hip_simple_instance.py and
tests/test_hip_one_light_general.py render them). Every builder returns a scene of exactly ONE light and fewer than 48 spheres (no grid: the
whole scene is staged in LDS) -- but lds_opt_in_scene, which is a small scene only under KAJO_FLAG_NO_GRID.

The `*_twin` builders add records NO ray meets: the twin's image is the base's, but its staging sends it to the other kernel. They return
(scene, ids): ids[old object id] = new object id, for whatever carries object ids (0 the background, then the planes, then the spheres)."""
import numpy as np

from kajo_amd.scene import Scene, material, plane_record, sphere_record
from scenes_extra import rotation

GRID_THRESHOLD = 48  # kajo_amd/csrc/stage.cpp buildGrid through kajo_hip_create: scenes of fewer spheres have no grid


def _ids(base):
    return np.arange(1 + base.n_planes + base.n_spheres, dtype=np.int32)


def turned_twin(base):
    """`base` plus a dark sphere far outside the room under a rotation about y: a general record no ray can reach (allTranslated = 0). It is put
    in front of the LAST sphere record, which stays the last: in STRICT and EXACT a ray that is not a number "hits" the last object
    (integrator.inc.hip trace), and that must be the object it was in `base`."""
    assert base.n_spheres >= 1
    c, s = np.float32(np.cos(0.3)), np.float32(np.sin(0.3))
    M = np.eye(4, dtype=np.float32)
    M[0, 0], M[0, 2], M[2, 0], M[2, 2] = c, s, -s, c
    M[:3, 3] = (0.0, 500.0, 0.0)  # (the world is y-down: far below the floor plane)
    rec = sphere_record(M.T.reshape(16).copy(), material(diffuse=[0.5, 0.5, 0.5]), 0.25)
    n = base.n_spheres
    spheres = np.concatenate([base.spheres[:n - 1], rec[None], base.spheres[n - 1:]])
    ids = _ids(base)
    ids[base.n_planes + n] += 1  # the last sphere moved one up
    return Scene(base.background, base.view, base.proj, spheres, base.planes, base.name + "+turned"), ids


def scaled_plane_twin(base):
    """`base` plus one plane parallel to the room's first plane, 50 units behind it (seen from the camera) and of the same orientation, under a
    uniform scale of 2 (determinant 8: planesRigid = 0, allTranslated as it was). In a closed room every ray that meets it has met the first plane
    at a smaller t, and its reported distance is 8 t: it is never the closest, and every real plane goes through the loop of scaled planes. The
    new plane is the last plane: the spheres' ids move one up."""
    P = base.planes[0, :16].reshape(4, 4).T.astype(np.float64)  # (column-major image -> matrix)
    cam = np.linalg.inv(base.view.reshape(4, 4).T.astype(np.float64))[:3, 3]
    normal = P[:3, 1]  # the plane is object-space y = 0: its normal is the matrix's y column
    away = -np.sign(normal @ (cam - P[:3, 3]))  # the side of the plane the camera is not on
    assert away != 0
    M = P.copy()
    M[:3, 3] += away * 50.0 * normal / np.linalg.norm(normal)
    M[:3, :3] *= 2.0
    M = M.astype(np.float32)
    assert np.array_equal(M.astype(np.float64)[:3, :3], 2.0 * P[:3, :3])
    rec = plane_record(M.T.reshape(16).copy(), material(diffuse=[0.5, 0.5, 0.5]))
    ids = _ids(base)
    ids[base.n_planes + 1:] += 1
    return Scene(base.background, base.view, base.proj, base.spheres, np.concatenate([base.planes, rec[None]]), base.name + "+scaled_plane"), ids


def both_twin(base):
    a, ia = turned_twin(base)
    b, ib = scaled_plane_twin(a)
    b.name = base.name + "+turned+scaled_plane"
    return b, ib[ia]


def _planes_the_camera_sees(base):
    """per plane of `base`: is it the first plane some ray of a 33 x 33 lattice over the frame meets (float64, the planes alone)"""
    inv = np.linalg.inv(base.proj.reshape(4, 4).T.astype(np.float64) @ base.view.reshape(4, 4).T.astype(np.float64))
    cam = np.linalg.inv(base.view.reshape(4, 4).T.astype(np.float64))[:3, 3]
    u, v = np.meshgrid(np.linspace(-1, 1, 33), np.linspace(-1, 1, 33))
    far = np.stack([u, v, np.ones_like(u), np.ones_like(u)], -1) @ inv.T
    d = far[..., :3] / far[..., 3:] - cam
    t = np.full((len(base.planes),) + u.shape, np.inf)
    for i, p in enumerate(base.planes):
        row = np.linalg.inv(p[:16].reshape(4, 4).T.astype(np.float64))[1]
        denom, oy = d @ row[:3], row[:3] @ cam + row[3]
        with np.errstate(divide="ignore", invalid="ignore"):
            ti = -oy / denom
        t[i] = np.where(np.isfinite(ti) & (ti >= 0), ti, np.inf)
    first = t.argmin(0)[np.isfinite(t.min(0))]
    return np.isin(np.arange(len(base.planes)), first)


def general_scene(base, seed, planes="rigid"):
    """A one-light scene whose general records ARE hit: the room of `base` with 8 .. 20 rotated spheres, the five material classes of
    scenes_extra.mixed_scene in turn, and ONE rotated emissive sphere under the ceiling, the last record. planes="scaled": every plane of the
    room with its object-space z axis scaled by 8 or by 1/8 about its own origin. The plane is object-space y = 0 and its frame is formed from
    the matrix's y and x columns alone (Raytracer.cpp:90-92), so it is the same plane with the same unit frame, and a power of two leaves row y
    of the inverse -- and so t -- the same numbers exactly; but the determinants are 8 and 0.125, and the reference reports t * determinant
    (Raytracer.cpp:96), which orders planes against spheres and each other and places the hit point. (A UNIFORM scale also scales the normal,
    and nine pixels in ten of the reference's frame are then not a number: nothing to compare.) The planes a camera ray can meet first get 8
    -- the spheres in front of them stay in front -- the others, which only later rays meet, 1/8. The range of the general spheres' object
    ids is general_ids(scene)."""
    assert planes in ("rigid", "scaled")
    rng = np.random.default_rng(seed)
    lin = lambda c: np.float32(c) ** np.float32(2.2)
    col = lambda lo=.1, hi=.9: [lin(rng.uniform(lo, hi)) for _ in range(3)]

    def some_material(k):
        if k == 0:
            return material(diffuse=col())
        if k == 1:
            return material(specular=col(), exponent=float(rng.choice([2, 10, 50, 100, 400])))
        if k == 2:
            return material(specular=col(.5, .9), exponent=0.0)  # ideal reflector
        if k == 3:
            return material(specular=col(.2, .6), transparency=col(.7, 1.0), exponent=float(rng.choice([20, 100])), ior=float(rng.choice([1.1, 1.5, 2.0, 2.4])))
        return material(diffuse=col(.1, .5), specular=col(.1, .5), exponent=float(rng.choice([5, 30])))

    recs = []
    for i in range(int(rng.integers(8, 21))):
        T = np.eye(4)
        T[:3, 3] = (rng.uniform(-4, 8), rng.uniform(-1.2, .4), rng.uniform(-1.5, 4))
        M = (T @ rotation(rng)).astype(np.float32)
        recs.append(sphere_record(M.T.reshape(16).copy(), some_material(i % 5), float(rng.uniform(.5, 1.2))))
    T = np.eye(4)
    T[:3, 3] = (rng.uniform(-2, 5), rng.uniform(-1.8, -1.4), rng.uniform(0, 3))
    M = (T @ rotation(rng)).astype(np.float32)
    recs.append(sphere_record(M.T.reshape(16).copy(), material(emission=[lin(rng.uniform(10, 16))] * 3), float(rng.uniform(.3, .5))))
    pl = base.planes.copy()
    if planes == "scaled":
        seen = _planes_the_camera_sees(base)
        assert seen.any() and not seen.all()  # (both determinants occur)
        for i in range(len(pl)):
            M = pl[i, :16].reshape(4, 4).T.copy()
            M[:3, 2] *= np.float32(8.0 if seen[i] else 0.125)
            pl[i, :16] = M.T.reshape(16)
    assert len(recs) < GRID_THRESHOLD
    return Scene(base.background, base.view, base.proj, np.stack(recs), pl, "general%d_%s" % (seed, planes))


def general_ids(scene):
    """object ids of general_scene's rotated spheres, the light among them: (first, last + 1)"""
    return 1 + scene.n_planes, 1 + scene.n_planes + scene.n_spheres


def lds_opt_in_scene(base):
    """200 translate-only spheres + 1 light (scenes_extra.dense_scene): with KAJO_FLAG_NO_GRID a small scene, staged whole in LDS, whose plan
    (52 992 bytes) is above the 48 KiB from which kajo_hip_create opts the kernels in to more dynamic LDS (tests/test_one_light_routing_cpu.py)"""
    from scenes_extra import dense_scene
    return dense_scene(base, 200, 1, seed=1)
