"""Seeded scenes generated where they are used (tests/test_hip_whole_frames.py; tools/whole_frame.py, oracle_vs_reference.py): not fixtures."""
import numpy as np
from kajo_amd.scene import Scene


def rotation(rng):
    """a rigid rotation (Rodrigues), as a 4 x 4"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = rng.uniform(0, 2 * np.pi)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R
    return M


def mixed_scene(base, seed):
    from kajo_amd.scene import material, sphere_record, plane_record
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
    planes = base.planes.copy()
    for i in range(len(planes)):
        planes[i, 16:38] = some_material() if rng.random() < .7 else planes[i, 16:38]
    recs = []
    for _ in range(int(rng.integers(8, 21))):
        T = np.eye(4)
        T[:3, 3] = (rng.uniform(-4, 8), rng.uniform(-1.5, .6), rng.uniform(-1.5, 4))
        M = (T @ rotation(rng)).astype(np.float32)
        recs.append(sphere_record(M.T.reshape(16).copy(), some_material(), float(rng.uniform(.2, 1.1))))
    for _ in range(int(rng.integers(1, 5))):
        T = np.eye(4)
        T[:3, 3] = (rng.uniform(-4, 8), rng.uniform(-1.8, -.8), rng.uniform(-1, 4))
        M = (T @ rotation(rng)).astype(np.float32)
        recs.append(sphere_record(M.T.reshape(16).copy(), material(emission=[lin(rng.uniform(6, 16))] * 3), float(rng.uniform(.1, .5))))
    return Scene(base.background, base.view, base.proj, np.stack(recs), planes, "mix%d" % seed)


def _lattice(n, extent):
    """cells per axis of a near-cubic lattice of at least n cells over a box of the given extent"""
    extent = np.asarray(extent, np.float64)
    pitch = (extent.prod() / max(n, 1)) ** (1.0 / extent.size)
    dims = np.maximum(1, np.ceil(extent / pitch - 1e-9).astype(int))
    while dims.prod() < n:
        dims[np.argmax(extent / dims)] += 1
    return dims


def dense_scene(base, n_spheres, n_lights, seed, shape="room"):
    """kajo_amd.scene.stress_scene's recipe for any size: the room of spheres_a169 with `n_spheres` translate-only spheres on a jittered
    lattice sized from their number, radii 0.1 .. 0.25 of the lattice pitch (centres keep 0.6 pitch apart: neighbours may touch, none
    swallows another), materials cycling diffuse / Phong, and `n_lights` emissive spheres r = 0.1 under the ceiling on a lattice that takes
    any count. shape "needle": the spheres in one thin row along x, y and z within a few radii, right under the lights' one row; "cluster":
    the spheres packed into the box of two units around the first light."""
    from kajo_amd.scene import material, sphere_record, translate
    rng = np.random.default_rng(seed)
    lin = lambda c: np.float32(c) ** np.float32(2.2)
    # lights: rows along x under the ceiling (world is Y-down: the ceiling is y = -2)
    lx, lz = (n_lights, 1) if shape == "needle" else _lattice(n_lights, (11.0, 5.5))
    light_at = [(-2.5 + 11.0 * (k % lx + .5) / lx, -1.85, -1.0 + 5.5 * (k // lx + .5) / lz) for k in range(n_lights)]
    if shape == "needle":
        # (the grid's bounds hold the lights too: the row lies just under their one row, so that the bounds stay a needle)
        lo, ext = np.array([-3.0, -1.72, light_at[0][2]]), np.array([12.0, 0.0, 0.0])
        dims = np.array([n_spheres, 1, 1])
    elif shape == "cluster":
        c = np.array(light_at[0])
        lo, ext = np.array([c[0] - 2.0, -1.7, c[2] - 2.0]), np.array([4.0, 2.0, 4.0])
        dims = _lattice(n_spheres, ext)
    else:
        assert shape == "room"
        lo, ext = np.array([-3.0, -1.7, -1.5]), np.array([12.0, 2.5, 6.0])
        dims = _lattice(n_spheres, ext)
    pitch = np.where(ext > 0, ext / dims, np.inf)
    unit = float(pitch.min())
    cells = rng.permutation(int(dims.prod()))[:n_spheres]
    recs = []
    for k, cidx in enumerate(cells):
        idx = np.array([cidx % dims[0], (cidx // dims[0]) % dims[1], cidx // (dims[0] * dims[1])])
        j = rng.random(3) * .4 + .3
        r = unit * (.1 + .15 * rng.random())
        p = lo + np.where(ext > 0, (idx + j) * ext / dims, 0.0)
        if shape == "needle":
            p[1:] += (rng.random(2) * 2 - 1) * 3 * r
        col = [lin(.2 + .6 * rng.random()) for _ in range(3)]
        if k % 2 == 0:
            m = material(diffuse=col)
        else:
            m = material(specular=col, exponent=float(rng.choice([10, 50, 100])))
        recs.append(sphere_record(translate(*p), m, r))
    for p in light_at:
        recs.append(sphere_record(translate(*p), material(emission=[lin(16.0)] * 3), .1))
    return Scene(base.background, base.view, base.proj, np.stack(recs), base.planes, "dense_%s%d_%d" % (shape, n_spheres, n_lights))



# Scene sizes at which create() takes another path (kajo_amd/csrc/launch_plan.h kajoLdsPlan, stage.cpp buildGrid / buildShadowLists):
# name -> dense_scene's arguments behind `base`. tests/test_scene_sizes_cpu.py pins, from the host's own plan, what each entry is named for and
# that its neighbour one sphere down is not there yet; tests/test_hip_scene_sizes.py renders every one. The plan lines, as computed there
# (STRICT build, no flags; FAST and EXACT plan large scenes alike):
#   window4      32 +  16 lights  ldsTotal   7824  gridInLds 1 window 4  grid 8x2x4     bins 64  the grid's threshold: 47 spheres in all get none
#   window2     834 +  16 lights  ldsTotal  34112  gridInLds 1 window 2  grid 20x5x10   bins 64
#   window1    1119 +  16 lights  ldsTotal  36880  gridInLds 1 window 1  grid 22x5x11   bins 64
#   grid_in_l2 1318 +  16 lights  ldsTotal  41840  gridInLds 0 window 4  grid 23x6x12   bins 64  cell lists left in L2 by size
#   over48k    1869 +   4 lights  ldsTotal  49168  gridInLds 0 window 4  grid 26x6x13   bins 64  first launch through the coldInLds == 0 opt-in
#   over64k    2893 +   4 lights  ldsTotal  65552  gridInLds 0 window 4  grid 30x7x15   bins 64
#   largest    9036 +   4 lights  ldsTotal 163840  gridInLds 0 window 4  grid 43x10x22  bins 64  160 KiB to the byte, in all three builds
#   too_large  9037 +   4 lights  ldsTotal 163856  fits 0 in all three builds
#   needle     1000 +   4 lights  ldsTotal  36464  gridInLds 1 window 2  grid 128x4x3   bins 64  139 cells wanted along x (800 spheres: 129)
#   lights17    300 +  17 lights  ldsTotal  28464  gridInLds 1 window 4  grid 15x4x8    bins 64
#   lights33    300 +  33 lights  ldsTotal  30496  gridInLds 1 window 4  grid 15x4x8    bins 64
#   lights64    300 +  64 lights  ldsTotal  34448  gridInLds 1 window 4  grid 15x4x8    bins 64
#   lights171   100 + 171 lights  ldsTotal  35904  gridInLds 1 window 2  grid 14x4x7    bins 32
#   cluster    3000 +   4 lights  ldsTotal  67264  gridInLds 0 window 4  grid 30x7x15   bins 64  longest row of bins 2597 items
SIZES = {
    "window4": dict(n_spheres=32, n_lights=16, seed=1),
    "window2": dict(n_spheres=834, n_lights=16, seed=1),
    "window1": dict(n_spheres=1119, n_lights=16, seed=1),
    "grid_in_l2": dict(n_spheres=1318, n_lights=16, seed=1),
    "over48k": dict(n_spheres=1869, n_lights=4, seed=1),
    "over64k": dict(n_spheres=2893, n_lights=4, seed=1),
    "largest": dict(n_spheres=9036, n_lights=4, seed=1),
    "too_large": dict(n_spheres=9037, n_lights=4, seed=1),
    "needle": dict(n_spheres=1000, n_lights=4, seed=1, shape="needle"),
    "lights17": dict(n_spheres=300, n_lights=17, seed=1),
    "lights33": dict(n_spheres=300, n_lights=33, seed=1),
    "lights64": dict(n_spheres=300, n_lights=64, seed=1),
    "lights171": dict(n_spheres=100, n_lights=171, seed=1),
    "cluster": dict(n_spheres=3000, n_lights=4, seed=1, shape="cluster"),
}


def sized_scene(base, name, **changes):
    """the SIZES entry `name` (changes: arguments to override, as the neighbour one sphere down)"""
    return dense_scene(base, **dict(SIZES[name], **changes))
