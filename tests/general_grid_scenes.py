"""Large scenes (48 spheres and more: kajo_amd/csrc/stage.cpp buildGrid) of spheres that are NOT balls under a pure translation, and still
go through the uniform grid: buildGrid asks that every sphere's float32 determinant is exactly 1 and that the planes are rigid, nothing more.
Quarter turns, shears, diagonal scales of product 1 and float32 rotations whose determinant rounds to 1 all pass. Such a scene has
allTranslated = 0: no visibility lists, the kernels `_big_lg` / `_big` (launch.inc.hip), GENERAL hot records of four words behind
sphereHotOffset, whole-box registration in the grid, hit normals through mat3(M). Not fixtures: built where they are used
(tests/test_general_grid_cpu.py pins what each entry's staging and plan are; tests/test_hip_general_grid.py renders them).

Everything is generated from the room, camera and planes of `spheres_a169` (the world is y-down: floor y = 1, ceiling y = -2, walls x = -8,
x = 10, z = -2, z = 6; the camera at (-6, -0.8, 4)). Every matrix is SEARCHED for: a record enters a scene only if the determinant the
library's own staging forms for it (kajo_amd.renderer.stage_scene, column 16) is exactly 1.f.

The plan lines, as tests/test_general_grid_cpu.py computes them (STRICT build, no flags; FAST and EXACT plan large scenes alike), and the
share of the 72 x 40 frame's pixel-centre camera rays whose first hit in the oracle is a general sphere:
  quarter_turns   44 + 4 lights  ldsTotal   8528  big 1 gridInLds 1 window 4  grid 8x2x4   items   66  general  48  share 0.332
  shears          44 + 4 lights  ldsTotal   8528  big 1 gridInLds 1 window 4  grid 8x2x4   items   64  general  48  share 0.294
  ellipsoids      44 + 4 lights  ldsTotal   8592  big 1 gridInLds 1 window 4  grid 8x2x4   items  102  general  48  share 0.321
  rotations       44 + 4 lights  ldsTotal   8528  big 1 gridInLds 1 window 4  grid 8x2x4   items   66  general  48  share 0.332
  mixed           44 + 4 lights  ldsTotal   8224  big 1 gridInLds 1 window 4  grid 8x2x4   items  109  general  40  share 0.273
  mixed_l2       494 + 4 lights  ldsTotal  46304  big 1 gridInLds 0 window 4  grid 16x5x8  items 2238  general 400  share 0.421
One sphere fewer: the 48-sphere entries get no grid (47 in all: a small scene, staged whole), mixed(493) keeps its cell lists in LDS
(gridInLds 1 at steal window 1, ldsTotal 40 832). rotations(44) drew 60 float32 rotations for its 44 records (seed 1): 16 were turned down,
their staged determinant an ulp off 1."""
import itertools

import numpy as np

from kajo_amd.renderer import stage_scene
from kajo_amd.scene import Scene, material, sphere_record
from scenes_extra import _lattice, rotation

GRID_THRESHOLD = 48  # stage.cpp buildGrid through kajo_hip_create: scenes of fewer spheres have no grid
N_LIGHTS = 4
# name -> (builder's name, n): n + N_LIGHTS spheres in all. 44: the grid's threshold. 494: the smallest n at which the plan of mixed(n)
# reports gridInLds 0 (the cell lists no longer fit LDS beside the hot records: kernel `_big`, not `_big_lg`), found from the host's plan
ENTRIES = {
    "quarter_turns": ("quarter_turns", GRID_THRESHOLD - N_LIGHTS),
    "shears": ("shears", GRID_THRESHOLD - N_LIGHTS),
    "ellipsoids": ("ellipsoids", GRID_THRESHOLD - N_LIGHTS),
    "rotations": ("rotations", GRID_THRESHOLD - N_LIGHTS),
    "mixed": ("mixed", GRID_THRESHOLD - N_LIGHTS),
    "mixed_l2": ("mixed", 494),
}
# what each entry is named for: (gridInLds, kernel class)
CLASS = {name: (1, "big_lg") for name in ENTRIES}
CLASS["mixed_l2"] = (0, "big")

lin = lambda c: np.float32(c) ** np.float32(2.2)


def staged_determinants(spheres):
    """the determinant kajo_hip_create's staging forms for every record of `spheres` (n, 39): stage.cpp determinant(), in float32"""
    spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 39)
    sc = Scene(np.zeros(4, np.float32), np.eye(4, dtype=np.float32).reshape(16), np.eye(4, dtype=np.float32).reshape(16), spheres, np.zeros((0, 38), np.float32))
    return stage_scene(sc)[0][:, 16].copy()


def _record(M3, centre, mat, radius):
    """a sphere record of mat3 `M3` (float32 already) about `centre`; asserted to stage with determinant exactly 1.f"""
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = M3
    M[:3, 3] = centre
    return sphere_record(M.T.reshape(16).copy(), mat, radius)


def quarter_turn_matrices():
    """the 23 signed permutation matrices of determinant +1 other than the identity: the rotation group of the cube"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3), np.float32)
            for r in range(3):
                M[r, perm[r]] = signs[r]
            if np.linalg.det(M.astype(np.float64)) > 0 and not np.array_equal(M, np.eye(3, dtype=np.float32)):
                out.append(M)
    assert len(out) == 23
    return out


def shear_matrices():
    """I + k e_ab: k in {+-0.25, +-0.5, +-1} over the six off-diagonal places"""
    out = []
    for k in (.25, -.25, .5, -.5, 1.0, -1.0):
        for a in range(3):
            for b in range(3):
                if a != b:
                    M = np.eye(3, dtype=np.float32)
                    M[a, b] = k
                    out.append(M)
    assert len(out) == 36
    return out


def ellipsoid_matrices():
    """diagonal scales whose product is exactly 1: (2, .5, 1), (4, .5, .5), (.25, 2, 2) and their permutations ((.5, 2, 1) among them)"""
    out = []
    for base in ((2.0, .5, 1.0), (4.0, .5, .5), (.25, 2.0, 2.0)):
        for s in sorted(set(itertools.permutations(base))):
            out.append(np.diag(np.array(s, np.float32)))
    assert len(out) == 12
    return out


class _Rotations:
    """scenes_extra.rotation(rng) rounded to float32, drawn until the STAGED determinant is exactly 1.f; counts its draws"""

    def __init__(self, rng):
        self.rng, self.draws, self.rejected = rng, 0, []

    def __call__(self):
        while True:
            M = rotation(self.rng)[:3, :3].astype(np.float32)
            self.draws += 1
            if staged_determinants(_record(M, (0, 0, 0), material(), 1.0))[0] == np.float32(1.0):
                return M
            self.rejected.append(M)


def some_material(k, rng):
    """the five material classes of scenes_extra.mixed_scene, in turn (tests/one_light_scenes.py general_scene's)"""
    col = lambda lo=.1, hi=.9: [lin(rng.uniform(lo, hi)) for _ in range(3)]
    k %= 5
    if k == 0:
        return material(diffuse=col())
    if k == 1:
        return material(specular=col(), exponent=float(rng.choice([2, 10, 50, 100, 400])))
    if k == 2:
        return material(specular=col(.5, .9), exponent=0.0)  # ideal reflector
    if k == 3:
        return material(specular=col(.2, .6), transparency=col(.7, 1.0), exponent=float(rng.choice([20, 100])), ior=float(rng.choice([1.1, 1.5, 2.0, 2.4])))
    return material(diffuse=col(.1, .5), specular=col(.1, .5), exponent=float(rng.choice([5, 30])))


def _lattice_points(n, rng, keep_out=()):
    """(centres (n, 3), unit): scenes_extra.dense_scene's jittered lattice over the room's box for n spheres -- centres keep 0.6 of the
    pitch apart; unit = the smallest pitch. keep_out: (centre, distance) pairs no lattice centre may come nearer than."""
    lo, ext = np.array([-3.0, -1.7, -1.5]), np.array([12.0, 2.5, 6.0])
    extra = 0
    while True:
        dims = _lattice(n + extra, ext)
        cells = rng.permutation(int(dims.prod()))
        pts = []
        for cidx in cells:
            idx = np.array([cidx % dims[0], (cidx // dims[0]) % dims[1], cidx // (dims[0] * dims[1])])
            p = lo + (idx + rng.random(3) * .4 + .3) * ext / dims
            if all(np.linalg.norm(p - np.asarray(c)) >= dist for c, dist in keep_out):
                pts.append(p)
            if len(pts) == n:
                return np.array(pts), float((ext / dims).min())
        extra += max(1, n // 8)  # (the keep-out regions took too many cells: a finer lattice)


def _lights(rng):
    """four emissive spheres r = 0.1 under the ceiling on dense_scene's lattice of lights, each under a quarter turn: general records
    (allTranslated = 0 by them alone) that are balls all the same, so that the light sampling (Light.cpp: centre and radius) is a ball's"""
    turns = quarter_turn_matrices()
    lx, lz = _lattice(N_LIGHTS, (11.0, 5.5))
    at = [(-2.5 + 11.0 * (k % lx + .5) / lx, -1.85, -1.0 + 5.5 * (k // lx + .5) / lz) for k in range(N_LIGHTS)]
    return [_record(turns[(5 * k + 3) % 23], p, material(emission=[lin(16.0)] * 3), .1) for k, p in enumerate(at)]


def _scene(base, recs, name):
    spheres = np.stack(recs)
    det = staged_determinants(spheres)
    assert (det == np.float32(1.0)).all(), (name, np.flatnonzero(det != 1.0)[:8])
    return Scene(base.background, base.view, base.proj, spheres, base.planes, name)


def _family(base, n, seed, name, matrices, radius):
    """n spheres on the jittered lattice, record i under matrices(i), radius(i, unit, M) its object-space radius, the five material classes in
    turn; then the four turned lights"""
    rng = np.random.default_rng(seed)
    pts, unit = _lattice_points(n, rng)
    recs = []
    for i, p in enumerate(pts):
        M = matrices(i)
        recs.append(_record(M, p, some_material(i, rng), radius(i, unit, M, rng)))
    return _scene(base, recs + _lights(rng), "%s%d" % (name, n))


def _stretch(M):
    """the largest half-extent of the unit sphere under M along a world axis (stage.cpp sphereBounds: the row norms)"""
    return float(np.sqrt((M.astype(np.float64) ** 2).sum(1)).max())


def quarter_turns(base, n, seed=1):
    """n balls under the 23 quarter turns in turn: radii 0.3 .. 0.45 of the lattice's smallest pitch (centres keep 0.6 of it apart:
    neighbours may touch and overlap, none swallows another's centre)"""
    turns = quarter_turn_matrices()
    return _family(base, n, seed, "quarter_turns", lambda i: turns[i % 23], lambda i, unit, M, rng: unit * (.3 + .15 * rng.random()))


def shears(base, n, seed=1):
    """I + k e_ab: the world-space half-extent along the sheared axis is r sqrt(1 + k^2); r is sized so that the largest half-extent is
    0.3 .. 0.45 of the pitch, as the balls' of quarter_turns: neighbours may touch"""
    mats = shear_matrices()
    return _family(base, n, seed, "shears", lambda i: mats[i % 36], lambda i, unit, M, rng: unit * (.3 + .15 * rng.random()) / _stretch(M))


def ellipsoids(base, n, seed=1):
    """diagonal scales of product 1, up to 4 : 1 / 8 : 1 between the axes. The object-space radius is sized so that the LONG half-axis is
    0.5 .. 0.7 of the pitch (they reach into the neighbours' cells and overlap them), the short ones an eighth of that at the least."""
    mats = ellipsoid_matrices()
    return _family(base, n, seed, "ellipsoids", lambda i: mats[i % 12], lambda i, unit, M, rng: unit * (.5 + .2 * rng.random()) / _stretch(M))


def rotations(base, n, seed=1, report=None):
    """float32 rotations whose staged determinant is exactly 1.f, drawn until it is. report: a dict that receives draws (how many
    rotations were drawn for the n records) and rejected (the float32 matrices turned down: their determinant is 1 -+ an ulp)."""
    rng = np.random.default_rng(seed)
    draw = _Rotations(np.random.default_rng(seed + 1000))
    pts, unit = _lattice_points(n, rng)
    recs = [_record(draw(), p, some_material(i, rng), unit * (.3 + .15 * rng.random())) for i, p in enumerate(pts)]
    print("rotations(%d): %d float32 rotations drawn for %d records" % (n, draw.draws, n))
    if report is not None:
        report.update(draws=draw.draws, rejected=draw.rejected)
    return _scene(base, recs + _lights(rng), "rotations%d" % n)


# mixed()'s constructed records, in front of the lattice's: their indices among the spheres
CUT_BY_FLOOR, LONG_ELLIPSOID, NEST_OUTER, NEST_INNER, TIE_FIRST, TIE_SECOND = range(6)
TIE_CENTRE, TIE_RADIUS = (2.0, -0.5, 3.0), 0.5


def mixed(base, n, seed=1):
    """All four kinds interleaved with plain balls (record i of the lattice: kind i % 5, 4 the plain ball), so that sphereHotOffset mixes
    one-word and four-word records; in front of them six constructed records:
      0  a sheared sphere cut by the floor y = 1 (centre 0.2 above it, half-height 0.5)
      1  an ellipsoid (4, .5, .5) r = 0.75 along x: 6 units long, more than a third of the grid's 12-unit x extent
      2  a glass ellipsoid (2, .5, 1) r = 0.8, and 3 a diffuse ball r = 0.25 nested inside it
      4, 5  two records with IDENTICAL quarter-turn matrices, centre (2, -0.5, 3) and radius 0.5, of different materials: a constructed tie --
            the later object wins (Raytracer.cpp:115). No lattice sphere comes within a unit of their surface: the rays of
            test_the_tie_goes_to_the_later_record start one unit from the centre.
    n counts all of them; then the four turned lights."""
    assert n >= 6 + 5
    rng = np.random.default_rng(seed)
    turns, shear, ell = quarter_turn_matrices(), shear_matrices(), ellipsoid_matrices()
    draw = _Rotations(np.random.default_rng(seed + 1000))
    glass = material(specular=[lin(.3)] * 3, transparency=[lin(.9)] * 3, exponent=100.0, ior=1.5)
    recs = [
        _record(shear[4], (4.0, .8, 2.5), material(diffuse=[lin(.7), lin(.3), lin(.2)]), .5),
        _record(np.diag(np.array([4, .5, .5], np.float32)), (3.0, -.4, 0.0), material(diffuse=[lin(.2), lin(.6), lin(.3)]), .75),
        _record(np.diag(np.array([2, .5, 1], np.float32)), (-1.0, .2, 2.0), glass, .8),
        _record(np.eye(3, dtype=np.float32), (-.9, .2, 2.0), material(diffuse=[lin(.8), lin(.7), lin(.1)]), .25),
        _record(turns[7], TIE_CENTRE, material(diffuse=[lin(.8), lin(.1), lin(.1)]), TIE_RADIUS),
        _record(turns[7], TIE_CENTRE, material(diffuse=[lin(.1), lin(.1), lin(.8)]), TIE_RADIUS),
    ]
    assert abs(recs[NEST_INNER][12] - recs[NEST_OUTER][12]) + .25 < 1.6 and .25 < .4  # the ball inside the ellipsoid's (1.6, .4, .8)
    assert np.array_equal(recs[TIE_FIRST][:16], recs[TIE_SECOND][:16]) and not np.array_equal(recs[TIE_FIRST][16:38], recs[TIE_SECOND][16:38])
    m = n - len(recs)
    reach = lambda unit: .7 * unit  # the largest half-extent of a lattice record, below
    # (the lattice's pitch is not known before its size: sized for the coarsest lattice the call can give, pitch <= 1.5)
    pts, unit = _lattice_points(m, rng, keep_out=[(TIE_CENTRE, TIE_RADIUS + 1.0 + reach(1.5))])
    for i, p in enumerate(pts):
        kind = i % 5
        M = (turns[i % 23], shear[i % 36], ell[i % 12], None, np.eye(3, dtype=np.float32))[kind]
        if M is None:
            M = draw()
        size = (.5 + .2 * rng.random()) if kind == 2 else (.3 + .15 * rng.random())
        recs.append(_record(M, p, some_material(i // 5 + kind, rng), unit * size / _stretch(M)))
    return _scene(base, recs + _lights(rng), "mixed%d" % n)


def nudged(scene, index, M3, name):
    """`scene` with the mat3 of sphere `index` replaced by M3, WITHOUT the condition on its determinant: the twins whose staged determinant is
    an ulp off 1, which must get no grid (tests/test_general_grid_cpu.py)"""
    spheres = scene.spheres.copy()
    M = spheres[index, :16].reshape(4, 4).T.copy()
    M[:3, :3] = np.asarray(M3, np.float32)
    spheres[index, :16] = M.T.reshape(16)
    return Scene(scene.background, scene.view, scene.proj, spheres, scene.planes, name)


def general_mask(scene):
    """per sphere: is its record a GENERAL one (stage.cpp stageScene: anything but a pure translation)"""
    M = scene.spheres[:, :16].reshape(-1, 4, 4)
    eye = np.eye(4, dtype=np.float32)
    return ~np.array([np.array_equal(m[:3], eye[:3]) and m[3, 3] == 1 for m in M])  # (column-major image: rows 0 .. 2 are mat3's columns)


def open_twin(scene):
    """(the same scene without the ceiling plane; ids): an open scene -- far origins go to the every-sphere loop (integrator.inc.hip trace():
    `far`). ids[old object id] = new object id (-1: the ceiling)."""
    from test_hip_scene_sizes import ceiling_plane  # (the plane y = -2, right above the lights)
    k = ceiling_plane(scene)
    keep = [i for i in range(scene.n_planes) if i != k]
    ids = np.arange(1 + scene.n_planes + scene.n_spheres, dtype=np.int32)
    ids[k + 2:] -= 1
    ids[k + 1] = -1
    return Scene(scene.background, scene.view, scene.proj, scene.spheres, scene.planes[keep], scene.name + "_open"), ids


_BUILDERS = dict(quarter_turns=quarter_turns, shears=shears, ellipsoids=ellipsoids, rotations=rotations, mixed=mixed)


def entry(base, name, **changes):
    """the ENTRIES scene `name` (changes: n=..., as the neighbour one sphere down)"""
    builder, n = ENTRIES[name]
    return _BUILDERS[builder](base, changes.pop("n", n), **changes)
