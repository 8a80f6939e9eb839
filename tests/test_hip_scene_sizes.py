"""The large-scene kernels from the grid's threshold (48 spheres) up to the LDS limit (9 036 + 4 lights: 160 KiB to the byte), at the
sizes where kajo_hip_create takes another path: tests/scenes_extra.py SIZES, whose plan fields tests/test_scene_sizes_cpu.py pins on the
host -- the grid's cell lists in LDS at steal window 4, 2 and 1 and left in L2 by size, the dynamic-LDS opt-in of the large classes
(launch.inc.hip _set_lds, coldInLds == 0) above 48 and 64 KiB, the grid's clamp to 128 cells per axis, the light loop and the visibility
lists at 17 .. 171 lights, the longest rows of bins, and the refusal one sphere past the limit. The oracle walks every object for every
ray: STRICT must equal it bit for bit through the lists, through the grid alone and through neither."""
import ctypes as C

import numpy as np
import pytest

from exact_tol import assert_exact_within_tolerance
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, stage_info, stage_scene, stage_shadow_lists
from kajo_amd.scene import Scene
from oraclelib import OracleLib, available
from scenes_extra import SIZES, sized_scene

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not available("oracle"), reason="oracle not built")]
SEED, SPP, PASSES, DEPTH = 0o715517, 4, 2, 4
ENTRIES = [name for name in SIZES if name != "too_large"]
# ragged against the 64x16 tiles on both axes; `largest`: the oracle walks 9 046 objects per ray, its frame is the smaller ragged one
FRAME = dict({name: (72, 40) for name in SIZES}, largest=(40, 24))
LISTS_GRID_NONE = (0, capi.KAJO_FLAG_NO_SHADOW_LISTS, capi.KAJO_FLAG_NO_GRID)


def same_words(a, b):
    """the compare of tests/test_hip_fuzz.py: word for word over RGB, NaN == NaN"""
    a, b = a[..., :3], b[..., :3]
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))


class Shared:
    """scenes, oracle frames and the frames of fresh handles: each made once, whichever test asks first, and left unchanged"""

    def __init__(self, scenes):
        self.base = scenes["spheres_a169"]
        self.lib = OracleLib("oracle")
        self._scene, self._want, self._fresh = {"small": self.base}, {}, {}

    def scene(self, name):
        if name not in self._scene:
            self._scene[name] = sized_scene(self.base, name)
        return self._scene[name]

    def frame(self, name):
        return FRAME.get(name, (72, 40))

    def want(self, name):
        if name not in self._want:
            W, H = self.frame(name)
            self._want[name] = self.lib.create(self.scene(name), 1).render(W, H, S=SPP, passes=PASSES, seed=SEED, depth_limit=DEPTH, threads=8)
            self._want[name].setflags(write=False)
        return self._want[name]

    def handle(self, name, build, flags=0, **kw):
        W, H = self.frame(name)
        return HipRenderer(self.scene(name), W, H, spp=SPP, depth_limit=DEPTH, seed=SEED, strict=build == "strict", exact=build == "exact", flags=flags, **kw)

    def fresh(self, name, build, flags=0):
        key = (name, build, flags)
        if key not in self._fresh:
            with self.handle(name, build, flags) as r:
                self._fresh[key] = r.render(PASSES).radiance()
            self._fresh[key].setflags(write=False)
        return self._fresh[key]


@pytest.fixture(scope="module")
def shared(scenes):
    return Shared(scenes)


@pytest.mark.parametrize("name", ENTRIES)
def test_strict_equals_the_every_object_oracle(shared, name):
    want = shared.want(name)
    for flags in LISTS_GRID_NONE:
        same = same_words(shared.fresh(name, "strict", flags), want)
        assert same.all(), (name, flags, int((~same).sum()))


@pytest.mark.parametrize("name", ENTRIES)
def test_exact_through_lists_and_grid(shared, name):
    want = shared.want(name)
    a, b = (shared.fresh(name, "exact", flags) for flags in LISTS_GRID_NONE[:2])
    assert same_words(a, b).all(), name
    assert np.array_equal(np.isfinite(a[..., :3]).all(-1), np.isfinite(want[..., :3]).all(-1)), name
    f = assert_exact_within_tolerance(a, want, PASSES, name)
    print(name, f)


@pytest.mark.parametrize("name", ENTRIES)
def test_fast_through_lists_and_grid(shared, name):
    a, b = (shared.fresh(name, "fast", flags) for flags in LISTS_GRID_NONE[:2])
    same = ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    assert same.all(), (name, int((~same).sum()))


def seeded_rays(sc, n, seed):
    """half from inside the room in random directions, half from the camera through the sphere cloud"""
    rng = np.random.default_rng(seed)
    half = n // 2
    o1 = np.stack([rng.uniform(-7.5, 9.5, half), rng.uniform(-1.9, .9, half), rng.uniform(-1.9, 5.9, half)], 1)
    d1 = rng.normal(size=(half, 3))
    eye = stage_scene(sc)[1][3].astype(np.float64)
    c, r = sc.spheres[:, 12:15].astype(np.float64), sc.spheres[:, 38].astype(np.float64)
    k = rng.integers(0, len(c), n - half)
    target = c[k] + rng.normal(size=(n - half, 3)) * r[k, None]  # through the sphere, past its rim, or just by it
    o2 = np.broadcast_to(eye, target.shape)
    d2 = target - o2
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("name", ENTRIES)
def test_kat_trace_equals_the_oracle(shared, name):
    sc = shared.scene(name)
    o, d = seeded_rays(sc, 4096, 20261019)
    want = shared.lib.create(sc, 1).trace(o, d)
    with HipRenderer(sc, 8, 8, strict=True) as r:
        got = r.kat_trace(o, d)
    assert np.array_equal(got["idx"], want["idx"]), (name, np.nonzero(got["idx"] != want["idx"])[0][:8])
    assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32)), name
    assert (want["idx"][2048:] > sc.n_planes).mean() > 0.25  # the camera's half does meet the cloud


@pytest.mark.parametrize("name,cls", [("window1", "biglist_lg"), ("grid_in_l2", "biglist"), ("largest", "biglist")])
def test_aov_and_matte_of_the_pinned_class(shared, name, cls):
    """(the class: tests/test_scene_sizes_cpu.py -- lists on, cell lists in LDS at window1, in L2 at the other two)"""
    got = []
    for flags in (0, capi.KAJO_FLAG_NO_GRID):
        with shared.handle(name, "strict", flags, aov=True, matte=True) as r:
            if flags == 0:
                assert r.aov_kernel() == "kajo_aov_strict_matte_" + cls, r.aov_kernel()
            r.render(PASSES)
            a, m = r.aov(), r.matte()
            got.append((a["raw"][0], a["raw"][1], m["ids"], m["counts"], a["samples"], m["samples"]))
    for x, y in zip(*got):  # (float sums word for word)
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) if x.dtype == np.float32 else np.array_equal(x, y), name
    assert got[0][4] == got[0][5] > 0 and (got[0][0][..., 3] > 0).any()


def test_lds_opt_in_survives_smaller_and_larger_handles(shared):
    """launch.inc.hip _set_lds: the opt-in is state of the function on the device, only ever raised. A small handle, one above 64 KiB, one
    below 48 KiB, the largest there is and a small one again, all alive together: every one renders the frame a fresh handle gives (STRICT:
    the oracle's as well)."""
    order = ["small", "over64k", "window2", "largest", "small"]
    for build in ("strict", "exact"):
        live, frames = [], []
        try:
            for name in order:
                live.append(shared.handle(name, build))
                frames.append(live[-1].render(PASSES).radiance())
            # once more from the first handles, now that larger and smaller ones have come after them
            again = []
            for r in live:
                r.reset()
                again.append(r.render(PASSES).radiance())
        finally:
            for r in live:
                r.close()
        for name, f, g in zip(order, frames, again):
            assert same_words(f, shared.fresh(name, build)).all(), (build, name)
            assert same_words(g, shared.fresh(name, build)).all(), (build, name, "second render")
            if build == "strict":
                assert same_words(f, shared.want(name)).all(), (build, name)


def test_a_scene_that_does_not_fit_is_refused_cleanly(shared):
    """One sphere past `largest`: KAJO_E_INVALID with the LDS message, after the uploads, which must all be released (hipMalloc is not
    torch's allocator: free device memory from hipMemGetInfo, which libkajo_hip.so's own HIP runtime answers)."""
    sc = shared.scene("too_large")

    def refused(build):
        with pytest.raises(capi.KajoError) as e:
            shared.handle("too_large", build)
        assert e.value.code == capi.KAJO_E_INVALID and "LDS staging limit" in str(e.value), str(e.value)

    for build in ("fast", "strict", "exact"):
        refused(build)
    hip_mem_get_info = capi.lib().hipMemGetInfo  # (resolved through the library's dependency on the HIP runtime)
    hip_mem_get_info.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        free, total = C.c_size_t(), C.c_size_t()
        assert hip_mem_get_info(C.byref(free), C.byref(total)) == 0
        return free.value

    before = free_bytes()
    for k in range(10):
        refused(("fast", "strict", "exact")[k % 3])
    after = free_bytes()
    # one upload of the scene (capi.cpp kajo_hip_create): the records -- hot 16, offset 4, cold 64, material <= 128 bytes per sphere --, the
    # grid (a cell start per cell, <= 4 cells per sphere, 2 bytes per item, <= 8 items per sphere) and the visibility lists: 4 bytes per
    # item, 16-bit offsets [nL * 6 * N * (N + 1)], row bases [nL * 6 * N]
    lists = stage_shadow_lists(sc)
    n, nl, N = sc.n_spheres, sc.n_lights, lists["n"]
    one_upload = n * (16 + 4 + 64 + 128) + n * (4 * 4 + 8 * 2) + 4 * lists["key"].size + 2 * nl * 6 * N * (N + 1) + 4 * nl * 6 * N
    print("free before %d after %d: fell by %d; one upload %d" % (before, after, before - after, one_upload))
    assert before - after <= one_upload, (before - after, one_upload)
    with shared.handle("small", "strict") as r:
        got = r.render(PASSES).radiance()
    assert same_words(got, shared.want("small")).all()


def test_needle_far_origins(shared):
    """The needle without the ceiling (the plane y = -2: tests/test_hip_open_scenes.py drops planes the same way): an open scene, no
    visibility lists, and origins beyond the grid's reach take their wave to the every-sphere loop (integrator.inc.hip trace(): `far`)."""
    full = shared.scene("needle")
    keep = [i for i in range(full.n_planes) if i != ceiling_plane(full)]
    sc = Scene(full.background, full.view, full.proj, full.spheres, full.planes[keep], "needle_open")
    info = stage_info(sc)
    assert info["grid"] and not info["closed_room"] and not info["shadow_lists"] and info["grid_reach"] > 0
    reach, centre = info["grid_reach"], info["grid_center"].astype(np.float64)
    rng = np.random.default_rng(128)
    c, rad = sc.spheres[:, 12:15].astype(np.float64), sc.spheres[:, 38].astype(np.float64)
    O, D = [], []
    for dist in (0.5 * reach, 0.95 * reach, 1.05 * reach, 2 * reach, 300.0, 3000.0):
        u = rng.normal(size=(300, 3)) * (.3, 1, .3)
        u[:150, 1] = -np.abs(u[:150, 1])  # half of them from above, where the ceiling was: nothing but the lights in the way
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = centre + u * dist
        k = rng.integers(0, len(c), 300)
        d = c[k] + rng.normal(size=(300, 3)) * .5 * rad[k, None] - o
        O.append(o)
        D.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    # ... and along the needle from beyond its ends: the walk with the most cells to step through
    for x in (-2 * reach, 2 * reach):
        o = np.tile(np.array([centre[0] + x, centre[1], centre[2]]), (100, 1))
        k = rng.integers(0, len(c), 100)
        d = c[k] + rng.normal(size=(100, 3)) * rad[k, None] - o
        O.append(o)
        D.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    o, d = np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32)
    want = shared.lib.create(sc, 1).trace(o, d)
    for flags in (0, capi.KAJO_FLAG_NO_GRID):
        with HipRenderer(sc, 8, 8, strict=True, flags=flags) as r:
            got = r.kat_trace(o, d)
        assert np.array_equal(got["idx"], want["idx"]), (flags, np.nonzero(got["idx"] != want["idx"])[0][:8])
        assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32)), flags
    assert (want["idx"] > sc.n_planes).sum() >= 100  # (the construction does reach the needle)
    # whole paths in the open needle: through the grid and without it, the oracle's frame
    W, H = 72, 40
    frame = shared.lib.create(sc, 1).render(W, H, S=SPP, passes=PASSES, seed=SEED, depth_limit=DEPTH, threads=8)
    for flags in (0, capi.KAJO_FLAG_NO_GRID):
        with HipRenderer(sc, W, H, spp=SPP, depth_limit=DEPTH, seed=SEED, strict=True, flags=flags) as r:
            got = r.render(PASSES).radiance()
        same = same_words(got, frame)
        assert same.all(), (flags, int((~same).sum()))


def ceiling_plane(sc):
    """the plane whose points have y = -2 (world is Y-down): the one right above the lights"""
    hits = []
    for i in range(sc.n_planes):
        M = sc.planes[i, :16].reshape(4, 4).T  # column-major image
        normal, point = M[:3, 1], M[:3, 3]
        if abs(abs(normal[1]) - 1) < 1e-5 and abs(point[1] + 2) < 1e-5:
            hits.append(i)
    assert len(hits) == 1, hits
    return hits[0]
