"""The noise estimate, adaptive sampling and the noise-guided denoiser at tile shapes other than the default 64x16: the tile-map readers
that came after tests/test_hip_tile_shapes.py -- kajo_noise_map, kajo_adapt_passes and kajo_denoise_guided_v0 through kajoTileSlot,
kajo_adapt_select through kajo::adaptSlotPixel (adapt_math.h), a second copy of the render kernel's slot-to-pixel arithmetic.

The oracle is that module's: a per-pixel output is a function of scene, parameters and pass count, not of the tile shape, so the
default-tile handle is the reference word for word, with no tolerance. (The default tile is what tests/test_hip_noise.py,
test_hip_adaptive.py and test_hip_denoise_guided.py hold to their numpy restatements.) One case is different: an adaptive handle whose
unit is 256 slots (a scene whose workgroups are four waves) retires four consecutive pixel blocks OF A TILE together, so which pixels share a unit -- and with it the frame --
depends on the tile shape by definition. There the reference is test_hip_adaptive.py's restatement with the layout of tile T, fed with
the records of the default-tile twin.

Frame 100x75: ragged on both axes for every shape of TILES. The host half of kajo::adaptSlotPixel is held to kajoTileSlot's exact inverse
in tests/test_adaptive_cpu.py, without a GPU."""
import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, NOISE_MOMENTS, noise_evaluate
from kajo_amd.tiles import TileLayout
from scenes_extra import dense_scene
from test_hip_adaptive import FLOOR, PASSES, expected, median_target, rel32, restate, run, same_records, twin, unit_of, unit_slots_of
from test_hip_tile_shapes import DEFAULT, SEED, TILES, H, W, bits, plant, same, tile_id

pytestmark = pytest.mark.gpu

BUILDS = {"strict": dict(strict=True), "exact": dict(exact=True), "fast": dict()}
OWNED_BY_THREE = [(24, 32), (40, 32), (128, 64)]  # (at 128x64 the frame is two tiles: the third owner owns nothing)
NAN_AT = (95, 71)  # in the ragged last tile of every shape
NAN_MARK = [(NAN_AT, (np.nan, np.nan, np.nan))]
PLANES = ("mean", "stderr", "relative", "batches")


def words(rec):
    """a record array as its four planes of 64-bit words"""
    return {k: np.ascontiguousarray(rec[k]).view(np.uint64) for k in ("s1", "s2", "n", "bad")}


# ---- the noise estimate ---------------------------------------------------------------------------------------------------------------

def _estimate(parts):
    """records, planes, histogram and counts of the owners of one frame: records and planes merged through out=, histograms added"""
    rec = np.zeros((H, W), NOISE_MOMENTS)
    rec["n"] = 99  # (every pixel has one owner: nothing of this is left)
    planes, hist, counts = None, np.zeros(capi.KAJO_NOISE_HIST_WORDS, np.uint64), np.zeros(4, np.int64)
    for p in parts:
        p.noise_moments(out=rec)
        planes = p.noise(floor=FLOOR, quantile=0.95, out=planes)
        hist += planes["hist"]
        counts += [planes[k] for k in ("pixels", "known", "unknown", "bad")]
    out = dict(words(rec), hist=hist, counts=counts, quantile_value=noise_evaluate(hist.astype(np.uint32), 0.95))
    if len(parts) == 1:
        assert bits(np.float32(planes["quantile_value"])) == bits(np.float32(out["quantile_value"]))
    out.update({k: planes[k].copy() for k in PLANES})
    return out


def _noise(sc, tile, owners, build):
    """-> the estimate after 16 passes, and after a NaN written into the accumulation at NAN_AT and four passes more"""
    parts = [HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, tile=tile, tile_index=k, tile_count=owners, **BUILDS[build])
             for k in range(owners)]
    try:
        for p in parts:
            p.render(16)
        clean = _estimate(parts)
        plant(parts, TileLayout(W, H, owners, tile=tile), NAN_MARK)
        for p in parts:
            p.render(4)
        return clean, _estimate(parts)
    finally:
        for p in parts:
            p.close()


@pytest.fixture(scope="module")
def noise_reference(scenes):
    """build -> the default-tile, one-owner handle's estimate at 16 passes, at 20 passes with the NaN planted at 16, and its records at 20
    passes with nothing planted"""
    cache = {}

    def get(build):
        if build not in cache:
            sc = scenes["spheres_a169"]
            clean, marked = _noise(sc, DEFAULT, 1, build)
            with HipRenderer(sc, W, H, spp=4, seed=SEED, noise=True, **BUILDS[build]) as r:
                unmarked = words(r.render(20).noise_moments())
            assert (clean["n"] + clean["bad"] == 4).all() and (clean["n"] == 4).mean() > 0.99
            assert tuple(clean["counts"]) == (W * H, W * H, 0, int((clean["bad"] > 0).sum())) and clean["quantile_value"] > 0
            x, y = NAN_AT
            assert clean["bad"][y, x] == 0  # (the pixel is clean until it is marked)
            for k in list(clean) + list(marked):
                for d in (clean, marked):
                    if isinstance(d[k], np.ndarray):
                        d[k].setflags(write=False)
            cache[build] = (clean, marked, unmarked)
        return cache[build]

    return get


def _check_noise(got, want, unmarked, why):
    clean, marked = got
    for name, g, w in (("at 16 passes", clean, want[0]), ("with the NaN", marked, want[1])):
        for k in w:
            assert same(g[k], w[k]), (why, name, k, np.argwhere(np.asarray(g[k] != w[k]))[:4])
    # bad marks the planted pixel and no other: every other pixel's record is that of a handle nothing was written into
    x, y = NAN_AT
    others = np.ones((H, W), bool)
    others[y, x] = False
    for k in ("s1", "s2", "n", "bad"):
        assert np.array_equal(marked[k][others], unmarked[k][others]), (why, k)
    assert (marked["bad"][y, x], marked["n"][y, x]) == (1, 4), why
    assert all(marked[k][y, x] == clean[k][y, x] for k in ("s1", "s2", "n")), why  # (the pixel keeps the four batches it had)
    assert marked["counts"][3] == clean["counts"][3] + 1 and marked["hist"][-1] == clean["hist"][-1] + 1, why


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("tile", TILES, ids=tile_id)
def test_noise_records_planes_and_histogram_are_the_default_tiles(scenes, noise_reference, tile, build):
    """noise_moments(), the four planes of noise(), its 516-word histogram, known / unknown / bad and the quantile: one owner at every
    shape, three owners at 24x32, 40x32 and 128x64, 16 passes; then a NaN in the tile buffer at (95, 71) and a fifth batch."""
    want = noise_reference(build)
    for owners in (1, 3) if tile in OWNED_BY_THREE else (1,):
        _check_noise(_noise(scenes["spheres_a169"], tile, owners, build), want, want[2], (tile, build, owners))
    if tile == (128, 64):
        lay = TileLayout(W, H, 3, tile)
        assert lay.n_tiles == 2 and lay.owned_pixels(2) == 0


# ---- adaptive sampling, a unit of 64 slots: one pixel block, whatever the tile ------------------------------------------------------------

@pytest.fixture(scope="module")
def adaptive_reference(scenes):
    """build -> (the rule, the default-tile adaptive handle's frame, records, pass plane and state after 32 passes)"""
    cache = {}

    def get(build):
        if build not in cache:
            sc = scenes["spheres_a169"]
            kw = dict(BUILDS[build], flags=0)
            _, records, _ = twin(sc, "spheres", W, H, kw)
            assert unit_slots_of(sc, W, H, **kw) == 64
            rule = dict(target=median_target(records, W, H, 64), floor=FLOOR, allowance=0)
            want = run(sc, W, H, (PASSES,), 1, rule, **kw)
            s = want[3]
            assert 0 < s["activePixels"] < W * H and s["lastDecisionPass"] == PASSES and (want[2] == 16).any() and (want[2] == PASSES).any(), s
            cache[build] = (rule, want)
        return cache[build]

    return get


@pytest.mark.parametrize("build", ["exact", "fast"])
@pytest.mark.parametrize("tile", TILES, ids=tile_id)
def test_adaptive_units_of_one_pixel_block_do_not_depend_on_the_tile_shape(scenes, adaptive_reference, tile, build):
    """spheres.json: a workgroup is one wave, a unit one 8x8 block aligned to 8 -- the same pixels at every tile shape. Frame, records and
    pass plane word for word, active pixels, traced paths and the last decision's pass: one owner everywhere, three at 24x32 and 128x64."""
    rule, want = adaptive_reference(build)
    sc = scenes["spheres_a169"]
    kw = dict(BUILDS[build], flags=0, tile=tile)
    assert unit_slots_of(sc, W, H, **kw) == 64
    for owners in (1, 3) if tile in ((24, 32), (128, 64)) else (1,):
        got = run(sc, W, H, (PASSES,), owners, rule, **kw)
        why = (tile, build, owners)
        assert np.array_equal(bits(got[0]), bits(want[0])), (why, np.argwhere(bits(got[0]) != bits(want[0]))[:4])
        assert same_records(got[1], want[1]), why
        assert np.array_equal(got[2], want[2]), (why, np.argwhere(got[2] != want[2])[:4])
        for k in ("pixels", "activePixels", "paths", "lastDecisionPass", "unitSlots"):
            assert got[3][k] == want[3][k], (why, k, got[3], want[3])


# ---- adaptive sampling, a unit of 256 slots: four consecutive pixel blocks of a tile ------------------------------------------------------
# Two scenes. "stress30" (30 spheres, two lights; tests/test_hip_pass_cuts.py's four-wave scene) has an LDS copy above 6 KiB, so a workgroup
# is four waves and a unit 256 slots (launch_plan.h wavesPerBlock): the case this section is about, at the default tile as well, which no
# other test of the select kernel's four-wave path reaches. "grid60", test_hip_adaptive.py's large-scene instance, keeps its hot records
# within 6 KiB and runs one-wave workgroups: its unit is 64 slots, the restatement with the layout of tile T is then the default tile's,
# and it is held to it all the same.
UNIT_TILES = [(8, 32), (32, 8), (24, 32), (96, 8)]
UNIT_CASES = [("stress30", t) for t in UNIT_TILES + [DEFAULT]] + [("grid60", t) for t in UNIT_TILES]
UNIT_SLOTS = {"stress30": 256, "grid60": 64}


@pytest.fixture(scope="module")
def unit_scenes(scenes):
    from kajo_amd.scene import stress_scene
    base = scenes["spheres_a169"]
    return {"stress30": stress_scene(base, 30, 2, seed=11), "grid60": dense_scene(base, 60, 3, seed=11)}


@pytest.mark.parametrize("scene,tile", UNIT_CASES, ids=["%s-%s" % (s, tile_id(t)) for s, t in UNIT_CASES])
def test_adaptive_units_of_four_pixel_blocks_follow_the_tile_shape(unit_scenes, scene, tile):
    """A unit of 256 slots is four consecutive blocks of a tile -- a column of 8x32 pixels at 8x32, a row of 32x8 at 32x8, and so on. Frame,
    records, pass plane and state against the restatement with the layout of this tile, fed with the default-tile twin's frames and
    records (a pixel's frame and record do not depend on the tile while its unit is active: the tests above); allowance 0 and 8; one
    owner, and three at 24x32."""
    sc, kw, slots = unit_scenes[scene], dict(BUILDS["exact"], flags=0), UNIT_SLOTS[scene]
    frames, records, _ = twin(sc, scene, W, H, kw)
    assert unit_slots_of(sc, W, H, **kw) == slots and unit_slots_of(sc, W, H, tile=tile, **kw) == slots
    # the median of the default tile's units' worst relative error at pass 16, as median_target has it; a pixel whose error is still
    # unknown there (stress30 has pixels with a non-finite batch or three) is loud whatever the target and is left out of it
    _, unit, _ = unit_of(W, H, 1, slots)
    rel = rel32(records[4])
    target = float(np.float32(np.median([rel[unit == u].max() for u in np.unique(unit)])))
    assert target > 0
    # what keeps the comparison from passing for nothing, from the twin's records alone: at this shape some pixel retires at 16 and some
    # stays active; and at 8x32 the retirement map of 256-slot units is not the default tile's, so a select kernel that took every tile
    # for 64x16 fails
    retired0 = restate(records, W, H, 1, slots, target, 0, tile=tile)
    assert (retired0 == 16).any() and (retired0 == 0).any(), (scene, tile, np.unique(retired0))
    differs = not np.array_equal(retired0, restate(records, W, H, 1, slots, target, 0))
    print("%s %s: retired at 16 / 32 / active: %d / %d / %d pixels; differs from the default tile's map: %s" %
          (scene, tile_id(tile), (retired0 == 16).sum(), (retired0 == 32).sum(), (retired0 == 0).sum(), differs))
    if slots == 256 and tile == (8, 32):
        assert differs
    for allowance in (0, 8):
        rule = dict(target=target, floor=FLOOR, allowance=allowance)
        for owners in (1, 3) if tile == (24, 32) else (1,):
            retired = restate(records, W, H, owners, slots, target, allowance, tile=tile)
            frame, rec, plane = expected(frames, records, retired)
            before = restate(records, W, H, owners, slots, target, allowance, passes=16, tile=tile)
            paths = 4 * 16 * (W * H + int((before == 0).sum()))
            for cuts in ((PASSES,), (1, 2, 29)):
                got = run(sc, W, H, cuts, owners, rule, tile=tile, **kw)
                why = (scene, tile, allowance, owners, cuts)
                assert np.array_equal(bits(got[0]), bits(frame)), (why, np.argwhere(bits(got[0]) != bits(frame))[:4])
                assert same_records(got[1], rec), why
                assert np.array_equal(got[2], plane), (why, np.argwhere(got[2] != plane)[:4])
                s = got[3]
                assert (s["pixels"], s["activePixels"], s["paths"], s["unitSlots"]) == (W * H, int((retired == 0).sum()), paths, slots), (why, s)
                assert s["lastDecisionPass"] == (PASSES if (before == 0).any() else 16), (why, s)


# ---- the noise-guided denoiser ----------------------------------------------------------------------------------------------------------

def _guided(r):
    d = r.denoise(iterations=5, noise_guided=True)
    return d["radiance"], d["argb8"]


@pytest.fixture(scope="module")
def guided_reference(scenes):
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, seed=SEED, exact=True, aov=True, noise=True) as r:
        r.render(16)
        nz = r.noise()
        want = _guided(r)
        plain = r.denoise(iterations=5)["radiance"]
    # more than half the pixels are measured, so the records' path through the tile map is what is compared
    assert ((nz["stderr"] >= 0) & (nz["mean"] > 0)).sum() > W * H / 2
    assert not np.array_equal(bits(want[0]), bits(plain))
    return want


@pytest.mark.parametrize("tile", TILES, ids=tile_id)
def test_the_guided_denoiser_reads_its_records_through_the_tile_map(scenes, guided_reference, tile):
    """EXACT, 16 passes, five iterations: the one owner's own records at every shape; at 24x32 also a three-owner root fed with the
    owners' planes (kajo_hip_denoise_guide_planes)."""
    from test_hip_aov_tiled import _compose
    sc = scenes["spheres_a169"]
    with HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, aov=True, noise=True, tile=tile) as r:
        r.render(16)
        got = _guided(r)
    assert same(got, guided_reference), (tile, np.argwhere(bits(got[0]) != bits(guided_reference[0]))[:4])
    if tile != (24, 32):
        return
    owners = [HipRenderer(sc, W, H, spp=4, seed=SEED, exact=True, aov=True, aov_tiled=True, noise=True, tile=tile, tile_index=i, tile_count=3)
              for i in range(3)]
    try:
        planes = None
        for o in owners:
            o.render(16)
        for o in owners:
            planes = o.noise(out=planes)
        keep = _compose(owners, matte=False)
        owners[0].denoise_guide_planes(planes["mean"], planes["stderr"])
        got = _guided(owners[0])
        assert same(got, guided_reference), (tile, "three owners")
        del keep
    finally:
        for o in owners:
            o.close()
