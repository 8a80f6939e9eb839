"""Every reader of the tile map at tile shapes other than the default 64x16 (KajoParams.tileW / tileH; kajo_amd/csrc/render_args.h TileMap).

The oracle is the library's own contract (include/kajo_hip.h): the frame is a function of scene, parameters and pass count, not of
workgroups or GPUs. A wave is always one 8x8 pixel block aligned to 8, tiles are multiples of 8 and start at multiples of the tile, and
a pixel's streams are keyed by (pixel, sample, pass, seed) -- so the set of pixels of every wave, and every sum formed for a pixel, is
the same for every tile shape. In ALL THREE numerics builds every per-pixel output of a handle with tile T must therefore equal that of
a handle with the default tile word for word (NaN payloads included); no tolerance appears in this file. The default tile's outputs are
what the neighbouring test modules hold to the oracle and to their numpy restatements; here the STRICT default-tile frame is in addition
compared with the oracle directly (`oracle_frames`).

Shapes: three are not powers of two -- 24x32, 40x32 (3 and 5 waves across a tile) and 96x8 (12 across, one down) -- where `%` and `/`
by tileW >> 3 are no masks and shifts; 8x32 and 32x8 tell tileW >> 3 from tileH >> 3; 128x64 is larger than the frames: one tile, and
of several owners all but one own nothing (kajo_hip_render's early return). Frames are ragged on both axes.

Which test reaches which reader (all at every shape of TILES unless said):
  the render kernels' "which pixel is mine" block, every kernel class ........ test_render_and_resolve, test_raw_tile_buffers
  kajo_compose, kajo_resolve_tiles_*, kajo_hip_counters' owned pixels ......... test_render_and_resolve, test_owners_through_the_device_paths
  kajo_amd/tiles.py against the device's buffers, slots outside the image ..... test_raw_tile_buffers
  kajo_tone_*_tiles, kajo_glare_bright / apply, kajo_despeckle_*, denoise ..... test_post_stages_from_a_tiled_handle (one owner),
                                                                                test_owners_through_the_device_paths (24x32, 40x32, 128x64)
  AOV, matte and KAT handles (which must NOT read the tile shape) ............. test_aov_and_mattes..., test_kat_trace...
  kajo_fold_parts and the parted launch tail (64x16 and 32x32) ................ test_parted_tail_with_rows_outside_the_image
The readers that came with the noise estimate, adaptive sampling and the noise-guided denoiser are reached by
tests/test_hip_noise_tile_shapes.py, which takes TILES, `same` and `bits` from here:
  kajo_noise_map (kajoTileSlot), kajo_hip_read_noise_moments' host loop ....... test_noise_records_planes_and_histogram_are_the_default_tiles
  kajo_adapt_passes (kajoTileSlot) ............................................ test_adaptive_units_of_one_pixel_block_do_not_depend_on_the_tile_shape,
                                                                                test_adaptive_units_of_four_pixel_blocks_follow_the_tile_shape
  kajo_adapt_select (kajo::adaptSlotPixel, adapt_math.h) ...................... the same two, and on the host, as kajoTileSlot's exact inverse,
                                                                                tests/test_adaptive_cpu.py
  kajo_denoise_guided_v0 (kajoTileSlot) ....................................... test_the_guided_denoiser_reads_its_records_through_the_tile_map"""
import numpy as np
import pytest

from framelib import bits
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import stress_scene
from kajo_amd.tiles import TileLayout

pytestmark = pytest.mark.gpu

TILES = [(8, 32), (32, 8), (24, 32), (40, 32), (96, 8), (128, 64)]
DEFAULT = (64, 16)
BUILDS = {"strict": dict(strict=True), "exact": dict(exact=True), "fast": dict()}
SEED = 0o715517  # (HipRenderer's default)
W, H = 100, 75
PASSES = 3
F32 = np.float32
tile_id = lambda t: "%dx%d" % t


def same(a, b):
    """Word equality of two results: float32 arrays by their bits, other arrays by value, Python floats as float32 words, tuples and
    dicts element by element."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return bool((bits(F32(a)) == bits(F32(b))).all())
    if isinstance(a, np.ndarray) and a.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


def raw_buffer(r):
    """The handle's whole tile buffer on the host: (slots, 4) float32, and the bytes kajo_hip_tile_buffer reports."""
    import torch
    from bench import DevicePtr
    r.wait()
    ptr, nbytes = r.tile_buffer()
    t = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").clone()
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(-1, 4), nbytes


def used_slots(lay):
    """(world, slots_per_owner) bool: the slots owner_and_slot maps an in-image pixel to."""
    ys, xs = np.mgrid[0:lay.H, 0:lay.W]
    owner, slot = lay.owner_and_slot(xs, ys)
    used = np.zeros((lay.world, lay.slots_per_owner), bool)
    used[owner, slot] = True
    return used


# A NaN pixel and a firefly (sums over PASSES), written into the accumulation as tests/test_hip_despeckle.py writes its holes: through the
# layout, whoever owns the pixel. (95, 71) lies in the ragged last tile of every shape; (47, 31) is the last pixel of a 24x32 tile and sits
# on a tile edge of 8x32, 24x32 and 96x8's rows, so the windows of repair and clamp cross tiles.
MARKS = [((95, 71), (np.nan, np.nan, np.nan)), ((47, 31), (3e5, 2e5, 1e5))]


def plant(owners, lay, marks=MARKS):
    import torch
    from bench import DevicePtr
    for o in owners:
        o.wait()
    for (x, y), rgb in marks:
        owner, slot = lay.owner_and_slot(np.array([x]), np.array([y]))
        ptr, nbytes = owners[int(owner[0])].tile_buffer()
        buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
        buf[int(slot[0]), :3] = torch.tensor(rgb, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def variants(scenes):
    """name -> (scene, create flags, the AOV instance of the scene's class -- chosen as the render kernel is): one per render kernel class."""
    from test_hip_aov import crowded_scene
    base = scenes["spheres_a169"]
    stress, crowd = stress_scene(base, 1000, 16), crowded_scene(base)
    return {
        "small": (base, 0, "kajo_aov_{}"),                    # one light: the PRESAMPLE instance; small frames: the SPLIT kernels
        "lights": (scenes["caustics_a169"], 0, "kajo_aov_{}"),  # three lights: the _lights instance
        "unsplit": (base, capi.KAJO_FLAG_NO_SPLIT, "kajo_aov_{}"),
        "biglist_lg": (stress, 0, "kajo_aov_{}_biglist_lg"),
        "big_lg": (stress, capi.KAJO_FLAG_NO_SHADOW_LISTS, "kajo_aov_{}_big_lg"),
        "biglist": (crowd, 0, "kajo_aov_{}_biglist"),
        "big": (crowd, capi.KAJO_FLAG_NO_SHADOW_LISTS, "kajo_aov_{}_big"),
    }


VARIANTS = ["small", "lights", "unsplit", "biglist_lg", "big_lg", "biglist", "big"]
ORACLE_VARIANTS = ("small", "biglist_lg")


@pytest.fixture(scope="module")
def oracle_frames(variants):
    """variant -> the oracle's (strict math) accumulation of the main frame, 4 spp x PASSES; None where the oracle is not built."""
    from oraclelib import OracleLib, available
    if not available("oracle"):
        return None
    O = OracleLib("oracle")
    out = {}
    for name in ORACLE_VARIANTS:
        f = O.create(variants[name][0], math=1).render(W, H, S=4, passes=PASSES, seed=SEED, depth_limit=8)
        f.setflags(write=False)
        out[name] = f
    return out


def equals_oracle(got, want):
    g, w = got[..., :3], want[..., :3]
    return bool(((bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))).all())


def test_the_scene_variants_are_one_per_kernel_class(variants):
    assert variants["lights"][0].n_lights > 1 and variants["small"][0].n_lights == 1
    for name, (sc, flags, kernel) in variants.items():
        with HipRenderer(sc, 16, 16, spp=4, strict=True, aov=True, flags=flags) as r:
            assert r.aov_kernel() == kernel.format("strict"), (name, r.aov_kernel())


# ---- (a) render and resolve, every kernel class ------------------------------------------------------------------------------------

FRAMES = [(100, 75, 4), (41, 23, 32), (65, 9, 4), (1, 1, 32)]  # W, H, samples per pass


def _render_and_resolve(sc, w, h, spp, tile, flags, build):
    with HipRenderer(sc, w, h, spp=spp, tile=tile, flags=flags, counters=True, **BUILDS[build]) as r:
        r.render(PASSES).wait()
        fused = r.argb8()   # no composed frame yet: straight from the tile buffer
        acc = r.radiance()  # composes the float frame
        two_pass = r.argb8()  # ... which the whole-frame resolve then reads
        c = r.counters()
    return dict(radiance=acc, fused=fused, two_pass=two_pass), c


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_render_and_resolve(variants, oracle_frames, variant, build):
    """radiance(), argb8() from the tile buffer and from the composed frame, and the counters, of every tile shape against the default
    tile's, per render kernel class and numerics build, on four ragged frames; the STRICT default-tile frame against the oracle."""
    sc, flags, _ = variants[variant]
    for w, h, spp in FRAMES:
        want, wc = _render_and_resolve(sc, w, h, spp, DEFAULT, flags, build)
        assert np.array_equal(want["fused"], want["two_pass"])
        if build == "strict" and (w, h) == (W, H) and variant in ORACLE_VARIANTS and oracle_frames is not None:
            assert equals_oracle(want["radiance"], oracle_frames[variant]), variant
        n = int(np.sqrt(float(spp)))
        for tile in TILES:
            got, c = _render_and_resolve(sc, w, h, spp, tile, flags, build)
            for k in want:
                assert same(got[k], want[k]), (variant, build, (w, h), tile, k, np.argwhere(bits(got[k]) != bits(want[k]))[:4])
            assert c["paths"] == TileLayout(w, h, 1, tile).owned_pixels(0) * n * n * PASSES == w * h * n * n * PASSES, (tile, c)
            assert c["passes"] == PASSES
            assert (c["traversals"], c["vertices"]) == (wc["traversals"], wc["vertices"]), (variant, build, (w, h), tile, c, wc)


# ---- the default-tile, one-owner references of the main frame ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reference(scenes, oracle_frames):
    """build -> the default-tile, one-owner handle's radiance and image of the main frame (spheres.json 16:9, 4 spp x PASSES), rendered
    once per build; the STRICT one is the oracle's frame."""
    cache = {}

    def get(build):
        if build not in cache:
            with HipRenderer(scenes["spheres_a169"], W, H, spp=4, **BUILDS[build]) as r:
                r.render(PASSES)
                acc, img = r.radiance(), r.argb8()
            if build == "strict" and oracle_frames is not None:
                assert equals_oracle(acc, oracle_frames["small"])
            acc.setflags(write=False)
            img.setflags(write=False)
            cache[build] = dict(radiance=acc, argb8=img)
        return cache[build]

    return get


# ---- (b) the raw tile buffer is what tiles.py says, and nothing else ---------------------------------------------------------------

@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("tile", TILES, ids=tile_id)
def test_raw_tile_buffers(scenes, reference, tile, build):
    """1, 3 and 8 owners: the owners' buffers, copied to the host and composed by kajo_amd/tiles.py, are the one-owner default-tile
    frame; their size is the layout's; and every slot no in-image pixel maps to -- the ragged tiles' outside parts, the padding tiles
    when the tile count is no multiple of the owners -- holds four +0.0 words, also after reset() and a second render."""
    from test_hip_tonemap import _gathered
    want = reference(build)["radiance"]
    sc = scenes["spheres_a169"]
    for count in (1, 3, 8):
        lay = TileLayout(W, H, count, tile)
        used = used_slots(lay)
        owners = [HipRenderer(sc, W, H, spp=4, tile=tile, tile_index=k, tile_count=count, **BUILDS[build]) for k in range(count)]
        try:
            for again in (False, True):
                for o in owners:
                    if again:
                        o.reset()
                    o.render(PASSES)
                raws = [raw_buffer(o) for o in owners]
                assert {nbytes for _, nbytes in raws} == {lay.slots_per_owner * 16}, (count, raws[0][1])
                g = np.stack([buf for buf, _ in raws])
                assert same(lay.compose(g), want), (tile, build, count, again)
                assert not bits(g)[~used].any(), (tile, build, count, again, np.argwhere(bits(g).any(-1) & ~used)[:4])
                # ... and the host mirror composes the buffers as the device's kajo_compose does
                gathered = _gathered(owners)
                owners[0].compose(gathered.data_ptr())
                assert same(owners[0].radiance(), lay.compose(g)), (tile, build, count, again)
        finally:
            for o in owners:
                o.close()
    assert (~used_slots(TileLayout(W, H, 8, tile))).any()  # (there are such slots at every shape)


# ---- (c) owners through the device paths -------------------------------------------------------------------------------------------

DS = dict(factor=2.0, rank=2, floor=0.01)
GL = dict(levels=4, strength=0.25)
TONE = dict(curve="reinhard", auto_exposure=True)


def _device_paths(owners, lay):
    """Every gathered device path on owners[0], then kajo_hip_compose and the whole-frame reads."""
    from test_hip_despeckle import _despeckle_params, _present_gathered
    from test_hip_glare import _display_gathered, _glare_params
    from test_hip_tonemap import _gathered, _gathered_image, _tone_params
    root = owners[0]
    gathered = _gathered(owners)
    d, g, t = _despeckle_params(**DS), _glare_params(**GL), _tone_params(**TONE)
    out = {}
    out["resolve"] = _gathered_image(root, gathered, lay.W, lay.H, resolve=True)[0]
    out["tonemap"] = _gathered_image(root, gathered, lay.W, lay.H, tone=t)
    out["display"] = _display_gathered(root, gathered, lay.W, lay.H, g, t)
    img, scale, counts = _present_gathered(root, gathered, lay.W, lay.H, d, g, t)
    out["present"] = (img, scale, np.array(counts, np.int64))
    root.compose(gathered.data_ptr())
    out["composed"] = (root.radiance(), root.argb8())
    return out


@pytest.fixture(scope="module")
def device_reference(scenes, reference):
    cache = {}

    def get(build):
        if build not in cache:
            with HipRenderer(scenes["spheres_a169"], W, H, spp=4, **BUILDS[build]) as r:
                r.render(PASSES)
                assert same(r.radiance(), reference(build)["radiance"])
                r.set_pass_count(PASSES)  # (forget the composed frame: the marks go into the tile buffer)
                plant([r], TileLayout(W, H, 1))
                cache[build] = _device_paths([r], TileLayout(W, H, 1))
            clamped, repaired = cache[build]["present"][2]
            assert clamped > 0 and repaired >= 1  # both despeckle kernels have work
        return cache[build]

    return get


@pytest.mark.parametrize("build", ["strict", "fast"])
@pytest.mark.parametrize("tile", [(24, 32), (40, 32), (128, 64)], ids=tile_id)
def test_owners_through_the_device_paths(scenes, device_reference, tile, build):
    """1, 2, 3 and 8 owners with a tile shape, gathered on one GPU: kajo_hip_compose + radiance() / argb8(), and the resolve, tonemap,
    display and present twins over the gathered buffers give the default-tile one-owner handle's image words, automatic-exposure
    scale word and despeckle counts."""
    want = device_reference(build)
    sc = scenes["spheres_a169"]
    for count in (1, 2, 3, 8):
        lay = TileLayout(W, H, count, tile)
        owners = [HipRenderer(sc, W, H, spp=4, tile=tile, tile_index=k, tile_count=count, **BUILDS[build]) for k in range(count)]
        try:
            for o in owners:
                o.render(PASSES)
            plant(owners, lay)
            got = _device_paths(owners, lay)
            for k in want:
                assert same(got[k], want[k]), (tile, build, count, k)
        finally:
            for o in owners:
                o.close()


# ---- (d) every post stage from a tiled handle ----------------------------------------------------------------------------------------

TONE_CURVES = [dict(curve="clamp"), dict(curve="reinhard", white=2.0), dict(curve="aces")]
MAX_LEVELS = int(np.ceil(np.log2(max(W, H))))  # halvings that take the frame to 1x1


def _stages(r, from_tiles):
    """Every post stage of the handle -> name -> result. from_tiles: forget the composed frame in front of every call (a stage may
    compose it), so that each one reads the tile buffer; otherwise compose it first, so that each one reads the frame."""
    def fresh():
        if from_tiles:
            r.set_pass_count(PASSES)
    if not from_tiles:
        r.radiance()
    out = {}
    for i, curve in enumerate(TONE_CURVES):
        for auto in (False, True):
            fresh()
            out["tone", i, auto] = r.tonemap(auto_exposure=auto, **curve)
    for iterations in (0, 3):
        for demodulate in (True, False):
            fresh()
            d = r.denoise(iterations=iterations, demodulate=demodulate)
            out["denoise", iterations, demodulate] = (d["radiance"], d["argb8"])
    for levels in (1, MAX_LEVELS):
        fresh()
        out["glare", levels] = r.glare(levels=levels, strength=0.3)
    fresh()
    d = r.despeckle()
    out["despeckle"] = (d["radiance"], np.int64([d["clamped"], d["repaired"]]))
    chain = dict(denoise=dict(iterations=2), glare=dict(levels=4, strength=0.3))
    fresh()
    out["display"] = r.display(curve="aces", auto_exposure=True, **chain)
    fresh()
    out["present"] = r.present(despeckle=dict(), curve="reinhard", white=2.0, auto_exposure=True, **chain) + (np.int64(r.despeckle_counts()),)
    return out


def _staged(scenes, tile, build):
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, tile=tile, aov=True, **BUILDS[build]) as r:
        r.render(PASSES)
        plant([r], TileLayout(W, H, 1, tile))
        before, _ = raw_buffer(r)
        tiles = _stages(r, from_tiles=True)
        frame = _stages(r, from_tiles=False)
        after, _ = raw_buffer(r)
        acc = r.radiance()
    assert same(before, after)  # the stages leave the accumulation alone
    assert same(acc, TileLayout(W, H, 1, tile).compose(after[None]))  # ... and radiance() is the raw sum
    return dict(tiles=tiles, frame=frame, radiance=acc)


@pytest.fixture(scope="module")
def staged_reference(scenes, reference):
    cache = {}

    def get(build):
        if build not in cache:
            got = _staged(scenes, DEFAULT, build)
            untouched = np.ones((H, W), bool)
            for (x, y), _ in MARKS:
                untouched[y, x] = False
            assert same(got["radiance"][untouched], reference(build)["radiance"][untouched])
            clamped, repaired = got["tiles"]["despeckle"][1]
            assert clamped >= 1 and repaired >= 1  # the firefly and the NaN pixel: both kernels fire
            cache[build] = got
        return cache[build]

    return get


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("tile", TILES, ids=tile_id)
def test_post_stages_from_a_tiled_handle(scenes, staged_reference, tile, build):
    """tonemap (three curves, with and without automatic exposure: image and scale), denoise (0 and 3 iterations, with and without
    demodulation: radiance and image), glare (1 level and as many as the frame holds), despeckle (radiance and both counts), display
    and present with every stage on -- each read from the tile buffer and from the composed frame -- against the default tile's. A NaN
    pixel and a firefly are in the accumulation, so despeckle's repair and clamp both have work."""
    want = staged_reference(build)
    got = _staged(scenes, tile, build)
    for path in ("tiles", "frame"):
        for k in want[path]:
            assert same(got[path][k], want[path][k]), (tile, build, path, k)
    assert same(got["radiance"], want["radiance"])


# ---- (e) AOV, matte and KAT handles are untouched by the tile shape --------------------------------------------------------------------

@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("specular", [False, True])
def test_aov_and_mattes_do_not_depend_on_the_tile_shape(scenes, build, specular):
    sc = scenes["caustics_a169"]

    def run(tile):
        with HipRenderer(sc, W, H, spp=4, tile=tile, aov=True, matte=True, aov_specular=specular, **BUILDS[build]) as r:
            r.render(PASSES)
            a, m = r.aov(), r.matte()
            return dict(aov=tuple(a["raw"]), samples=a["samples"], ids=m["ids"], counts=m["counts"], mask=r.matte_mask([0, 3]), radiance=r.radiance())

    want = run(DEFAULT)
    assert want["samples"] == 4 * PASSES and (want["counts"] > 0).any()
    for tile in ((24, 32), (8, 32)):
        assert same(run(tile), want), (tile, build, specular)


@pytest.mark.parametrize("build", ["strict", "fast"])
def test_kat_trace_does_not_depend_on_the_tile_shape(scenes, build):
    """The known-answer path fixes a 64x16 tile of its own: a handle created with 40x32 returns the default handle's words."""
    from test_hip_kat import _adversarial_rays
    sc = scenes["spheres_a1"]
    o, d = _adversarial_rays(sc, np.random.default_rng(7))
    with HipRenderer(sc, 8, 8, **BUILDS[build]) as r:
        want = r.kat_trace(o, d)
    with HipRenderer(sc, 8, 8, tile=(40, 32), **BUILDS[build]) as r:
        got = r.kat_trace(o, d)
    assert (want["idx"] > 0).any()
    assert same(got, want)
    if build == "strict":
        from oraclelib import OracleLib, available
        if available("oracle"):
            ref = OracleLib("oracle").create(sc, 0).trace(o, d)
            assert np.array_equal(got["idx"], ref["idx"]) and same(got["t"], ref["t"])


# ---- (f) the parted tail with a tile shape and rows outside the image ------------------------------------------------------------------

TAIL_W, TAIL_H = 1280, 728  # 14 560 pixel blocks in 16- or 32-row tiles, the last 8 rows of them outside the image


def _launches(sc, tile, flags=0, **build):
    """-> (raw tile buffer after launches of 16, 16 and 8 passes, tailGroups after each)"""
    groups = []
    with HipRenderer(sc, TAIL_W, TAIL_H, seed=SEED, passes_per_launch=16, tile=tile, flags=flags, **build) as r:
        for p in (16, 16, 8):
            r.render(p).wait()
            groups.append(r.counters()["tailGroups"])
        return raw_buffer(r)[0], groups


@pytest.mark.parametrize("build", ["fast", "exact"])
@pytest.mark.parametrize("tile", [(64, 16), (32, 32)], ids=tile_id)
def test_parted_tail_with_rows_outside_the_image(scenes, tile, build):
    """tests/test_hip_tail_parts.py at a frame whose last tile row is half outside the image: those pixel blocks cost nothing, sort
    last and are rendered in parts, and kajo_fold_parts adds every thread's side-buffer slot into the tile buffer -- for a lane
    outside the image a slot no part writes. The RAW tile buffer must be that of the unparted run (KAJO_FLAG_NO_SPLIT) word for
    word, with +0.0 words in every slot outside the image.
    Best effort: memory that was never cleared is often zero on a fresh allocation, so a handle of the same size is rendered in
    parts and closed first, to leave sums in freed device memory; nothing obliges the allocator to hand that memory out again."""
    sc = scenes["spheres_a169"]
    _launches(sc, tile, **BUILDS[build])  # (dirties what the next handle may be given)
    got, g = _launches(sc, tile, **BUILDS[build])
    assert g[0] == 0 and g[1] > 0 and g[2] > 0, g
    want, g0 = _launches(sc, tile, flags=capi.KAJO_FLAG_NO_SPLIT, **BUILDS[build])
    assert g0 == [0, 0, 0]
    lay = TileLayout(TAIL_W, TAIL_H, 1, tile)
    assert got.shape == (lay.slots_per_owner, 4)
    outside = ~used_slots(lay)[0]
    assert outside.sum() == TAIL_W * 8
    assert not bits(want)[outside].any()
    assert not bits(got)[outside].any(), np.argwhere(bits(got).any(-1) & outside)[:4]
    assert same(got, want), np.argwhere(bits(got) != bits(want))[:4]
