"""Depth of field (include/kajo_hip.h kajo_hip_lens, kajo_hip_lens_coc, kajo_hip_lens_depth_at, kajo_hip_present_lens_argb8;
kajo_amd/csrc/lens.hip) on the GPU.

The kernels are held to tests/lens_replay.py, the numpy restatement of the header's definition. The stage's decisions -- the planes r and
z -- must be the restatement's float32 planes bit for bit. For the frame the counting masks must agree exactly, the pixels that do not
count and the .w channel keep their bits, and at a counting pixel, per channel,
    |out - ref| / P <= (n + 16) 2^-23 sum(w |m_q|) / sum(w),    n = (2 maxRadius + 1)^2:
the kernel forms sum(w m) and sum(w) as float32 sums of at most n terms of non-negative weight, each of which carries at most n 2^-24 of
the sum of the magnitudes, and a weight is five roundings from the restatement's (re + 1, the product, the scaling by pi, the sum, the
quotient), the quotient and the scaling by P three more: 16 covers those. It is not tuned. Synthetic inputs go in through the tile
buffers of a handle with tiled AOVs. Where the definition makes the output a copy the images are the existing calls' bit for bit; image
and planes must not depend on how many owners the frame was dealt to, and the calls must leave the handle as a twin that never ran them."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import bits, read_png, upload_aov, upload_frame
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import Scene, stress_scene
from lens_replay import aov_of, bound, counting, depth_fields, planes, restate
from local_replay import synthetic_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
F32, F64 = np.float32, np.float64
FOCUS = 10.0
# the workgroup tile is 32x16: 130x70 makes five tiles by five, with halos that cross tiles on both axes
SHAPES = [(1, 1), (2, 1), (7, 5), (41, 23), (65, 9), (130, 70)]
PARAMS = [dict(max_radius=R, aperture=a) for R in (1, 5, 16) for a in (0.01, 0.1, 1.0)]
SEEN = dict(share=0.0)  # the largest share of the allowance seen in the session, printed by every test that compares


def check_against(got, F, A, B, passes, what="", **params):
    """The conditions of the module docstring against the restatement; -> the largest share of the allowance used."""
    want = restate(F, A, B, passes, **params)
    F = np.asarray(F, F32)
    c = want["counts"]
    assert np.array_equal(counting(got, passes)[1], c), (what, params)      # the same pixels count: a condition, no tolerance
    assert np.array_equal(bits(got[~c]), bits(F[~c])), (what, params)        # the others: as they went in
    assert np.array_equal(bits(got[..., 3]), bits(F[..., 3])), (what, params)
    allowance = bound(params.get("max_radius", 16)) * want["scale"][c]
    err = np.abs(got[..., :3].astype(F64)[c] - want["out64"][c]) / passes
    with np.errstate(all="ignore"):
        share = float(np.max(np.where(err > 0, err / allowance, 0.0), initial=0.0))
    SEEN["share"] = max(SEEN["share"], share)
    print("%s %s: largest share of the allowance %.4f (r up to %.2f)" % (what, sorted(params.items()), share, want["r"].max()))
    assert (err <= allowance).all(), (what, params, share)
    return share


def _report(what):
    print("%s: largest share of the allowance so far %.4f" % (what, SEEN["share"]))


def _frames(W, H, passes):
    frames = synthetic_frames(W, H, passes)
    f = np.full((H, W, 4), 0.01, F32) * F32(passes)
    f[H // 2, W // 2 - (1 if W > 1 else 0), :3] = F32([900.0, 450.0, 120.0]) * F32(passes)  # beside the depth step, on its near side
    frames["on_step"] = f
    return frames


CHUNKS = [(s, k, 3 if s == (130, 70) else 1) for s in SHAPES for k in range(3 if s == (130, 70) else 1)]


@pytest.mark.parametrize("shape,chunk,chunks", CHUNKS, ids=["%dx%d-%d" % (s[0], s[1], k) for s, k, _ in CHUNKS])
def test_synthetic_frames_and_depths_match_the_restatement(scenes, shape, chunk, chunks):
    """Every depth field x every frame at each shape, the parameter grid (maxRadius 1, 5, 16 x aperture 0.01, 0.1, 1) dealt over the pairs
    in turn: windows wider than the image, odd sizes, frames of one workgroup and of several. The planes are compared for every field and
    every parameter set."""
    W, H = shape
    passes = 3
    fields = depth_fields(W, H, FOCUS)
    frames = _frames(W, H, passes)
    pairs = [(fn, gn) for fn in fields for gn in frames]
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True, aov=True, aov_tiled=True) as r:
        loaded = None
        for i, (fn, gn) in enumerate(pairs):
            if i % chunks != chunk:
                continue
            A, B = aov_of(fields[fn])
            if loaded != gn:
                upload_frame(r, frames[gn], passes)
                loaded = gn
            upload_aov(r, A, B)
            params = dict(PARAMS[(i // chunks + 4 * chunk) % len(PARAMS)], focus_distance=FOCUS)
            check_against(r.lens(**params), frames[gn], A, B, passes, "%dx%d %s %s" % (W, H, fn, gn), **params)
            if gn == "constant":
                for p in PARAMS:  # the decisions: bit for bit, no tolerance
                    coc = r.lens_coc(focus_distance=FOCUS, **p)
                    rr, zz = planes(A, B, p["aperture"], FOCUS, p["max_radius"])
                    assert np.array_equal(bits(coc["radius"]), bits(rr)) and np.array_equal(bits(coc["depth"]), bits(zz)), (fn, p)
    _report("%dx%d" % (W, H))


def test_copy_and_in_focus_cases(scenes):
    """aperture 0: the frame itself, whatever else is set; every r zero: (F / P) P bit for bit."""
    W, H, passes = 41, 23, 3
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True, aov=True, aov_tiled=True) as r:
        A, B = aov_of(depth_fields(W, H, FOCUS)["focus"])
        for name, frame in _frames(W, H, passes).items():
            upload_frame(r, frame, passes)
            upload_aov(r, A, B)
            assert np.array_equal(bits(r.lens(aperture=0.0, focus_distance=3.0, max_radius=7)), bits(frame)), name
            got = r.lens(aperture=1.0, focus_distance=FOCUS)
            m, c = counting(frame, passes)
            want = frame.copy()
            want[..., :3] = np.where(c[..., None], m * F32(passes), frame[..., :3])
            assert np.array_equal(bits(got[c]), bits(want[c])) and np.array_equal(bits(got[~c]), bits(frame[~c])), name


def _scene(scenes, name):
    return stress_scene(scenes["spheres_a169"], 1000, 16) if name == "1000" else scenes[name]


RENDERED = [("spheres_a169", 160, 90, b, s) for b in sorted(BUILDS) for s in (False, True)] + [("1000", 96, 54, "exact", False)]


@pytest.mark.parametrize("name,W,H,build,specular", RENDERED, ids=["%s-%s%s" % (n, b, "-specular" if s else "") for n, _, _, b, s in RENDERED])
def test_rendered_frames_match_the_restatement(scenes, name, W, H, build, specular):
    """The restatement fed from the handle's own aov() and the stage's own input frame; focus on what the centre pixel shows:
    lens_depth_at is the depth plane's value there and r is exactly 0 there."""
    with HipRenderer(_scene(scenes, name), W, H, spp=4, aov=True, aov_specular=specular, **BUILDS[build]) as r:
        r.render(3)
        acc = r.radiance()
        A, B = r.aov()["raw"]
        z = r.lens_depth_at(W // 2, H // 2)
        assert np.isfinite(z) and z > 0
        params = dict(aperture=0.05, focus_distance=z, max_radius=16)
        coc = r.lens_coc(**params)
        rr, zz = planes(A, B, 0.05, z, 16)
        assert np.array_equal(bits(coc["radius"]), bits(rr)) and np.array_equal(bits(coc["depth"]), bits(zz))
        assert bits(F32([z]))[0] == bits(coc["depth"])[H // 2, W // 2] and coc["radius"][H // 2, W // 2] == 0.0
        for x, y in ((0, 0), (W - 1, H - 1), (W // 3, 2 * H // 3)):
            assert bits(F32([r.lens_depth_at(x, y)]))[0] == bits(coc["depth"])[y, x]
        assert coc["radius"].max() > 2.0
        got = r.lens(**params)
        check_against(got, acc, A, B, 3, "%s %s" % (name, build), **params)
        assert not np.array_equal(bits(got[..., :3]), bits(acc[..., :3]))
        if build == "exact" and not specular:
            # behind the denoiser and behind the despeckle: the stage's input is their frame
            dn, ds = dict(iterations=2), dict(factor=2.0, floor=0.01)
            check_against(r.lens(denoise=dn, **params), r.denoise(**dn)["radiance"], A, B, 3, "after denoise", **params)
            check_against(r.lens(despeckle=ds, **params), r.despeckle(**ds)["radiance"], A, B, 3, "after despeckle", **params)
    _report("%s %dx%d %s" % (name, W, H, build))


def test_specular_aovs_defocus_reflections_by_their_chain_length(scenes):
    """spheres.json has a mirror wall and a glass ball: with aov_specular the depth is the whole chain's, so the CoC plane differs from the
    first-hit one exactly where a sample was followed -- where the depth sums differ -- and is identical elsewhere."""
    W, H = 160, 90
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, exact=True, aov=True) as first, \
            HipRenderer(scenes["spheres_a169"], W, H, spp=4, exact=True, aov=True, aov_specular=True) as chain:
        first.render(2)
        chain.render(2)
        z = first.lens_depth_at(W // 2, H // 2)
        p = dict(aperture=0.05, focus_distance=z)
        a, b = first.lens_coc(**p), chain.lens_coc(**p)
        followed = bits(first.aov()["raw"][1][..., 3]) != bits(chain.aov()["raw"][1][..., 3])
        followed |= bits(first.aov()["raw"][0][..., 3]) != bits(chain.aov()["raw"][0][..., 3])
        assert followed.sum() > W * H // 50 and (~followed).sum() > W * H // 4
        assert np.array_equal(bits(a["radius"])[~followed], bits(b["radius"])[~followed])
        assert np.array_equal(bits(a["depth"])[~followed], bits(b["depth"])[~followed])
        longer = b["depth"][followed] > a["depth"][followed]
        assert longer.mean() > 0.9  # the chain goes on behind the mirror
        assert (bits(a["radius"])[followed] != bits(b["radius"])[followed]).mean() > 0.5


TONES = [dict(), dict(curve="reinhard", exposure=1.0, white=2.0), dict(curve="aces", auto_exposure=True)]


def _same_result(a, b):
    return all(bits(F32([a[k]]))[0] == bits(F32([b[k]]))[0] if isinstance(a[k], float) else a[k] == b[k] for k in a) and a.keys() == b.keys()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_copy_cases_are_the_existing_calls_bit_for_bit(scenes, build):
    """aperture 0: kajo_hip_lens is the frame the first stages give, present(lens=copy, ...) is present(...), image and scale or result,
    with and without each other stage; lens == NULL in the chain call is kajo_hip_present_local_argb8."""
    ds, dn, gl, mt = dict(factor=2.0, rank=2, floor=0.01), dict(iterations=2), dict(levels=4, strength=0.25), dict(percentile=0.4, auto_white=True)
    lc = dict(iterations=3, compression=0.5)
    copy = dict(aperture=0.0, focus_distance=3.0, max_radius=7)
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(3)
        assert np.array_equal(bits(r.lens(**copy)), bits(r.radiance()))
        assert np.array_equal(bits(r.lens(denoise=dn, **copy)), bits(r.denoise(**dn)["radiance"]))
        assert np.array_equal(bits(r.lens(despeckle=ds, **copy)), bits(r.despeckle(**ds)["radiance"]))
        assert np.array_equal(bits(r.lens(despeckle=ds, denoise=dn, **copy)), bits(r.local(despeckle=ds, denoise=dn, compression=1.0, detail=1.0)))
        for tone in TONES:
            for stages in (dict(), dict(despeckle=ds), dict(denoise=dn), dict(glare=gl), dict(local=lc), dict(despeckle=ds, denoise=dn, glare=gl, local=lc)):
                img, s = r.present(lens=copy, **stages, **tone)
                want, s_want = r.present(**stages, **tone)
                assert np.array_equal(img, want) and bits(F32([s]))[0] == bits(F32([s_want]))[0], (tone, stages)
                if not tone.get("auto_exposure"):
                    img, res = r.present(lens=copy, meter=mt, **stages, **tone)
                    want, res_want = r.present(meter=mt, **stages, **tone)
                    assert np.array_equal(img, want) and _same_result(res, res_want), (tone, stages)
        assert np.array_equal(r.present(lens=copy)[0], r.argb8())
        # lens == NULL: kajo_hip_present_lens_argb8 is kajo_hip_present_local_argb8
        L = capi.lib()
        t, m, l = r._tone_params(curve="reinhard"), r._meter_params(**mt), r._local_params(**lc)
        ref = lambda p: None if p is None else C.byref(p)
        for meter in (None, m):
            for local in (None, l):
                a, b = np.empty((75, 100), np.uint32), np.empty((75, 100), np.uint32)
                ra, rb = capi.KajoMeterResult(), capi.KajoMeterResult()
                capi.check(L.kajo_hip_present_lens_argb8(r._h, None, None, None, None, ref(local), ref(meter), C.byref(t),
                                                         a.ctypes.data_as(C.c_void_p), C.byref(ra)))
                capi.check(L.kajo_hip_present_local_argb8(r._h, None, None, None, ref(local), ref(meter), C.byref(t), b.ctypes.data_as(C.c_void_p),
                                                          C.byref(rb)))
                assert np.array_equal(a, b) and _same_result(r._meter_result(ra), r._meter_result(rb))
    # ... and with lens == NULL the handle needs no AOVs
    with HipRenderer(scenes["spheres_a43"], 64, 48, spp=4, exact=True) as plain:
        plain.render(1)
        a = np.empty((48, 64), np.uint32)
        t = plain._tone_params()
        capi.check(capi.lib().kajo_hip_present_lens_argb8(plain._h, None, None, None, None, None, None, C.byref(t), a.ctypes.data_as(C.c_void_p), None))
        assert np.array_equal(a, plain.argb8())


LENS = dict(aperture=0.08, focus_distance=6.0, max_radius=12)


def test_chain_is_the_local_chain_over_the_stage_s_own_frame(scenes):
    """present(lens=L, glare, local, meter, **tone) = kajo_hip_present_local_argb8 over kajo_hip_lens's own frame written into a twin's
    accumulation: the blur sits in front of the glare, behind the despeckle and the denoiser."""
    sc = scenes["spheres_a169"]
    gl, lc, mt = dict(levels=4, strength=0.25), dict(iterations=3, compression=0.5), dict(percentile=0.4, auto_white=True)
    with HipRenderer(sc, 130, 70, spp=4, exact=True, aov=True) as r, HipRenderer(sc, 130, 70, spp=4, exact=True) as twin:
        r.render(3)
        for front in (dict(), dict(despeckle=dict(factor=2.0, floor=0.01), denoise=dict(iterations=2))):
            frame = r.lens(**front, **LENS)
            upload_frame(twin, frame, 3)
            for behind in (dict(), dict(glare=gl), dict(glare=gl, local=lc)):
                for tone in TONES:
                    img, s = r.present(lens=LENS, **front, **behind, **tone)
                    want, s_want = twin.present(**behind, **tone)
                    assert np.array_equal(img, want) and bits(F32([s]))[0] == bits(F32([s_want]))[0], (front, behind, tone)
                    assert not np.array_equal(img, r.present(**front, **behind, **tone)[0])
                img, res = r.present(lens=LENS, meter=mt, **front, **behind, curve="reinhard")
                want, res_want = twin.present(meter=mt, **behind, curve="reinhard")
                assert np.array_equal(img, want) and _same_result(res, res_want), (front, behind)


@pytest.mark.parametrize("tile", [(64, 16), (32, 8)], ids=["tile64x16", "tile32x8"])
def test_frame_and_planes_do_not_depend_on_the_owners(scenes, tile):
    """130x70 on one handle, on a second call, on a twin, and on the root of 2, 3 and 8 tiled owners on one device after compose and
    compose_aov: the same bits."""
    from test_hip_aov_tiled import _close, _compose, _render, _tiled
    sc = scenes["spheres_a169"]
    W, H = 130, 70
    gl, tone = dict(levels=3, strength=0.2), dict(curve="reinhard")
    kw = dict(spp=4, seed=0o715517, tile=tile, aov=True, exact=True)
    with HipRenderer(sc, W, H, **kw) as r, HipRenderer(sc, W, H, **kw) as twin:
        _render([r])
        _render([twin])
        z = r.lens_depth_at(W // 2, H // 2)
        lens = dict(aperture=0.06, focus_distance=z)
        frame, coc, (img, s) = r.lens(**lens), r.lens_coc(**lens), r.present(lens=lens, glare=gl, **tone)
        assert np.array_equal(bits(frame), bits(r.lens(**lens))) and np.array_equal(img, r.present(lens=lens, glare=gl, **tone)[0])
        assert np.array_equal(bits(frame), bits(twin.lens(**lens))) and np.array_equal(img, twin.present(lens=lens, glare=gl, **tone)[0])
        assert bits(F32([twin.lens_depth_at(W // 2, H // 2)]))[0] == bits(F32([z]))[0]
        r.radiance()  # composes the float frame: the calls now read it, row-major
        assert np.array_equal(bits(frame), bits(r.lens(**lens)))
        denoised = r.lens(denoise=dict(iterations=2), **lens)
    for count in (2, 3, 8):
        owners = _tiled(sc, W, H, tile, count, dict(exact=True))
        try:
            _render(owners)
            keep = _compose(owners, matte=False)
            root = owners[0]
            assert bits(F32([root.lens_depth_at(W // 2, H // 2)]))[0] == bits(F32([z]))[0], count
            got = root.lens_coc(**lens)
            assert np.array_equal(bits(got["radius"]), bits(coc["radius"])) and np.array_equal(bits(got["depth"]), bits(coc["depth"])), count
            assert np.array_equal(bits(root.lens(**lens)), bits(frame)), count
            assert np.array_equal(bits(root.lens(denoise=dict(iterations=2), **lens)), bits(denoised)), count
            assert np.array_equal(root.present(lens=lens, glare=gl, **tone)[0], img), count
            del keep
        finally:
            _close(owners)


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_the_stage_leaves_the_handle_as_it_was(scenes, build):
    """radiance(), argb8(), aov(), matte() and counters() (kernelMs included) of a handle that ran the stage every way are those of a twin
    that never did; so are the passes rendered afterwards."""
    sc = scenes["spheres_a43"]
    kw = dict(spp=4, aov=True, matte=True, counters=True, **BUILDS[build])
    with HipRenderer(sc, 100, 75, **kw) as a, HipRenderer(sc, 100, 75, **kw) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        a.lens()
        a.lens(aperture=0.2, focus_distance=4.0, max_radius=9, denoise=dict(iterations=2), despeckle=dict())
        a.lens_coc(aperture=0.5)
        a.lens_depth_at(3, 4)
        a.present(lens=dict(aperture=0.1), curve="aces", auto_exposure=True)
        a.present(lens=dict(), glare=dict(), local=dict(metered=True), meter=dict(auto_white=True), denoise=dict(iterations=3), curve="reinhard")
        assert a.counters()["kernelMs"] == ms
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert np.array_equal(a.argb8(), b.argb8())
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        ma, mb = a.matte(), b.matte()
        assert np.array_equal(ma["ids"], mb["ids"]) and np.array_equal(ma["counts"], mb["counts"]) and ma["samples"] == mb["samples"]
        ca, cb = a.counters(), b.counters()
        for key in ("passes", "launches", "paths", "traversals", "vertices"):
            assert ca[key] == cb[key], key
        assert ca["passes"] == 3
        a.render(2)
        b.render(2)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert a.counters()["passes"] == 5
        assert np.array_equal(bits(a.lens(aperture=0.1)), bits(b.lens(aperture=0.1)))


def _code(call):
    with pytest.raises(capi.KajoError) as e:
        call()
    return e.value.code


def test_refusals_and_states_on_a_device(scenes):
    sc = scenes["spheres_a43"]
    every = lambda r: (r.lens, r.lens_coc, lambda: r.lens_depth_at(1, 1), lambda: r.present(lens=dict()))
    with HipRenderer(sc, 64, 48, spp=4, exact=True) as plain:  # no AOV flag
        plain.render(1)
        for call in every(plain):
            assert _code(call) == capi.KAJO_E_STATE
        assert "AOV flag" in capi.lib().kajo_hip_last_error().decode()
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True) as r:
        for call in every(r):
            assert _code(call) == capi.KAJO_E_STATE  # nothing rendered
        assert "nothing rendered" in capi.lib().kajo_hip_last_error().decode()
        r.render(1)
        for x, y in ((-1, 0), (0, -1), (64, 0), (0, 48)):
            assert _code(lambda: r.lens_depth_at(x, y)) == capi.KAJO_E_INVALID
        for call in (lambda: r.lens(aperture=2.0), lambda: r.lens_coc(max_radius=0), lambda: r.present(lens=dict(focus_distance=0.0))):
            assert _code(call) == capi.KAJO_E_INVALID
        l = r._lens_params()
        assert capi.lib().kajo_hip_lens(r._h, None, None, C.byref(l), None) == 0  # radiance may be NULL
        assert capi.lib().kajo_hip_lens_coc(r._h, C.byref(l), None, None) == 0
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True, aov_tiled=True) as t:
        t.render(1)
        for call in every(t):
            assert _code(call) == capi.KAJO_E_STATE  # before compose_aov
        t.compose_aov()
        t.lens()
        t.lens_coc()
        t.render(1)
        for call in every(t):
            assert _code(call) == capi.KAJO_E_STATE  # a later render
        t.compose_aov()
        t.present(lens=dict())
        t.reset()
        for call in every(t):
            assert _code(call) == capi.KAJO_E_STATE  # a reset
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True, aov_tiled=True, tile_index=1, tile_count=2) as part:
        part.render(1)
        for call in every(part):
            assert _code(call) == capi.KAJO_E_STATE  # a share of the frame, nothing composed


@pytest.fixture(scope="module")
def driver_reference():
    """caustics 96x54, 2 passes, through the C ABI: the image of the chain the driver is asked for, focused on the centre pixel."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    with HipRenderer(sc, 96, 54, exact=True, aov=True) as r:
        r.render(2)
        acc = r.radiance()
        focus = r.lens_depth_at(48, 27)
        lens = dict(aperture=0.05, focus_distance=focus, max_radius=12)
        px, _ = r.present(lens=lens, glare=dict(strength=0.1), curve="aces")
        plain, _ = r.present(glare=dict(strength=0.1), curve="aces")
        at, _ = r.present(lens=dict(lens, focus_distance=r.lens_depth_at(10, 40)), glare=dict(strength=0.1), curve="aces")
        rmax = float(r.lens_coc(**lens)["radius"].max())
    assert not np.array_equal(px, plain) and not np.array_equal(px, at)
    return dict(acc=acc, px=px, focus=focus, rmax=rmax, at=at)


DRIVER = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "--json"]
SCENE = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("owners", ["1", "3-on-one-device-tiled"])
def test_driver_writes_the_c_abi_s_image(tmp_path, driver_reference, owners):
    """kajo_render --lens-aperture 0.05 --lens-max-radius 12 --glare 0.1 --tonemap aces writes the PNG HipRenderer.present gives on the
    same frame focused on the centre pixel; --json reports the focus and the largest radius; --raw stays the accumulation."""
    gpus = {"1": ["--gpus", "1"], "3-on-one-device-tiled": ["--gpus", "3", "--same-device", "--aov-tiled"]}[owners]
    ref = driver_reference
    out, raw = str(tmp_path / "o.png"), str(tmp_path / "o.raw")
    p = subprocess.run(DRIVER + gpus + ["-o", out, "--raw", raw, "--lens-aperture", "0.05", "--lens-max-radius", "12", "--glare", "0.1",
                                        "--tonemap", "aces", SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    assert np.array_equal(bits(np.fromfile(raw, np.float32).reshape(54, 96, 4)), bits(ref["acc"]))
    png = read_png(out)
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (ref["px"] >> shift) & 255), k
    assert F32(stats["lens_focus"]) == F32(ref["focus"]) and F32(stats["lens_max_radius_px"]) == F32(ref["rmax"])
    if owners == "1":
        p = subprocess.run(DRIVER + gpus + ["-o", out, "--lens-aperture", "0.05", "--lens-max-radius", "12", "--lens-focus-at", "10,40", "--glare",
                                            "0.1", "--tonemap", "aces", SCENE], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        png = read_png(out)
        for k, shift in enumerate((16, 8, 0)):
            assert np.array_equal(png[..., k], (ref["at"] >> shift) & 255), k
