"""The grade (include/kajo_hip.h "The grade", kajo_hip_grade, kajo_hip_present_grade_*; kajo_amd/csrc/grade.hip) on the GPU.

The kernels are held WORD FOR WORD to kajo_hip_grade_pixels, the same lines (grade_math.h) compiled for the host, over the handle's own
radiance() / P and matte_mask() planes; and to tests/grade_replay.py's binary64 restatement within the allowance it derives from the
rule's rounding count and the power's conditioning (its docstring; nothing in it is tuned). Pixels that do not count keep their bits,
the identity case is the existing calls' image, the chain entry is the chain run by hand, the image does not depend on the owners, and
the calls leave the handle as a twin that never ran them."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import bits, read_png
from framelib import upload_frame as _upload
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, grade_neutral, grade_params, grade_pixels, grade_white_balance
from kajo_amd.scene import Scene, stress_scene
from grade_replay import fill, masks_of, restate64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
F32, F64 = np.float32, np.float64
SHAPES = [(1, 1), (7, 5), (41, 23), (65, 9), (130, 70)]  # 64x4 workgroups: one lane, ragged, several groups on both axes
PASSES = 3
SEEN = dict(share=0.0)

OPS = [dict(slope=[2.0, 0.5, 0.0], saturation=0.0), dict(offset=[0.05, -0.02, 0.1], power=[2.2, 1.0, 0.125]),
       dict(slope=0.25, power=8.0, saturation=4.0), dict(slope=[1.5, 1.0, 0.75], offset=-0.01, saturation=1.7)]


def specs(objects):
    """objects: four lists of ids, overlapping"""
    return {
        "white_balance": dict(slope=[float(g) for g in grade_white_balance(3200)]),  # (the gains as the slope: what white_balance= makes of them)
        "global_full": dict(slope=[1.2, 1.0, 0.0], offset=[-0.01, 0.0, 0.02], power=[0.125, 2.2, 8.0], saturation=4.0),
        "saturation_0": dict(saturation=0.0, power=[1.0, 2.2, 1.0]),
        "one_region": dict(slope=[1.1, 1.0, 0.9], regions=[dict(objects=objects[0], amount=1.0, **OPS[0])]),
        "four_regions": dict(saturation=1.3, regions=[dict(objects=o, amount=a, **op) for o, a, op in zip(objects, (0.0, 0.5, 1.0, 0.5), OPS)]),
    }


def _masks(r, spec):
    regions = spec.get("regions", ())
    if not regions:
        return None
    return np.ascontiguousarray(np.stack([r.matte_mask(reg["objects"])[0] for reg in regions], -1))


def check(r, spec, what, front=None):
    """grade() against grade_pixels word for word and against the binary64 restatement within its allowance"""
    front = front or {}
    F = r.lens(aperture=0.0, **front) if front else r.radiance()  # (aperture 0: the frame the stages in front leave)
    P = F32(r.passes)
    got = r.grade(**front, **spec)
    with np.errstate(all="ignore"):
        m = (F[..., :3] / P).astype(F32)
    masks = _masks(r, spec)
    host = grade_pixels(m, masks, **spec)
    cnt = np.isfinite(m).all(-1)
    with np.errstate(all="ignore"):
        want = np.where(cnt[..., None], (host * P).astype(F32), F[..., :3])
    assert np.array_equal(bits(got[..., :3]), bits(want)), (what, int((bits(got[..., :3]) != bits(want)).sum()))
    assert np.array_equal(bits(got[..., 3]), bits(F[..., 3])), what
    masks64 = None
    if masks is not None:
        t = r.matte()
        masks64, masks32 = masks_of(t["ids"], t["counts"], t["samples"], fill(spec)["regions"])
        assert np.array_equal(bits(masks32), bits(masks)), what  # kajo_hip_matte_mask's words, from the tables in integers
    ref = restate64(spec, m, masks64)
    c = ref["ranged"]
    err = np.abs(got[..., :3].astype(F64) / float(P) - ref["out64"])[c]
    # (the scaling by P and back: one more rounding of the result)
    allowance = ref["allowance"][c] + 2.0 ** -24 * np.abs(ref["out64"][c])
    share = float(np.max(np.where(err > 0, err / allowance, 0.0), initial=0.0))
    SEEN["share"] = max(SEEN["share"], share)
    print("%s: largest share of the allowance %.4f (so far %.4f), %d of %d pixels" % (what, share, SEEN["share"], c.sum(), c.size))
    assert (err <= allowance).all(), (what, share)
    return got


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_grade_is_grade_pixels_word_for_word(scenes, shape, build):
    W, H = shape
    sc = scenes["spheres_a169"]
    n = sc.n_planes + sc.n_spheres
    objects = [[n], [n - 1, n], [0, 1, 2], list(range(1, n + 1))[:16]]
    with HipRenderer(sc, W, H, spp=4, aov=True, matte=True, **BUILDS[build]) as r:
        r.render(PASSES)
        for name, spec in specs(objects).items():
            check(r, spec, "%dx%d %s %s" % (W, H, build, name))
        if shape == (41, 23):
            check(r, specs(objects)["four_regions"], "behind despeckle and denoise", front=dict(despeckle=dict(), denoise=dict(iterations=2)))


def test_mirrors_select_the_object_seen_in_them(scenes):
    """a grid of 60 spheres in the room of spheres.json, whose back wall is a mirror, with aov_specular: the tables name the object seen
    IN the mirror, and a region regrades it there too"""
    base = scenes["spheres_a169"]
    sc = stress_scene(base, 60, 3, seed=11)
    n = sc.n_planes + sc.n_spheres
    objects = [[sc.n_planes + 5], [sc.n_planes + k for k in range(1, 17)], [0], [n, n - 1, n - 2]]
    for build in ("exact", "strict"):
        with HipRenderer(sc, 130, 70, spp=4, aov=True, aov_specular=True, matte=True, **BUILDS[build]) as r:
            r.render(2)
            for name in ("one_region", "four_regions"):
                check(r, specs(objects)[name], "grid60 %s %s" % (build, name))
            covered = r.matte_mask(objects[1])[0]
            assert 0 < (covered > 0).mean() < 1


def test_pixels_that_do_not_count_keep_their_bits_and_reach_no_neighbour(scenes):
    """NaN, +-Inf pixels written into the accumulation come out with their bits; negative ones follow the rule (max lifts them to 0) and
    keep their bits in the identity case; every other pixel is what it is without them"""
    sc = scenes["spheres_a169"]
    W, H = 41, 23
    n = sc.n_planes + sc.n_spheres
    spec = specs([[n], [n - 1, n], [0, 1, 2], [1, 2, 3]])["four_regions"]
    with HipRenderer(sc, W, H, spp=4, exact=True, aov=True, matte=True) as r:
        r.render(PASSES)
        clean = r.radiance()
        graded = r.grade(**spec)
        bad = clean.copy()
        spots = {(0, 0): [np.nan, 1, 1], (5, 7): [1, np.inf, 2], (22, 40): [3, 1, -np.inf], (10, 10): [-4.0, 2.0, -0.5], (11, 30): [np.nan] * 3}
        for (y, x), v in spots.items():
            bad[y, x, :3] = F32(v)
        bad[3, 3, 3] = np.nan  # (.w is carried, never read)
        _upload(r, bad, PASSES)
        got = check(r, spec, "poisoned")
        touched = np.zeros((H, W), bool)
        for (y, x) in spots:
            touched[y, x] = True
        assert np.array_equal(bits(got[~touched][:, :3]), bits(graded[~touched][:, :3]))
        for (y, x), v in spots.items():
            if not np.isfinite(v).all():
                assert np.array_equal(bits(got[y, x]), bits(bad[y, x])), (y, x)
        # under an op without saturation the rule lifts a negative channel to 0 (the slope keeps its sign, the max cuts it)
        lifted = r.grade(slope=[0.5, 2.0, 0.25])
        assert np.array_equal(bits(lifted[10, 10, :3]), bits(F32([0.0, F32(F32(F32(2.0) / F32(PASSES)) * F32(2.0)) * F32(PASSES), 0.0])))
        assert np.array_equal(bits(r.grade()), bits(bad))  # the identity case: the source itself, negative channels included


def test_masks_compose_as_grade_pixels_orders_them(scenes):
    sc = scenes["spheres_a169"]
    W, H = 65, 9
    n = sc.n_planes + sc.n_spheres
    with HipRenderer(sc, W, H, spp=4, exact=True, aov=True, matte=True) as r:
        r.render(PASSES)
        glob = dict(slope=[1.3, 1.0, 0.8], saturation=0.8)
        base = r.grade(**glob)
        # a pixel with mask 0 in every region is the global-only result bit for bit
        regions = [dict(objects=[n], **OPS[1]), dict(objects=[n - 1], **OPS[3])]
        got = r.grade(regions=regions, **glob)
        none = (r.matte_mask([n])[0] == 0) & (r.matte_mask([n - 1])[0] == 0)
        assert none.any() and not none.all()
        assert np.array_equal(bits(got[none]), bits(base[none])) and not np.array_equal(bits(got[~none]), bits(base[~none]))
        # a region of every object with amount 1: the global grade composed with the op, in grade_pixels' own order
        every = list(range(0, n + 1))
        assert len(every) <= 16
        got = r.grade(regions=[dict(objects=every, **OPS[3])], **glob)
        mask = r.matte_mask(every)[0]
        t = r.matte()
        assert (t["dropped"] == 0).all() and (mask == 1).all()
        P = F32(r.passes)
        m = (base[..., :3] / P).astype(F32)
        # (c of the global op is not (c P) / P in general: compose on the means the stage itself had)
        mean = (r.radiance()[..., :3] / P).astype(F32)
        c = grade_pixels(mean, **glob)
        want = grade_pixels(c, np.ones((H, W, 1), F32), regions=[dict(objects=every, **OPS[3])])
        assert np.array_equal(bits(got[..., :3]), bits((want * P).astype(F32)))
        del m


TONES = [dict(curve="reinhard"), dict(curve="aces", auto_exposure=True)]


def test_identity_and_null_are_the_existing_calls(scenes):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 100, 75, spp=4, exact=True, aov=True) as r:
        r.render(2)
        assert np.array_equal(bits(r.grade()), bits(r.radiance()))
        ds, dn, gl, lc, ln = dict(), dict(iterations=2), dict(strength=0.2), dict(iterations=2), dict(aperture=0.05)
        vw = dict(out_w=50, out_h=37)
        for tone in TONES:
            for stages in (dict(), dict(despeckle=ds), dict(denoise=dn, glare=gl), dict(lens=ln), dict(view=vw),
                           dict(despeckle=ds, denoise=dn, lens=ln, glare=gl, local=lc, view=vw)):
                img, s = r.present(grade=dict(), **stages, **tone)
                want, s_want = r.present(**stages, **tone)
                assert np.array_equal(img, want) and bits(F32([s]))[0] == bits(F32([s_want]))[0], (tone, stages)
        img, res = r.present(grade=dict(), meter=dict(auto_white=True), glare=gl, curve="reinhard")
        want, res_want = r.present(meter=dict(auto_white=True), glare=gl, curve="reinhard")
        assert np.array_equal(img, want) and res == res_want
        # grade == NULL: kajo_hip_present_view_argb8 itself
        L = capi.lib()
        t, v = r._tone_params(curve="reinhard"), r._view_params(**vw)
        for view in (None, v):
            shape = (75, 100) if view is None else (37, 50)
            a, b = np.empty(shape, np.uint32), np.empty(shape, np.uint32)
            ref = lambda p: None if p is None else C.byref(p)
            capi.check(L.kajo_hip_present_grade_argb8(r._h, None, None, None, None, None, None, None, C.byref(t), ref(view),
                                                      a.ctypes.data_as(C.c_void_p), None))
            capi.check(L.kajo_hip_present_view_argb8(r._h, None, None, None, None, None, None, C.byref(t), ref(view),
                                                     b.ctypes.data_as(C.c_void_p), None))
            assert np.array_equal(a, b)
    # without regions the handle needs no AOVs
    with HipRenderer(sc, 64, 48, spp=4, exact=True) as plain:
        plain.render(1)
        assert np.array_equal(plain.present(grade=dict())[0], plain.argb8())
        assert not np.array_equal(plain.present(grade=dict(saturation=0.0))[0], plain.argb8())


def test_chain_is_the_chain_run_by_hand(scenes):
    """present(grade=G, lens, glare, local, **tone) = the chain over kajo_hip_grade's own frame written into a twin's accumulation"""
    sc = scenes["spheres_a169"]
    n = sc.n_planes + sc.n_spheres
    G = dict(white_balance=grade_white_balance(4000), saturation=1.4, regions=[dict(objects=[n], slope=0.3), dict(objects=[n - 1], power=2.2)])
    gl, lc, ln = dict(levels=4, strength=0.25), dict(iterations=3, compression=0.5), dict(aperture=0.06, focus_distance=6.0)
    kw = dict(spp=4, exact=True, aov=True, matte=True)
    with HipRenderer(sc, 130, 70, **kw) as r, HipRenderer(sc, 130, 70, **kw) as twin:
        r.render(3)
        twin.render(3)  # (the twin's AOVs are the handle's: the lens reads them)
        for front in (dict(), dict(despeckle=dict(factor=2.0, floor=0.01), denoise=dict(iterations=2))):
            frame = r.grade(**front, **G)
            _upload(twin, frame, 3)
            for behind in (dict(), dict(lens=ln, glare=gl), dict(glare=gl, local=lc), dict(view=dict(out_w=65, out_h=35))):
                for tone in TONES:
                    img, s = r.present(grade=G, **front, **behind, **tone)
                    want, s_want = twin.present(**behind, **tone)
                    assert np.array_equal(img, want) and bits(F32([s]))[0] == bits(F32([s_want]))[0], (front, behind, tone)
                    assert not np.array_equal(img, r.present(**front, **behind, **tone)[0])
            img, res = r.present(grade=G, meter=dict(percentile=0.4), glare=gl, **front, curve="reinhard")
            want, res_want = twin.present(meter=dict(percentile=0.4), glare=gl, curve="reinhard")
            assert np.array_equal(img, want) and res == res_want, front


def test_repeatable(scenes):
    sc = scenes["spheres_a169"]
    n = sc.n_planes + sc.n_spheres
    A = specs([[n], [n - 1, n], [0, 1, 2], [1, 2, 3]])["four_regions"]
    B = dict(saturation=0.2, regions=[dict(objects=[1], slope=2.0)])
    kw = dict(spp=4, exact=True, aov=True, matte=True)
    with HipRenderer(sc, 130, 70, **kw) as r, HipRenderer(sc, 130, 70, **kw) as twin:
        r.render(2)
        twin.render(2)
        a = r.grade(**A)
        assert np.array_equal(bits(a), bits(r.grade(**A))) and np.array_equal(bits(a), bits(twin.grade(**A)))
        b = r.grade(**B)
        assert not np.array_equal(bits(a), bits(b))
        assert np.array_equal(bits(a), bits(r.grade(**A))) and np.array_equal(bits(b), bits(twin.grade(**B)))
        r.radiance()  # composes the float frame: the calls now read it, row-major
        assert np.array_equal(bits(a), bits(r.grade(**A)))


def _grade_gathered(root, gathered, d, grade, g, tone, v=None):
    import torch
    n = root.width * root.height if v is None else v.outW * v.outH
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    ref = lambda p: None if p is None else C.byref(p)
    capi.check(capi.lib().kajo_hip_present_grade_gathered_argb8_device(root._h, src, ref(d), ref(grade), ref(g), None, None, C.byref(tone), ref(v),
                                                                       C.c_void_p(out.data_ptr()), None))
    root.wait()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape((root.height, root.width) if v is None else (v.outH, v.outW))


@pytest.mark.parametrize("tile", [(64, 16), (32, 8)], ids=["tile64x16", "tile32x8"])
def test_the_image_does_not_depend_on_the_owners(scenes, tile):
    from test_hip_tonemap import _gathered
    from test_hip_aov_tiled import _close, _compose, _render, _tiled
    sc = scenes["spheres_a169"]
    n = sc.n_planes + sc.n_spheres
    W, H = 130, 70
    G = dict(white_balance=grade_white_balance(3200), power=[1.0, 2.2, 1.0], saturation=1.5)
    R = dict(G, regions=[dict(objects=[n], slope=0.3), dict(objects=[n - 1, 1], power=2.2, amount=0.5)])
    gl, tone = dict(levels=3, strength=0.2), dict(curve="reinhard")
    with HipRenderer(sc, W, H, spp=4, exact=True, tile=tile) as r:
        r.render(3)
        g, t, d = r._glare_params(**gl), r._tone_params(**tone), r._despeckle_params()
        v = r._view_params(out_w=65, out_h=35)
        want = r.present(grade=G, glare=gl, despeckle=dict(), **tone)[0]
        want_v = r.present(grade=G, glare=gl, view=dict(out_w=65, out_h=35), **tone)[0]
        assert np.array_equal(_grade_gathered(r, None, d, grade_params(**G), g, t), want)
        assert np.array_equal(_grade_gathered(r, None, None, grade_params(**G), g, t, v), want_v)
        with pytest.raises(capi.KajoError) as e:
            _grade_gathered(r, None, None, grade_params(**R), g, t)
        assert e.value.code == capi.KAJO_E_INVALID and "coverage tables" in str(e.value)
    for count in (2, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile=tile, tile_index=k, tile_count=count) for k in range(count)]
        try:
            for o in owners:
                o.render(3)
            gathered = _gathered(owners)
            assert np.array_equal(_grade_gathered(owners[0], gathered, d, grade_params(**G), g, t), want), count
            assert np.array_equal(_grade_gathered(owners[0], gathered, None, grade_params(**G), g, t, v), want_v), count
        finally:
            for o in owners:
                o.close()
    # regions: the root of three tiled owners after compose + compose_aov is one handle
    kw = dict(spp=4, seed=0o715517, tile=tile, aov=True, matte=True, exact=True)
    with HipRenderer(sc, W, H, **kw) as one:
        _render([one])
        frame, img = one.grade(**R), one.present(grade=R, glare=gl, **tone)[0]
    owners = _tiled(sc, W, H, tile, 3, dict(exact=True), matte=True)
    try:
        _render(owners)
        with pytest.raises(capi.KajoError) as e:
            owners[0].grade(**R)
        assert e.value.code == capi.KAJO_E_STATE  # tiled, before compose_aov
        keep = _compose(owners)
        assert np.array_equal(bits(owners[0].grade(**R)), bits(frame))
        assert np.array_equal(owners[0].present(grade=R, glare=gl, **tone)[0], img)
        del keep
    finally:
        _close(owners)


def _code(call):
    with pytest.raises(capi.KajoError) as e:
        call()
    return e.value.code


def test_refusals_and_states_on_a_device(scenes):
    sc = scenes["spheres_a43"]
    n = sc.n_planes + sc.n_spheres
    R = dict(regions=[dict(objects=[1], slope=2.0)])
    every = lambda r: (lambda: r.grade(**R), lambda: r.present(grade=R))
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True) as plain:  # no matte flag
        plain.render(1)
        for call in every(plain):
            assert _code(call) == capi.KAJO_E_STATE
        assert "matte flag" in capi.lib().kajo_hip_last_error().decode()
        plain.grade(saturation=0.5)  # the global op needs no tables
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True, matte=True) as r:
        for call in every(r) + (lambda: r.grade(saturation=0.5),):
            assert _code(call) == capi.KAJO_E_STATE  # nothing rendered
        assert "nothing rendered" in capi.lib().kajo_hip_last_error().decode()
        r.render(1)
        assert _code(lambda: r.grade(regions=[dict(objects=[n + 1])])) == capi.KAJO_E_INVALID
        assert "object id out of range" in capi.lib().kajo_hip_last_error().decode()
        r.grade(regions=[dict(objects=[n])])
        assert _code(lambda: r.grade(saturation=9.0)) == capi.KAJO_E_INVALID
        p = grade_params(**R)
        assert capi.lib().kajo_hip_grade(r._h, None, None, C.byref(p), None) == 0  # radiance may be NULL
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True, matte=True, aov_tiled=True) as t:
        t.render(1)
        for call in every(t):
            assert _code(call) == capi.KAJO_E_STATE  # before compose_aov
        t.grade(saturation=0.5)
        t.compose_aov()
        t.grade(**R)
        t.render(1)
        for call in every(t):
            assert _code(call) == capi.KAJO_E_STATE  # a later render
    with HipRenderer(sc, 64, 48, spp=4, exact=True, aov=True, matte=True, aov_tiled=True, tile_index=1, tile_count=2) as part:
        part.render(1)
        for call in every(part) + (lambda: part.grade(saturation=0.5),):
            assert _code(call) == capi.KAJO_E_STATE  # a share of the frame, nothing composed


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_the_stage_leaves_the_handle_as_it_was(scenes, build):
    sc = scenes["spheres_a43"]
    kw = dict(spp=4, aov=True, matte=True, counters=True, **BUILDS[build])
    R = dict(saturation=1.5, regions=[dict(objects=[1, 2], slope=2.0, power=2.2), dict(objects=[3], saturation=0.0, amount=0.5)])
    with HipRenderer(sc, 100, 75, **kw) as a, HipRenderer(sc, 100, 75, **kw) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        a.grade()
        a.grade(**R)
        a.grade(denoise=dict(iterations=2), despeckle=dict(), white_balance=grade_white_balance(2800, 0.2))
        a.present(grade=R, curve="aces", auto_exposure=True)
        a.present(grade=R, lens=dict(), glare=dict(), local=dict(metered=True), meter=dict(auto_white=True), denoise=dict(iterations=3),
                  view=dict(out_w=50, out_h=38), curve="reinhard")
        _grade_gathered(a, None, None, grade_params(saturation=0.3), None, a._tone_params("reinhard"))
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
        assert np.array_equal(bits(a.grade(**R)), bits(b.grade(**R)))


# -- the driver ----------------------------------------------------------------------------------------------------------------------

SCENE = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
DRIVER = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "--json"]


@pytest.fixture(scope="module")
def driver_reference():
    """caustics 96x54, 2 passes, through the C ABI: the images of the chains the driver is asked for"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    n = sc.n_planes + sc.n_spheres
    with HipRenderer(sc, 96, 54, exact=True, aov=True, matte=True) as r:
        r.render(2)
        acc = r.radiance()
        G = dict(white_balance=grade_white_balance(3200), regions=[dict(objects=[1, 2], slope=[2.0, 0.5, 0.5], amount=0.5),
                                                                   dict(objects=[n], saturation=0.0, power=2.2)])
        px = r.present(grade=G, glare=dict(strength=0.1), curve="aces")[0]
        plain = r.present(glare=dict(strength=0.1), curve="aces")[0]
        glob = r.present(grade=dict(slope=[1.5, 1.0, 0.5], offset=[0.0, 0.01, 0.0], power=[1.0, 2.2, 1.0], saturation=1.5), glare=dict(strength=0.1),
                         curve="aces")[0]
        mean = acc[20, 30, :3]
        at = r.present(grade=dict(white_balance=grade_neutral(mean)), glare=dict(strength=0.1), curve="aces")[0]
        small = r.present(grade=G, glare=dict(strength=0.1), view=dict(out_w=48, out_h=27), curve="aces")[0]
        slope = [float(F32(g)) for g in grade_white_balance(3200)]
    assert len({px.tobytes(), plain.tobytes(), glob.tobytes(), at.tobytes()}) == 4
    return dict(acc=acc, px=px, plain=plain, glob=glob, at=at, small=small, n=n, slope=slope)


def _run_driver(tmp_path, extra):
    out = str(tmp_path / "o.png")
    p = subprocess.run(DRIVER + ["-o", out, "--glare", "0.1", "--tonemap", "aces"] + extra + [SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return read_png(out), json.loads(p.stdout.strip().splitlines()[-1])


def _same_png(png, argb):
    return all(np.array_equal(png[..., k], (argb >> shift) & 255) for k, shift in enumerate((16, 8, 0)))


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("owners", ["1", "3-on-one-device-tiled"])
def test_driver_writes_the_c_abi_s_image(tmp_path, driver_reference, owners):
    """kajo_render --white-balance 3200 --grade-region ... writes the PNG HipRenderer.present gives on the same frame; --json reports the
    slope; --raw stays the accumulation; without the options the plain PNG"""
    gpus = {"1": ["--gpus", "1"], "3-on-one-device-tiled": ["--gpus", "3", "--same-device", "--aov-tiled"]}[owners]
    ref = driver_reference
    raw = str(tmp_path / "o.raw")
    regions = ["--grade-region", "1,2:slope=2,0.5,0.5:amount=0.5", "--grade-region", "%d:saturation=0:power=2.2" % ref["n"]]
    png, stats = _run_driver(tmp_path, gpus + ["--raw", raw, "--white-balance", "3200"] + regions)
    assert np.array_equal(bits(np.fromfile(raw, np.float32).reshape(54, 96, 4)), bits(ref["acc"]))
    assert _same_png(png, ref["px"])
    assert [F32(v) for v in stats["grade_slope"]] == [F32(v) for v in ref["slope"]] and stats["grade_regions"] == 2
    assert stats["grade_white_balance_kelvin"] == 3200
    png, stats = _run_driver(tmp_path, gpus if owners == "1" else ["--gpus", "3", "--same-device"])
    assert _same_png(png, ref["plain"]) and "grade_slope" not in stats
    if owners == "1":
        png, _ = _run_driver(tmp_path, gpus + ["--white-balance", "3200", "--output-size", "48x27"] + regions)
        assert _same_png(png, ref["small"])
    else:
        # the global op needs no mattes: any number of owners, nothing tiled
        png, stats = _run_driver(tmp_path, ["--gpus", "3", "--same-device", "--grade-slope", "1.5,1,0.5", "--grade-offset", "0,0.01,0", "--grade-power",
                                            "1,2.2,1", "--grade-saturation", "1.5"])
        assert _same_png(png, ref["glob"]) and stats["grade_saturation"] == 1.5 and stats["grade_regions"] == 0
        png, stats = _run_driver(tmp_path, ["--gpus", "3", "--same-device", "--white-balance-at", "30,20"])
        assert _same_png(png, ref["at"])
