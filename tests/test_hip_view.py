"""The view (include/kajo_hip.h "The view", kajo_hip_view_argb8, kajo_hip_present_view_*; kajo_amd/csrc/view.hip) on the GPU.

The kernels are held to tests/view_replay.py WORD FOR WORD: the restatement uses the library's own weight rows and tables and sums in
the definition's order, so there is no tolerance anywhere in this file. Synthetic images go through kajo_hip_view_argb8, which needs
no pass rendered; the chain entry must equal the stage applied to the chain's own image; the gathered twin must give the one-handle
image for any number of owners; and the calls must leave the handle as a twin that never ran them."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from framelib import bits, read_png
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from view_replay import FILTERS, restate, test_images as images_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
SHAPES = [(1, 1), (2, 1), (7, 5), (41, 23), (65, 9), (130, 70)]


def _views(W, H):
    """(out_w, out_h, rect) for a W x H source. One output pixel takes the whole frame where that is a minification of at most
    KAJO_VIEW_MAX_SCALE = 64; the wider frames (65x9, 130x70) are refused there by the definition's own limit
    (test_refusals_that_need_the_frame), so theirs is the largest rectangle that is not: 64 source pixels along the long axis"""
    one = None if max(W, H) <= 64 else (0.5, 0.0, min(W, 64.5), min(H, 64.0))
    out = [(1, 1, one), (W, H, (0.25, 0.5, W - 0.5, H - 0.25)), (math.ceil(W / 2), math.ceil(H / 2), None), (2 * W + 1, 2 * H + 1, None)]
    if (W / 65 <= 64 and H / 5 <= 64):
        out.append((65, 5, None))  # one column past a workgroup's width
    if (W, H) == (130, 70):
        out.append((16, 9, None))  # a ratio of about 8: LANCZOS3 rows of 49 taps, past the LDS form's 16
    return out


def _check(r, images, views):
    for filter in FILTERS:
        for out_w, out_h, rect in views:
            for name, img in images.items():
                got = r.view(img, out_w=out_w, out_h=out_h, rect=rect, filter=filter)
                want = restate(img, out_w, out_h, rect, filter)
                assert got.shape == (out_h, out_w) and (got >> 24 == 255).all(), (name, filter, out_w, out_h)
                assert np.array_equal(got, want), (name, filter, out_w, out_h, rect, int((got != want).sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_synthetic_images_match_the_restatement_word_for_word(scenes, shape):
    W, H = shape
    with HipRenderer(scenes["spheres_a1"], W, H, spp=1) as r:  # (nothing is rendered: the stage needs no pass)
        _check(r, images_of(W, H), _views(W, H))


@pytest.mark.parametrize("shape", [(4096, 1), (1, 4096)], ids=["4096x1", "1x4096"])
def test_the_largest_scale_and_the_longest_rows(scenes, shape):
    """4096 -> 64 along one axis: scale 64, LANCZOS3 rows of KAJO_VIEW_MAX_TAPS = 384 taps; the handle is created at that shape"""
    W, H = shape
    with HipRenderer(scenes["spheres_a1"], W, H, spp=1) as r:
        _check(r, images_of(W, H), [(max(W // 64, 1), max(H // 64, 1), None)])


def test_cases_that_must_leave_bits_alone(scenes):
    W, H = 41, 23
    images = images_of(W, H)
    img = images["random"] & np.uint32(0x7FFFFFFF)  # (an alpha that is not 255: the copy case returns the words it was given)
    with HipRenderer(scenes["spheres_a1"], W, H, spp=1) as r, HipRenderer(scenes["spheres_a1"], W, H, spp=1) as twin:
        for filter in FILTERS:  # the copy case: the source words, under any filter
            assert np.array_equal(r.view(img, filter=filter), img), filter
            assert np.array_equal(r.view(img, out_w=W, out_h=H, rect=(0, 0, W, H), filter=filter), img), filter
        a = dict(out_w=20, out_h=11, filter="lanczos3")
        b = dict(out_w=20, out_h=11, rect=(3.5, 2.25, 30.0, 20.0), filter="triangle")
        first = r.view(img, **a)
        assert np.array_equal(r.view(img, **a), first)  # a second call (the cached rows)
        assert np.array_equal(twin.view(img, **a), first)  # a twin handle
        other = r.view(img, **b)  # other parameters: their own rows, then the first ones again
        assert np.array_equal(other, restate(img, 20, 11, b["rect"], "triangle")) and not np.array_equal(other, first)
        assert np.array_equal(r.view(img, **a), first)
        assert np.array_equal(r.view(images["checker"], **a), restate(images["checker"], 20, 11, None, "lanczos3"))  # same rows, new image
        grown = r.view(img, out_w=83, out_h=47, filter="area")  # a larger output: the scratch grows
        assert np.array_equal(grown, restate(img, 83, 47, None, "area"))
        assert np.array_equal(r.view(img, **a), first)


def test_refusals_that_need_the_frame(scenes):
    """the checks against W and H fall behind the null handle (tests/test_view_cpu.py): here they are, before any device work"""
    with HipRenderer(scenes["spheres_a1"], 130, 70, spp=1) as r:
        img = images_of(130, 70)["checker"]
        for kw, message in ((dict(rect=(0, 0, 130.5, 70)), "view rectangle must lie inside the frame"),
                            (dict(rect=(0, 0, 130, 71)), "view rectangle must lie inside the frame"),
                            (dict(out_w=2, out_h=70), "view minification must be at most 64"),
                            (dict(out_w=130, out_h=1), "view minification must be at most 64")):
            with pytest.raises(capi.KajoError, match=message.replace("(", r"\(")) as e:
                r.view(img, **kw)
            assert e.value.code == capi.KAJO_E_INVALID
        with pytest.raises(capi.KajoError, match="nothing rendered|no pass|rendered"):  # the chain entry then meets the handle's state
            r.present(view=dict(out_w=65, out_h=35))
        assert r.view(img, out_w=3, out_h=2).shape == (2, 3)  # (scale 43: accepted)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_chain_is_the_stage_over_the_chain_s_own_image(scenes, build):
    with HipRenderer(scenes["spheres_a43"], 100, 75, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(3)
        chains = (dict(curve="aces"), dict(denoise=dict(iterations=2), glare=dict(levels=3, strength=0.2), curve="reinhard"))
        for chain in chains:
            plain, scale = r.present(**chain)
            for view in (dict(out_w=50, out_h=38), dict(out_w=64, out_h=48, rect=(10.5, 7.25, 90.0, 70.0), filter="lanczos3"),
                         dict(out_w=201, out_h=151, filter="triangle"), dict(out_w=25, out_h=19, filter="nearest")):
                got, got_scale = r.present(view=view, **chain)
                assert got.shape == (view["out_h"], view["out_w"])
                assert np.array_equal(got, r.view(plain, **view)), (build, view)
                assert got_scale == scale
            same, _ = r.present(view=dict(), **chain)  # the copy case of the chain
            assert np.array_equal(same, plain)
        # view=None is kajo_hip_present_lens_argb8's image: through the C ABI with a NULL view
        t = r._tone_params(curve="aces")
        out = np.zeros((75, 100), np.uint32)
        capi.check(capi.lib().kajo_hip_present_view_argb8(r._h, None, None, None, None, None, None, C.byref(t), None,
                                                          out.ctypes.data_as(C.c_void_p), None))
        assert np.array_equal(out, r.present(curve="aces")[0])


def test_supersampling_through_the_chain(scenes):
    """--supersample 2's two sizes: the chain at 96x54, the AREA view down to 48x27 -- four pixels of equal weight each"""
    with HipRenderer(scenes["spheres_a169"], 96, 54, spp=4, exact=True) as r:
        r.render(2)
        big, _ = r.present(curve="aces")
        small, _ = r.present(view=dict(out_w=48, out_h=27, filter="area"), curve="aces")
        assert np.array_equal(small, restate(big, 48, 27, None, "area"))
        assert not np.array_equal(small, big[::2, ::2])


def _view_gathered(root, gathered, d, g, l, m, tone, v):
    """kajo_hip_present_view_gathered_argb8_device on `root` -> argb8"""
    import torch
    out = torch.zeros(v.outW * v.outH, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    ref = lambda p: None if p is None else C.byref(p)
    result = capi.KajoMeterResult()
    capi.check(capi.lib().kajo_hip_present_view_gathered_argb8_device(root._h, src, ref(d), ref(g), ref(l), ref(m), C.byref(tone), ref(v),
                                                                      C.c_void_p(out.data_ptr()), C.byref(result)))
    root.wait()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(v.outH, v.outW)


@pytest.mark.parametrize("tile", [(64, 16), (32, 8)], ids=["tile64x16", "tile32x8"])
def test_the_image_does_not_depend_on_the_owners(scenes, tile):
    from test_hip_tonemap import _gathered
    sc = scenes["spheres_a169"]
    W, H = 130, 70
    gl, tone = dict(levels=3, strength=0.2), dict(curve="reinhard")
    views = (dict(out_w=65, out_h=35), dict(out_w=48, out_h=27, rect=(1.5, 2.0, 120.25, 64.0), filter="lanczos3"), dict())
    with HipRenderer(sc, W, H, spp=4, exact=True, tile=tile) as r:
        r.render(3)
        want = [r.present(glare=gl, view=v, **tone)[0] for v in views]
        g, t = r._glare_params(**gl), r._tone_params(**tone)
        params = [r._view_params(**v) for v in views]
        for v, w in zip(params, want):
            assert np.array_equal(_view_gathered(r, None, None, g, None, None, t, v), w)
    for count in (2, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile=tile, tile_index=k, tile_count=count) for k in range(count)]
        try:
            for o in owners:
                o.render(3)
            gathered = _gathered(owners)
            for v, w in zip(params, want):
                assert np.array_equal(_view_gathered(owners[0], gathered, None, g, None, None, t, v), w), (count, v.outW)
        finally:
            for o in owners:
                o.close()


def test_the_stage_leaves_the_handle_as_it_was(scenes):
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, exact=True) as a, \
            HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, exact=True) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        a.view(images_of(100, 75)["random"], out_w=33, out_h=20, filter="lanczos3")
        a.present(view=dict(out_w=50, out_h=38), curve="aces")
        a.present(view=dict(out_w=201, out_h=151, filter="triangle"), denoise=dict(iterations=2), glare=dict(), curve="reinhard")
        _view_gathered(a, None, None, None, None, None, a._tone_params("reinhard"), a._view_params(out_w=50, out_h=38))
        assert a.counters()["kernelMs"] == ms
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert np.array_equal(a.argb8(), b.argb8())
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        ca, cb = a.counters(), b.counters()
        for key in ("passes", "launches", "paths", "traversals", "vertices"):
            assert ca[key] == cb[key], key
        assert ca["passes"] == 3
        a.render(2)
        b.render(2)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        assert a.counters()["passes"] == 5


def test_the_gathered_twin_enqueues_without_waiting(scenes):
    """On a caller's stream that is kept busy by a spinning kernel in front (no host sleep: the device spins), the parent's twin
    returns while the stream still has work pending -- and so does the view's twin, once its scratch stands (a first call with the same
    parameters): neither its cached rows, nor its intermediate, nor its frame make it wait. The image behind the spin is the image."""
    import torch
    W, H = 130, 70
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, exact=True) as r:
        r.render(2).wait()
        t, v = r._tone_params(curve="reinhard"), r._view_params(out_w=65, out_h=35, filter="lanczos3")
        want = _view_gathered(r, None, None, None, None, None, t, v)  # (allocates the scratch, uploads the rows)
        stream = torch.cuda.Stream()
        r.set_stream(stream.cuda_stream)
        out = torch.zeros(v.outW * v.outH, dtype=torch.int32, device="cuda")
        plain = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        L = capi.lib()
        try:
            with torch.cuda.stream(stream):
                torch.cuda._sleep(20_000_000)  # device time in front of the calls: hundreds of times what enqueueing them takes
            capi.check(L.kajo_hip_present_local_gathered_argb8_device(r._h, None, None, None, None, None, C.byref(t),
                                                                      C.c_void_p(plain.data_ptr()), None))
            parent_pending = not stream.query()
            capi.check(L.kajo_hip_present_view_gathered_argb8_device(r._h, None, None, None, None, None, C.byref(t), C.byref(v),
                                                                     C.c_void_p(out.data_ptr()), None))
            pending = not stream.query()
            stream.synchronize()
        finally:
            stream.synchronize()
            r.set_stream(None)
        assert parent_pending, "the spin ended before the parent's twin returned: the check below would show nothing"
        assert pending, "the view's twin waited for the stream"
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(v.outH, v.outW), want)


# -- the driver ----------------------------------------------------------------------------------------------------------------------

SCENE = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")


@pytest.fixture(scope="module")
def driver_reference():
    """caustics at 160x90, 2 passes, through the C ABI, computed once: the plain image, its 80x45 AREA view (what --output-size 80x45 and
    --supersample 2 -w 80 -h 45 must both write) and a cropped LANCZOS3 view"""
    from kajo_amd.scene import Scene
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    with HipRenderer(sc, 160, 90, exact=True) as r:
        r.render(2)
        plain, _ = r.present(curve="aces")
        small, _ = r.present(view=dict(out_w=80, out_h=45, filter="area"), curve="aces")
        crop, _ = r.present(view=dict(out_w=100, out_h=60, rect=(10.5, 5.0, 120.0, 80.25), filter="lanczos3"), curve="aces")
    return dict(plain=plain, small=small, crop=crop)


def _run_driver(tmp_path, name, args):
    out = str(tmp_path / name)
    p = subprocess.run([BIN, "-r", "hip", "--passes", "2", "--json", "--tonemap", "aces", "-o", out] + args + [SCENE], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    png = read_png(out)
    words = (png[..., 0].astype(np.uint32) << 16) | (png[..., 1].astype(np.uint32) << 8) | png[..., 2].astype(np.uint32) | np.uint32(0xFF000000)
    return words, json.loads(p.stdout.strip().splitlines()[-1]), open(out, "rb").read()


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("owners", ["1", "3-on-one-device"])
def test_driver_writes_the_c_abi_s_image(tmp_path, driver_reference, owners):
    gpus = {"1": ["--gpus", "1"], "3-on-one-device": ["--gpus", "3", "--same-device"]}[owners]
    ref = driver_reference
    got, stats, _ = _run_driver(tmp_path, "s.png", gpus + ["-w", "160", "-h", "90", "--output-size", "80x45"])
    assert got.shape == (45, 80) and np.array_equal(got, ref["small"])
    assert (stats["view_out_w"], stats["view_out_h"], stats["view_filter"], stats["view_scale_x"], stats["view_scale_y"]) == (80, 45, "area", 2.0, 2.0)
    assert (stats["width"], stats["height"]) == (160, 90)
    got, stats, _ = _run_driver(tmp_path, "c.png", gpus + ["-w", "160", "-h", "90", "--output-size", "100x60", "--view", "10.5,5,120,80.25",
                                                           "--view-filter", "lanczos3"])
    assert np.array_equal(got, ref["crop"]) and stats["view_filter"] == "lanczos3"
    assert np.float32(stats["view_scale_x"]) == np.float32(109.5 / 100)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_supersample_and_the_plain_image(tmp_path, driver_reference):
    ref = driver_reference
    got, stats, _ = _run_driver(tmp_path, "ss.png", ["-w", "80", "-h", "45", "--supersample", "2"])
    assert got.shape == (45, 80) and np.array_equal(got, ref["small"])
    assert (stats["width"], stats["height"], stats["view_out_w"], stats["view_out_h"], stats["view_filter"]) == (160, 90, 80, 45, "area")
    # without any of the new options: the frame's own image, and the same FILE as the whole frame viewed at its own size (the copy case)
    plain, stats, data = _run_driver(tmp_path, "p.png", ["-w", "160", "-h", "90"])
    assert np.array_equal(plain, ref["plain"]) and "view_out_w" not in stats
    same, _, same_data = _run_driver(tmp_path, "q.png", ["-w", "160", "-h", "90", "--output-size", "160x90"])
    assert data == same_data
