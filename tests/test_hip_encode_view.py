"""The float view (include/kajo_hip.h "The float view"; kajo_hip_encode_view, kajo_hip_encode_view_present and its gathered twin;
kajo_amd/csrc/encode_view.cpp) on the GPU. The two kernels are held WORD FOR WORD to tests/encode_view_replay.py's numpy restatement
over the library's weight rows, and to kajo_hip_encode_view_pixels, the same lines compiled for the host: no tolerance anywhere but the
constant-frame statement, which the header makes within one code. Frames are values written into the tile buffer and rendered frames,
at shapes that cross the 64-column and 4-row workgroup edges and the tile edges; rows of 384 taps over several chunks; the copy case;
the chain in the three numerics builds; one image for any number of owners; the gathered twin's asynchrony; what the stage leaves
alone; the driver's --encode-view file against the C ABI's words."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import read_png
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, encode_params, encode_view_pixels
import encode_view_replay as R
from test_hip_encode import upload, words

pytestmark = pytest.mark.gpu
F32 = np.float32
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
SHAPES = [(1, 1), (2, 1), (7, 5), (41, 23), (65, 9), (130, 70)]
FILTERS = ("nearest", "area", "triangle", "lanczos3")
CONFIGS = sorted(R.CONFIGS)


def frame_of(mean):
    """(H, W, 3) means -> (H, W, 4) sums of one pass (.w is never read)"""
    f = np.full(mean.shape[:2] + (4,), np.nan, F32)
    f[..., :3] = mean
    return f


def stage(r, config, out_w, out_h, rect, filt):
    e, tone = R.encode_kwargs(R.CONFIGS[config])
    return words(r.encode(e, view=dict(out_w=out_w, out_h=out_h, rect=rect, filter=filt), **tone))


def want_of(config, mean, out_w, out_h, rect, filt):
    """the replay's words and, beside them, the host twin's: the two must agree before either is held against the device"""
    cfg = R.CONFIGS[config]
    want = R.restate(cfg, mean, out_w, out_h, rect, filt).reshape(-1)
    e, tone = R.encode_kwargs(cfg)
    twin = encode_view_pixels(mean, e, dict(out_w=out_w, out_h=out_h, rect=rect, filter=filt), **tone).reshape(-1)
    assert want.dtype == twin.dtype and np.array_equal(want, twin), (config, filt, out_w, out_h)
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_stage_is_the_replay_word_for_word(scenes, shape):
    """random values over many binades with NaN, +-Inf, negatives, -0 and values above 65504 among them: every (format, transfer, flags) of
    the covering set under every filter, the output sizes in rotation, and every output size under every filter for one of them"""
    W, H = shape
    mean = R.frames(W, H)["wild"]
    sizes = R.out_sizes(W, H)
    names = sorted(sizes)
    cases = [(c, f, names[(i + j) % 4]) for i, c in enumerate(CONFIGS) for j, f in enumerate(FILTERS)]
    cases += [("rgba16_pq600_dither", f, n) for f in FILTERS for n in names]
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4) as r:
        upload(r, frame_of(mean), 1, (64, 16))
        for config, filt, name in dict.fromkeys(cases):
            out_w, out_h, rect = sizes[name]
            got = stage(r, config, out_w, out_h, rect, filt)
            want = want_of(config, mean, out_w, out_h, rect, filt)
            assert got.dtype == want.dtype and np.array_equal(got, want), (config, filt, name, np.nonzero(got != want)[0][:4])
        # ... and from the row-major frame the radiance reader composes
        r.radiance()
        out_w, out_h, rect = sizes["half_up"]
        assert np.array_equal(stage(r, "rgb10a2_srgb", out_w, out_h, rect, "lanczos3"), want_of("rgb10a2_srgb", mean, out_w, out_h, rect, "lanczos3"))


@pytest.mark.parametrize("shape", [(4096, 1), (1, 4096)], ids=lambda s: "%dx%d" % s)
def test_rows_of_384_taps_over_several_chunks(scenes, shape):
    """scale 64: LANCZOS3's rows have 384 taps and a workgroup's span takes several chunks; AREA's 64"""
    W, H = shape
    mean = R.frames(W, H)["wild"]
    out_w, out_h = (64, 1) if H == 1 else (1, 64)
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4) as r:
        upload(r, frame_of(mean), 1, (64, 16))
        for config, filt in (("rgba16_pq600_dither", "lanczos3"), ("rgba16f_scene", "area"), ("argb8_gamma22_dither", "triangle")):
            got = stage(r, config, out_w, out_h, None, filt)
            want = want_of(config, mean, out_w, out_h, None, filt)
            assert np.array_equal(got, want), (config, filt, np.nonzero(got != want)[0][:4])


def test_bright_pixels_constants_and_the_copy_case(scenes):
    """41x23: one bright pixel in the interior, on an edge and in a corner, word for word; constants within one code of the plain encode of
    a constant frame; the copy case returns kajo_hip_encode's words under any filter; NEAREST without dither gathers them"""
    W, H = 41, 23
    frames = R.frames(W, H)
    sizes = R.out_sizes(W, H)
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4) as r:
        for name in ("bright_interior", "bright_edge", "bright_corner"):
            upload(r, frame_of(frames[name]), 1, (64, 16))
            for config, filt, size in (("rgba16_linear", "lanczos3", "double_plus_1"), ("rgba16_pq600_dither", "lanczos3", "half_up"),
                                       ("rgba16f", "triangle", "same_frac"), ("argb8_gamma22_dither", "area", "half_up")):
                out_w, out_h, rect = sizes[size]
                got = stage(r, config, out_w, out_h, rect, filt)
                assert np.array_equal(got, want_of(config, frames[name], out_w, out_h, rect, filt)), (name, config, filt)
        for name in sorted(n for n in frames if n.startswith("const_")):
            upload(r, frame_of(frames[name]), 1, (64, 16))
            worst = 0
            for config in CONFIGS:
                cfg = R.CONFIGS[config]
                for filt, size in (("lanczos3", "half_up"), ("area", "double_plus_1"), ("triangle", "same_frac")):
                    out_w, out_h, rect = sizes[size]
                    got = stage(r, config, out_w, out_h, rect, filt)
                    assert np.array_equal(got, want_of(config, frames[name], out_w, out_h, rect, filt)), (name, config, filt)
                    flat = R.plain(cfg, np.broadcast_to(frames[name][0, 0], (out_h, out_w, 3)))
                    off = np.abs(R.channels(cfg, got.reshape(out_h, out_w)) - R.channels(cfg, flat)).max()
                    assert off <= 1, (name, config, filt, size)
                    worst = max(worst, int(off))
            print("%s: largest distance from the plain encode %d code(s)" % (name, worst))
        mean = frames["wild"]
        upload(r, frame_of(mean), 1, (64, 16))
        for config in CONFIGS:
            e, tone = R.encode_kwargs(R.CONFIGS[config])
            plain = words(r.encode(e, **tone))
            assert np.array_equal(plain, R.plain(R.CONFIGS[config], mean).reshape(-1))
            for filt in FILTERS:
                assert np.array_equal(stage(r, config, W, H, None, filt), plain), (config, filt)
                assert np.array_equal(stage(r, config, W, H, (0.0, 0.0, float(W), float(H)), filt), plain), (config, filt)
            if not e["dither"]:
                out_w, out_h, rect = sizes["half_up"]
                fx = np.floor((np.arange(out_w) + 0.5) * (W / out_w)).astype(int)
                fy = np.floor((np.arange(out_h) + 0.5) * (H / out_h)).astype(int)
                gathered = plain.reshape(H, W)[fy][:, fx].reshape(-1)
                assert np.array_equal(stage(r, config, out_w, out_h, rect, "nearest"), gathered), config


def test_a_second_call_a_twin_handle_and_a_change_of_parameters_and_back(scenes):
    W, H = 65, 9
    mean = R.frames(W, H)["random"]
    a_args = ("rgba16_pq600_dither", 33, 5, None, "lanczos3")
    b_args = ("rgb10a2_srgb", 131, 19, (0.25, 0.25, W - 0.25, H - 0.25), "area")
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4) as r, HipRenderer(scenes["spheres_a43"], W, H, spp=4) as twin:
        upload(r, frame_of(mean), 1, (64, 16))
        upload(twin, frame_of(mean), 1, (64, 16))
        a = stage(r, *a_args)
        assert np.array_equal(a, want_of(a_args[0], mean, *a_args[1:]))
        assert np.array_equal(stage(r, *a_args), a)
        assert np.array_equal(stage(twin, *a_args), a)
        b = stage(r, *b_args)
        assert np.array_equal(b, want_of(b_args[0], mean, *b_args[1:]))
        assert np.array_equal(stage(r, *a_args), a) and np.array_equal(stage(r, *b_args), b)
        # the 8-bit view shares the rows and the intermediate: it gives what it gave, in between
        image = r.present()[0]
        v8 = r.present(view=dict(out_w=33, out_h=5, filter="lanczos3"))[0]
        assert np.array_equal(stage(r, *a_args), a)
        assert np.array_equal(r.present(view=dict(out_w=33, out_h=5, filter="lanczos3"))[0], v8) and np.array_equal(r.present()[0], image)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_chain_is_the_replay_over_the_frame_the_stages_in_front_leave(scenes, build):
    W, H, P = 96, 54, 3
    L = capi.lib()
    cfg = R.CONFIGS["rgba16_pq600_dither"]
    e, tone = R.encode_kwargs(cfg)
    view = dict(out_w=48, out_h=27, filter="area")
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(P)
        for front in (dict(), dict(denoise=dict(iterations=2), glare=dict(levels=4, strength=0.2))):
            with np.errstate(all="ignore"):
                radiance = r.glare(**front["glare"], denoise=front["denoise"]) if front else r.radiance()
                mean = (radiance[..., :3] / F32(P)).astype(F32)
            got, result = r.present(encode=e, view=view, **front, **tone)
            assert result is None and got.shape == (27, 48, 4)
            assert np.array_equal(words(got), R.restate(cfg, mean, 48, 27, None, "area").reshape(-1)), front
            # view=None: kajo_hip_encode_present's words
            ep, t = encode_params(**e), r._tone_params(**tone)
            d = r._denoise_params(**front["denoise"]) if front else None
            g = r._glare_params(**front["glare"]) if front else None
            ref = lambda p: None if p is None else C.byref(p)
            out = np.zeros(W * H, np.uint64)
            capi.check(L.kajo_hip_encode_view_present(r._h, None, ref(d), None, None, ref(g), None, None, C.byref(t), None, C.byref(ep),
                                                      out.ctypes.data_as(C.c_void_p), None))
            assert np.array_equal(out, words(r.present(encode=e, **front, **tone)[0])), front
            # with a meter the tone parameters are the host-patched ones
            m, res = r._meter_params(), capi.KajoMeterResult()
            v = r._view_params(**view)
            out = np.zeros(48 * 27, np.uint64)
            capi.check(L.kajo_hip_encode_view_present(r._h, None, ref(d), None, None, ref(g), None, C.byref(m), C.byref(t), C.byref(v), C.byref(ep),
                                                      out.ctypes.data_as(C.c_void_p), C.byref(res)))
            patched = capi.KajoToneParams()
            capi.check(L.kajo_hip_meter_tone(C.byref(res), C.byref(m), C.byref(t), C.byref(patched)))
            assert res.metered > 0 and patched.exposure != t.exposure
            metered = cfg[:6] + (patched.exposure, patched.white)
            assert np.array_equal(out, R.restate(metered, mean, 48, 27, None, "area").reshape(-1)), front
            assert not np.array_equal(out, words(got))


def _gathered_viewed(root, gathered, e, tone, view, guard=16):
    import torch
    ep, v = encode_params(**e), root._view_params(**view)
    per = 2 if ep.format in (capi.KAJO_ENCODE_RGBA16, capi.KAJO_ENCODE_RGBA16F) else 1
    n = v.outW * v.outH * per
    out = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    capi.check(capi.lib().kajo_hip_encode_view_present_gathered_device(root._h, src, None, None, None, None, None, C.byref(tone), C.byref(v),
                                                                       C.byref(ep), C.c_void_p(out.data_ptr()), None))
    root.wait()
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert (host[n:] == 0x5A5A5A5A).all()
    return np.ascontiguousarray(host[:n]).view(np.uint64 if per == 2 else np.uint32)


@pytest.mark.parametrize("tile", [(64, 16), (32, 8)], ids=["tile64x16", "tile32x8"])
def test_the_image_does_not_depend_on_the_owners(scenes, tile):
    from test_hip_tonemap import _gathered
    sc = scenes["spheres_a169"]
    W, H = 130, 70
    cases = [(dict(format="rgba16", transfer="pq", peak_nits=600.0, dither=True, dither_seed=3), dict(out_w=65, out_h=35, filter="area")),
             (dict(format="argb8", dither=True, dither_seed=9), dict(out_w=87, out_h=47, rect=(3.5, 2.25, 120.0, 66.5), filter="lanczos3"))]
    with HipRenderer(sc, W, H, spp=4, exact=True, tile=tile) as r:
        r.render(2)
        t = r._tone_params("reinhard", 0.5)
        want = [words(r.encode(e, view=v, curve="reinhard", exposure=0.5)) for e, v in cases]
        for (e, v), w in zip(cases, want):
            assert np.array_equal(_gathered_viewed(r, None, e, t, v), w), (e, v)
    for count in (2, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile=tile, tile_index=k, tile_count=count) for k in range(count)]
        try:
            for o in owners:
                o.render(2)
            gathered = _gathered(owners)
            for (e, v), w in zip(cases, want):
                assert np.array_equal(_gathered_viewed(owners[0], gathered, e, t, v), w), (count, e, v)
        finally:
            for o in owners:
                o.close()


def test_the_gathered_twin_enqueues_on_the_caller_s_stream_without_waiting(scenes):
    """tests/test_hip_streams.py's pattern: a spin on the caller's stream S, a render behind it, the twin behind that, once its scratch
    stands. The call returns while the spin runs, and after S alone is waited for the words are those of the frame rendered behind the
    spin."""
    import torch
    from test_hip_streams import Spin
    W, H = 96, 54
    e = dict(format="rgba16", transfer="pq", peak_nits=500.0, dither=True)
    view = dict(out_w=48, out_h=27, filter="lanczos3")
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r, HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as twin:
        S = torch.cuda.Stream()
        tone = r._tone_params("aces")
        twin.render(2)
        want = words(twin.encode(e, view=view, curve="aces"))
        r.set_stream(S.cuda_stream)
        r.render(1).wait()
        stale = _gathered_viewed(r, None, e, tone, view)  # (the warm-up: the rows, the table and the intermediate stand)
        ep, v = encode_params(**e), r._view_params(**view)
        out = torch.zeros(48 * 27 * 2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        try:
            spin = Spin(S)
            r.render(1)
            rendered = spin.running()
            capi.check(capi.lib().kajo_hip_encode_view_present_gathered_device(r._h, None, None, None, None, None, None, C.byref(tone), C.byref(v),
                                                                               C.byref(ep), C.c_void_p(out.data_ptr()), None))
            returned = spin.running()
            S.synchronize()
            got = out.cpu().numpy().view(np.uint64)
        finally:
            torch.cuda.synchronize()
            r.set_stream(None)
        assert not np.array_equal(stale, want), "the previous frame reads as the true one: the case would show nothing"
        assert rendered, "spin ended early, or kajo_hip_render waited for the stream"
        assert returned, "spin ended early, or the call waited for the stream: it was over when the call returned"
        assert np.array_equal(got, want)


def test_the_stage_leaves_the_handle_as_it_was(scenes):
    sc = scenes["spheres_a43"]
    kw = dict(spp=4, aov=True, counters=True, exact=True)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    with HipRenderer(sc, 100, 75, **kw) as a, HipRenderer(sc, 100, 75, **kw) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        before = a.argb8()
        for config in CONFIGS:
            stage(a, config, 50, 38, None, "lanczos3")
        a.present(encode=dict(format="rgba16", transfer="pq"), view=dict(out_w=201, out_h=151), denoise=dict(iterations=2), despeckle=dict(),
                  glare=dict(), meter=dict(), curve="reinhard")
        _gathered_viewed(a, None, dict(format="rgb10a2", dither=True), a._tone_params("aces"), dict(out_w=25, out_h=19))
        assert a.counters()["kernelMs"] == ms
        assert np.array_equal(a.argb8(), before) and np.array_equal(a.argb8(), b.argb8())
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        ca, cb = a.counters(), b.counters()
        for key in ("passes", "launches", "paths", "traversals", "vertices"):
            assert ca[key] == cb[key], key
        a.render(2)
        b.render(2)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance())) and a.counters()["passes"] == 5


def test_refusals_on_a_device(scenes):
    L = capi.lib()
    with HipRenderer(scenes["spheres_a43"], 64, 48, spp=4) as r:
        with pytest.raises(capi.KajoError) as e:
            r.encode(view=dict(out_w=32, out_h=24))
        assert e.value.code == capi.KAJO_E_STATE and "nothing rendered" in str(e.value)
        r.render(1)
        for view, text in ((dict(rect=(0.0, 0.0, 65.0, 48.0)), "view rectangle must lie inside the frame"), (dict(out_w=0), "view output size"),
                           (dict(filter=7), "unknown view filter")):
            with pytest.raises(capi.KajoError) as e:
                r.encode(view=view)
            assert e.value.code == capi.KAJO_E_INVALID and text in str(e.value), view
        p, t, v = encode_params(), r._tone_params(), r._view_params(out_w=32, out_h=24)
        assert L.kajo_hip_encode_view(r._h, C.byref(p), C.byref(t), C.byref(v), None) == 0  # dst may be NULL
        assert L.kajo_hip_encode_view_present_gathered_device(r._h, None, None, None, None, None, None, C.byref(t), C.byref(v), C.byref(p), None,
                                                              None) == capi.KAJO_E_INVALID


# -- the driver ----------------------------------------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
SCENE = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
DRIVER = [BIN, "-w", "80", "-h", "45", "-r", "hip", "--passes", "2", "--json", "--supersample", "2", "--tonemap", "aces", "--exposure", "0.5"]


@pytest.fixture(scope="module")
def driver_reference():
    """caustics rendered at 160x90, 2 passes, through the C ABI: the words the driver is asked for"""
    from kajo_amd.scene import Scene
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    chain = dict(curve="aces", exposure=0.5)
    view = dict(out_w=80, out_h=45, filter="area")
    with HipRenderer(sc, 160, 90, exact=True) as r:
        r.render(2)
        return dict(viewed16=r.present(encode=dict(format="rgba16"), view=view, **chain)[0], full16=r.present(encode=dict(format="rgba16"), **chain)[0],
                    viewed8=r.present(view=view, **chain)[0],
                    dithered=r.present(encode=dict(format="argb8", dither=True, dither_seed=9), view=view, **chain)[0])


@pytest.mark.parametrize("owners", ["1", "3-on-one-device"])
def test_driver_writes_the_c_abi_s_words(tmp_path, driver_reference, owners):
    """kajo_render --supersample 2 -w 80 -h 45 --png16 f.png --encode-view writes present(encode=RGBA16, view=AREA) of the 160x90 handle,
    for one GPU and for three owners on one device; the same command without the switch writes the file it has always written, the
    16-bit image at the rendered size; --dither goes with the view under the switch"""
    from test_encode_cpu import read_png16
    assert os.path.exists(BIN), BIN
    gpus = {"1": ["--gpus", "1"], "3-on-one-device": ["--gpus", "3", "--same-device"]}[owners]
    ref = driver_reference
    same = lambda png, argb: all(np.array_equal(png[..., k], (argb >> shift) & 255) for k, shift in enumerate((16, 8, 0)))
    out, deep = str(tmp_path / "o.png"), str(tmp_path / "deep.png")

    def run(extra):
        p = subprocess.run(DRIVER + gpus + ["-o", out] + extra + [SCENE], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        return json.loads(p.stdout.strip().splitlines()[-1])

    stats = run(["--png16", deep, "--encode-view"])
    got, _ = read_png16(deep)
    assert got.shape == (45, 80, 3) and np.array_equal(got, ref["viewed16"][..., :3])
    assert same(read_png(out), ref["viewed8"])  # -o stays the 8-bit view's
    assert (stats["encode_view_out_w"], stats["encode_view_out_h"], stats["view_out_w"], stats["encode_format"]) == (80, 45, 80, "rgba16")
    stats = run(["--png16", deep])
    got, _ = read_png16(deep)
    assert got.shape == (90, 160, 3) and np.array_equal(got, ref["full16"][..., :3]) and "encode_view_out_w" not in stats
    assert same(read_png(out), ref["viewed8"])
    stats = run(["--dither", "--dither-seed", "9", "--encode-view"])
    assert same(read_png(out), ref["dithered"]) and stats["encode_view_out_w"] == 80
