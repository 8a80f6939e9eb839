"""The encode (include/kajo_hip.h "The encode", kajo_hip_encode, kajo_hip_encode_present and its gathered twin; kajo_amd/csrc/encode.cpp)
on the GPU. The kernel is held WORD FOR WORD to kajo_hip_encode_pixels, the same lines (encode_math.h) compiled for the host, and to
tests/encode_replay.py's numpy restatement, which shares nothing with the library: no tolerance anywhere. Synthetic frames (the edge
inputs and a ramp through every binade) at ragged shapes and three tile shapes, read as tiles and as a row-major frame; the chain against
the partial chain's radiance; the image for 1 and 3 owners; what the stage leaves alone; the gathered twin's asynchrony; the driver's
--png16 and --dither files against the C ABI's words."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import read_png
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, encode_params, encode_pixels, grade_params
from kajo_amd.tiles import TileLayout
import encode_replay as R

pytestmark = pytest.mark.gpu
F32 = np.float32
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
# 64x4-pixel blocks: one lane; ragged on both axes; more than one block a row; whole tiles; several blocks on both axes
CASES = [((1, 1), (64, 16)), ((70, 19), (8, 32)), ((257, 3), (128, 8)), ((64, 16), (64, 16)), ((136, 40), (8, 32)), ((136, 40), (128, 8))]
CURVES = [("clamp", 0.0, 0.0), ("reinhard", 1.5, 4.0), ("aces", -0.5, 0.0)]
CURVE_ID = dict(clamp=R.CLAMP, reinhard=R.REINHARD, aces=R.ACES)
FORMATS = {"argb8": R.ARGB8, "rgb10a2": R.RGB10A2, "rgba16": R.RGBA16, "rgba16f": R.RGBA16F}
TRANSFERS = {"gamma22": R.GAMMA22, "srgb": R.SRGB, "pq": R.PQ, "linear": R.LINEAR}
PEAK, SEED = 600.0, 0x9ABCDEF1


def every_encode():
    """every format x transfer x dither the stage accepts, as encode_params()'s arguments"""
    out = []
    for f in ("argb8", "rgb10a2", "rgba16"):
        for t in TRANSFERS:
            for dither in (False, True):
                out.append(dict(format=f, transfer=t, dither=dither, peak_nits=PEAK, dither_seed=SEED))
    out.append(dict(format="rgba16f"))
    out.append(dict(format="rgba16f", scene=True))
    return out


def words(a):
    """an encoded array as the flat words of its format"""
    a = np.ascontiguousarray(a)
    return a.reshape(-1) if a.dtype == np.uint32 else a.view(np.uint64).reshape(-1)


def replay(e, curve, exposure, white, mean, W):
    flags = (R.DITHER if e.get("dither") else 0) | (R.SCENE if e.get("scene") else 0)
    transfer = e.get("transfer") or ("linear" if e["format"] == "rgba16f" else "gamma22")
    return R.encode_pixels(FORMATS[e["format"]], TRANSFERS[transfer], flags, e.get("peak_nits", 1000.0), e.get("dither_seed", 0), CURVE_ID[curve],
                           exposure, white, mean, 0, 0, W)


def synthetic(W, H):
    """(H, W, 4) sums: the edge inputs and the binade ramp, repeated to fill the frame"""
    m = np.concatenate([R.edge_means(), R.binade_ramp()])
    m = m[np.arange(W * H) % len(m)] if W * H >= 64 else m[17::len(m) // (W * H) or 1][:W * H]
    frame = np.zeros((H, W, 4), F32)
    frame[..., :3] = m.reshape(H, W, 3)
    frame[..., 3] = np.nan  # (.w is never read)
    return frame


def upload(r, frame, passes, tile):
    """`frame` into the handle's accumulation through its tile buffer, declared the sum of `passes`: read as tiles from here on"""
    import torch
    from bench import DevicePtr
    H, W = frame.shape[:2]
    ptr, nbytes = r.tile_buffer()
    buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
    ys, xs = np.mgrid[0:H, 0:W]
    _, slots = TileLayout(W, H, 1, tile).owner_and_slot(xs, ys)
    buf[torch.as_tensor(slots.reshape(-1).astype(np.int64), device="cuda")] = torch.as_tensor(np.ascontiguousarray(frame).reshape(-1, 4), device="cuda")
    torch.cuda.synchronize()
    r.set_pass_count(passes)


@pytest.fixture(scope="module")
def expected():
    """(shape, passes) -> the means and, per encode and curve, the replay's words: computed once, shared, never written"""
    cache = {}

    def get(W, H, passes):
        key = (W, H, passes)
        if key not in cache:
            frame = synthetic(W, H)
            with np.errstate(all="ignore"):
                mean = (frame[..., :3] / F32(passes)).astype(F32)
            want = {(i, c[0]): replay(e, *c, mean, W) for i, e in enumerate(every_encode()) for c in CURVES}
            for v in want.values():
                v.setflags(write=False)
            cache[key] = (frame, mean, want)
        return cache[key]

    return get


@pytest.mark.parametrize("shape,tile", CASES, ids=["%dx%d-tile%dx%d" % (s + t) for s, t in CASES])
def test_synthetic_frames_word_for_word(scenes, expected, shape, tile):
    """every format x transfer x dither under the three curves, from tiles and from the row-major frame: the device's words are
    kajo_hip_encode_pixels' and the replay's; alpha and padding included, nothing written beyond kajo_hip_encode_bytes"""
    W, H = shape
    passes = 1 if W * H != 136 * 40 else 3  # (P = 1 keeps the edge inputs as they are; P = 3 divides them)
    frame, mean, want = expected(W, H, passes)
    L = capi.lib()
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, tile=tile) as r:
        upload(r, frame, passes, tile)
        for source in ("tiles", "frame"):
            if source == "frame":
                assert np.array_equal(np.ascontiguousarray(r.radiance()[..., :3]).view(np.uint32), frame[..., :3].view(np.uint32))  # (composes: row-major now)
            for i, e in enumerate(every_encode()):
                p = encode_params(**e)
                size = C.c_size_t()
                assert L.kajo_hip_encode_bytes(C.byref(p), W, H, C.byref(size)) == 0
                assert size.value == W * H * R.BYTES[p.format]
                for curve, exposure, white in CURVES:
                    t = r._tone_params(curve, exposure, white)
                    out = np.full(size.value + 64, 0xA5, np.uint8)
                    capi.check(L.kajo_hip_encode(r._h, C.byref(p), C.byref(t), out.ctypes.data_as(C.c_void_p)))
                    assert (out[size.value:] == 0xA5).all(), (source, e, curve)
                    got = out[:size.value].view(R.DTYPE[p.format])
                    twin = encode_pixels(mean, p, row_width=W, curve=curve, exposure=exposure, white=white)
                    assert np.array_equal(got, twin), (source, e, curve, np.nonzero(got != twin)[0][:4])
                    assert np.array_equal(got, want[(i, curve)]), (source, e, curve, np.nonzero(got != want[(i, curve)])[0][:4])
        # the Python wrapper's shapes
        assert r.encode(dict(format="rgb10a2")).shape == (H, W) and r.encode(dict(format="rgba16")).shape == (H, W, 4)
        half = r.encode(dict(format="rgba16f"))
        assert half.dtype == np.float16 and (half[..., 3] == 1.0).all()


def test_behind_a_glare_the_stage_reads_the_row_major_frame(scenes):
    """glare with strength > 0 leaves a row-major frame in its scratch: the words are encode_pixels of kajo_hip_glare's radiance"""
    W, H, P = 136, 40, 3
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True, tile=(8, 32)) as r:
        r.render(P)
        gl = dict(levels=3, strength=0.3)
        mean = (r.glare(**gl)[..., :3] / F32(P)).astype(F32)
        r.set_pass_count(P)  # (the accumulation is read as tiles again)
        for e in (dict(format="rgba16", transfer="pq", peak_nits=PEAK), dict(format="rgb10a2", transfer="srgb", dither=True, dither_seed=5),
                  dict(format="rgba16f", scene=True)):
            got, _ = r.present(glare=gl, encode=e, curve="aces", exposure=0.5)
            assert np.array_equal(words(got), encode_pixels(mean, e, row_width=W, curve="aces", exposure=0.5)), e
            assert np.array_equal(words(got), replay(e, "aces", 0.5, 0.0, mean, W)), e


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_chain_is_encode_pixels_of_the_partial_chain_s_radiance(scenes, build):
    W, H, P = 96, 54, 3
    L = capi.lib()
    front = dict(despeckle=dict(), denoise=dict(iterations=2), glare=dict(levels=4, strength=0.2))
    local = dict(compression=0.7)
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, aov=True, **BUILDS[build]) as r:
        r.render(P)
        with np.errstate(all="ignore"):
            mean = (r.local(**front, **local)[..., :3] / F32(P)).astype(F32)
        for e, tone in ((dict(format="rgba16", transfer="srgb"), dict(curve="reinhard", exposure=1.0, white=3.0)),
                        (dict(format="argb8", dither=True, dither_seed=11), dict(curve="clamp")),
                        (dict(format="rgb10a2", transfer="pq", peak_nits=400.0), dict(curve="aces", exposure=-1.0))):
            got, result = r.present(local=local, encode=e, **front, **tone)
            assert result is None
            assert np.array_equal(words(got), encode_pixels(mean, e, row_width=W, **tone)), (e, tone)
            # with a meter the tone parameters are the host-patched ones
            ep, t, m = encode_params(**e), r._tone_params(**tone), r._meter_params(auto_white=True)
            s, d, g, l = r._despeckle_params(), r._denoise_params(iterations=2), r._glare_params(levels=4, strength=0.2), r._local_params(**local)
            res = capi.KajoMeterResult()
            out = np.zeros(W * H, R.DTYPE[ep.format])
            capi.check(L.kajo_hip_encode_present(r._h, C.byref(s), C.byref(d), None, None, C.byref(g), C.byref(l), C.byref(m), C.byref(t), C.byref(ep),
                                                 out.ctypes.data_as(C.c_void_p), C.byref(res)))
            patched = capi.KajoToneParams()
            capi.check(L.kajo_hip_meter_tone(C.byref(res), C.byref(m), C.byref(t), C.byref(patched)))
            assert res.metered > 0 and patched.exposure != t.exposure
            want = np.zeros_like(out)
            capi.check(L.kajo_hip_encode_pixels(C.byref(ep), C.byref(patched), mean.ctypes.data_as(C.c_void_p), W * H, 0, 0, W,
                                                want.ctypes.data_as(C.c_void_p)))
            assert np.array_equal(out, want), (e, tone)
            assert not np.array_equal(out, words(got))


def _gathered_encoded(root, gathered, e, tone, despeckle=None, grade=None, glare=None, guard=16):
    import torch
    ep = encode_params(**e)
    n = root.width * root.height * R.BYTES[ep.format] // 4
    out = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    ref = lambda p: None if p is None else C.byref(p)
    capi.check(capi.lib().kajo_hip_encode_present_gathered_device(root._h, src, ref(despeckle), ref(grade), ref(glare), None, None, C.byref(tone),
                                                                  C.byref(ep), C.c_void_p(out.data_ptr()), None))
    root.wait()
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert (host[n:] == 0x5A5A5A5A).all()
    return np.ascontiguousarray(host[:n]).view(R.DTYPE[ep.format])


@pytest.mark.parametrize("tile", [(64, 16), (32, 8)], ids=["tile64x16", "tile32x8"])
def test_the_image_does_not_depend_on_the_owners(scenes, tile):
    from test_hip_tonemap import _gathered
    sc = scenes["spheres_a169"]
    W, H = 130, 70
    gl = dict(levels=3, strength=0.2)
    encodes = [dict(format="argb8", dither=True, dither_seed=3), dict(format="rgba16", transfer="pq", peak_nits=PEAK, dither=True),
               dict(format="rgb10a2", transfer="srgb"), dict(format="rgba16f", scene=True)]
    with HipRenderer(sc, W, H, spp=4, exact=True, tile=tile) as r:
        r.render(3)
        g, t, d, c = r._glare_params(**gl), r._tone_params("reinhard", 0.5), r._despeckle_params(), grade_params(saturation=1.3)
        want = [words(r.present(despeckle=dict(), grade=dict(saturation=1.3), glare=gl, encode=e, curve="reinhard", exposure=0.5)[0]) for e in encodes]
        for e, w in zip(encodes, want):
            assert np.array_equal(_gathered_encoded(r, None, e, t, d, c, g), w), e
    owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile=tile, tile_index=k, tile_count=3) for k in range(3)]
    try:
        for o in owners:
            o.render(3)
        gathered = _gathered(owners)
        for e, w in zip(encodes, want):
            assert np.array_equal(_gathered_encoded(owners[0], gathered, e, t, d, c, g), w), e
    finally:
        for o in owners:
            o.close()


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_the_stage_leaves_the_handle_as_it_was(scenes, build):
    sc = scenes["spheres_a43"]
    kw = dict(spp=4, aov=True, counters=True, **BUILDS[build])
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    with HipRenderer(sc, 100, 75, **kw) as a, HipRenderer(sc, 100, 75, **kw) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        before = a.argb8()
        for e in every_encode()[::5]:
            a.encode(e, curve="aces")
        a.present(encode=dict(format="rgba16", transfer="pq"), denoise=dict(iterations=2), despeckle=dict(), glare=dict(), meter=dict(),
                  local=dict(), lens=dict(), grade=dict(saturation=1.2), curve="reinhard")
        _gathered_encoded(a, None, dict(format="rgb10a2", dither=True), a._tone_params("aces"))
        assert a.counters()["kernelMs"] == ms
        assert np.array_equal(a.argb8(), before) and np.array_equal(a.argb8(), b.argb8())
        assert np.array_equal(bits(a.radiance()), bits(b.radiance()))
        for x, y in zip(a.aov()["raw"], b.aov()["raw"]):
            assert np.array_equal(bits(x), bits(y))
        ca, cb = a.counters(), b.counters()
        for key in ("passes", "launches", "paths", "traversals", "vertices"):
            assert ca[key] == cb[key], key
        assert ca["passes"] == 3
        a.render(2)
        b.render(2)
        assert np.array_equal(bits(a.radiance()), bits(b.radiance())) and a.counters()["passes"] == 5


def test_refusals_on_a_device(scenes):
    with HipRenderer(scenes["spheres_a43"], 64, 48, spp=4) as r:
        with pytest.raises(capi.KajoError) as e:
            r.encode()
        assert e.value.code == capi.KAJO_E_STATE and "nothing rendered" in str(e.value)
        r.render(1)
        with pytest.raises(capi.KajoError) as e:
            r.encode(auto_exposure=True)
        assert e.value.code == capi.KAJO_E_INVALID and "metered exposure" in str(e.value)
        p, t = encode_params(), r._tone_params()
        assert capi.lib().kajo_hip_encode(r._h, C.byref(p), C.byref(t), None) == 0  # dst may be NULL
        assert capi.lib().kajo_hip_encode_present_gathered_device(r._h, None, None, None, None, None, None, C.byref(t), C.byref(p), None,
                                                                  None) == capi.KAJO_E_INVALID
    with HipRenderer(scenes["spheres_a43"], 64, 48, spp=4, tile_index=1, tile_count=2) as part:
        part.render(1)
        with pytest.raises(capi.KajoError) as e:
            part.encode()
        assert e.value.code == capi.KAJO_E_STATE


def test_the_gathered_twin_enqueues_on_the_caller_s_stream_without_waiting(scenes):
    """tests/test_hip_streams.py's pattern: a spin on the caller's stream S, a render behind it, the twin behind that. The call returns
    while the spin runs, and after S alone is waited for the words are those of the frame rendered behind the spin. The transfer's
    peak differs from the warm-up's, so the table's upload goes through the staging block inside the window too."""
    import torch
    from test_hip_streams import Spin
    W, H = 96, 54
    e0, e1 = dict(format="rgba16", transfer="pq", peak_nits=1000.0), dict(format="rgba16", transfer="pq", peak_nits=500.0, dither=True)
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r, HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as twin:
        S = torch.cuda.Stream()
        tone = r._tone_params("aces")
        twin.render(2)
        want = words(twin.encode(e1, curve="aces"))
        r.set_stream(S.cuda_stream)
        r.render(1).wait()
        stale = _gathered_encoded(r, None, e1, tone)
        _gathered_encoded(r, None, e0, tone)  # (the warm-up: every buffer stands, the table is the other peak's)
        ep = encode_params(**e1)
        out = torch.zeros(W * H * 2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        try:
            spin = Spin(S)
            r.render(1)
            rendered = spin.running()
            capi.check(capi.lib().kajo_hip_encode_present_gathered_device(r._h, None, None, None, None, None, None, C.byref(tone), C.byref(ep),
                                                                          C.c_void_p(out.data_ptr()), None))
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


# -- the driver ----------------------------------------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
SCENE = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
DRIVER = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "--json", "--glare", "0.1", "--tonemap", "aces", "--exposure", "0.5"]


@pytest.fixture(scope="module")
def driver_reference():
    """caustics 96x54, 2 passes, through the C ABI: the words of the chains the driver is asked for"""
    from kajo_amd.scene import Scene
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    chain = dict(glare=dict(strength=0.1), curve="aces", exposure=0.5)
    with HipRenderer(sc, 96, 54, exact=True) as r:
        r.render(2)
        ref = dict(plain=r.present(**chain)[0],
                   dither=r.present(encode=dict(format="argb8", dither=True, dither_seed=9), **chain)[0],
                   gamma=r.present(encode=dict(format="rgba16"), **chain)[0],
                   pq=r.present(encode=dict(format="rgba16", transfer="pq", peak_nits=600.0), **chain)[0],
                   metered=r.present(encode=dict(format="rgba16", transfer="srgb"), meter=dict(), **chain)[0])
    assert not np.array_equal(ref["plain"], ref["dither"]) and not np.array_equal(ref["gamma"], ref["pq"])
    return ref


@pytest.mark.parametrize("owners", ["1", "3-on-one-device"])
def test_driver_writes_the_c_abi_s_words(tmp_path, driver_reference, owners):
    """kajo_render --png16 / --dither write the words HipRenderer.present(encode=...) gives on the same frame, for one GPU and for three
    owners on one device (the gathered twin); --json reports the encode; without the options the plain PNG"""
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

    stats = run(["--png16", deep, "--transfer", "pq", "--peak-nits", "600", "--dither", "--dither-seed", "9"])
    assert same(read_png(out), ref["dither"])
    got, chunks = read_png16(deep)
    assert np.array_equal(got, ref["pq"][..., :3]) and chunks[b"cICP"] == bytes([1, 16, 0, 1])
    assert (stats["encode_format"], stats["encode_transfer"], stats["encode_peak_nits"], stats["encode_dither"]) == ("rgba16", "pq", 600, True)
    stats = run(["--png16", deep])
    assert same(read_png(out), ref["plain"])  # -o stays the undithered resolve
    got, chunks = read_png16(deep)
    assert np.array_equal(got, ref["gamma"][..., :3]) and b"cICP" not in chunks
    assert (stats["encode_format"], stats["encode_transfer"], stats["encode_peak_nits"], stats["encode_dither"]) == ("rgba16", "gamma22", None, False)
    stats = run(["--png16", deep, "--transfer", "srgb", "--meter-exposure", "0.5"])
    assert np.array_equal(read_png16(deep)[0], ref["metered"][..., :3])
    stats = run(["--dither", "--dither-seed", "9"])
    assert same(read_png(out), ref["dither"]) and (stats["encode_format"], stats["encode_dither"]) == ("argb8", True)
    stats = run([])
    assert same(read_png(out), ref["plain"]) and "encode_format" not in stats
