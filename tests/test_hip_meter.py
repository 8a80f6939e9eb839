"""Histogram metering (include/kajo_hip.h kajo_hip_meter, kajo_hip_present_metered_*; kajo_amd/csrc/meter.hip) on the GPU.

The kernels are held to `restate`, a numpy float32 restatement of the header's definition with its order of operations, over synthetic
frames written into the accumulation through the tile buffer and over rendered frames. The luminance is three float32 products and two
float32 sums in a fixed order, the bin is integer arithmetic on its bits and the counts are integers: there is NO tolerance anywhere in
this file. The histogram and the count of pixels that do not count must equal the restatement's word for word, from tiles, from a
composed frame and from gathered buffers of any number of owners; the metered present must be the plain present with the patched tone
parameters bit for bit; and the calls leave the handle as a twin that never metered. The two bounds of the rendered-frame test are
derived from the bin shape (see there)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from framelib import bits, read_pfm, read_png
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import Scene
from kajo_amd.tiles import TileLayout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
BUILDS = {"fast": dict(), "exact": dict(exact=True), "strict": dict(strict=True)}
F32, F64 = np.float32, np.float64
BINS = 514
BASE = (127 - 16) << 4
FLT_MAX = np.finfo(F32).max
RESULT_INTS = ("pixels", "nonfinite", "under", "over", "metered", "minBin", "maxBin")
RESULT_FLOATS = ("anchorL", "whiteL", "exposure")


def luminance(F, passes):
    """-> (counts (bool), l (float32)) per pixel: include/kajo_hip.h, operation for operation."""
    F = np.ascontiguousarray(F, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        m = F[..., :3] / F32(passes)
        counts = np.isfinite(m).all(-1)
        x = np.maximum(m, F32(0))
        l = (F32(0.2126) * x[..., 0] + F32(0.7152) * x[..., 1]) + F32(0.0722) * x[..., 2]
    assert l.dtype == F32
    return counts, l


def bin_of(l):
    k = ((bits(l) & np.uint32(0x7fffffff)) >> np.uint32(19)).astype(np.int64)
    return np.where(k < BASE, 0, np.minimum(k - BASE + 1, BINS - 1))


def restate(F, passes):
    """-> (hist (514,) uint32, nonfinite): the words kajo_hip_meter must give."""
    counts, l = luminance(F, passes)
    hist = np.bincount(bin_of(l)[counts].reshape(-1), minlength=BINS).astype(np.uint32)
    nonfinite = int((~counts).sum())
    assert nonfinite + int(hist.astype(np.int64).sum()) == counts.size
    return hist, nonfinite


def check_words(got, F, passes, what=""):
    hist, result = got
    want, nonfinite = restate(F, passes)
    assert hist.dtype == np.uint32 and hist.shape == (BINS,)
    differ = np.flatnonzero(hist != want)
    assert differ.size == 0, (what, differ[:8], hist[differ[:8]], want[differ[:8]])
    assert result["nonfinite"] == nonfinite and result["pixels"] == F.shape[0] * F.shape[1], (what, result, nonfinite)
    assert result["nonfinite"] + int(hist.astype(np.int64).sum()) == result["pixels"], what
    assert (result["under"], result["over"], result["metered"]) == (int(want[0]), int(want[513]), int(want[1:].astype(np.int64).sum())), what


def _upload(owners, frame, passes, tile=(64, 16)):
    """Write `frame` (H, W, 4) float32 into the accumulation of the handles that share it, through their tile buffers, and declare it
    the sum of `passes`."""
    import torch
    from bench import DevicePtr
    H, W = frame.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    owner, slots = TileLayout(W, H, len(owners), tile).owner_and_slot(xs, ys)
    owner, slots, flat = owner.reshape(-1), slots.reshape(-1).astype(np.int64), frame.reshape(-1, 4)
    for k, r in enumerate(owners):
        r.wait()
        ptr, nbytes = r.tile_buffer()
        buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
        mine = owner == k
        if mine.any():
            buf[torch.as_tensor(slots[mine], device="cuda")] = torch.as_tensor(flat[mine], device="cuda")
    torch.cuda.synchronize()
    for r in owners:
        r.set_pass_count(passes)


def _steps(start, n):
    """the 2 n + 1 consecutive floats around `start` (positive, finite)"""
    return (bits(F32([start]))[0].astype(np.int64) + np.arange(-n, n + 1)).astype(np.uint32).view(F32)


_POOLS = {}


def pool(passes):
    """(N, 4) float32 pixels, sums over `passes`, shared by the tests and not changed: for every bin edge 2^k, k = -17..17, and the
    float one ulp either side of it, a pixel whose luminance is exactly that float (found by searching one channel's sums ulp by ulp:
    the restatement tells which float a sum gives); then zeros of both signs, negative channels, denormals, FLT_MAX in all channels,
    NaN, +Inf and -Inf."""
    if passes in _POOLS:
        return _POOLS[passes]
    px = []
    for k in range(-17, 18):
        edge = F32(2.0 ** k)
        for target in (np.nextafter(edge, F32(0)), edge, np.nextafter(edge, F32(np.inf))):
            for ch, weight in ((1, 0.7152), (0, 0.2126), (2, 0.0722)):
                cand = np.zeros((801, 4), F32)
                cand[:, ch] = _steps(F32(F64(target) / weight * passes), 400)
                _, l = luminance(cand, passes)
                hit = np.flatnonzero(bits(l) == bits(F32([target]))[0])
                if hit.size:
                    px.append(cand[hit[0]])
                    break
            else:
                raise AssertionError("no pixel found whose luminance is %r over %d passes" % (target, passes))
    den = np.array([1], np.uint32).view(F32)[0]  # the smallest denormal
    for rgb in ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-0.0, 0.0, -0.0), (-1.0, 2.0, -3.0), (-5.0, -5.0, -5.0), (4.0, -1e30, 0.5), (den, den, den),
                (1e-40, 1e-39, 1e-41), (1e-38, 0.0, 0.0), (FLT_MAX, FLT_MAX, FLT_MAX), (FLT_MAX, 0.0, 0.0), (0.0, FLT_MAX, 1.0), (np.nan, 1.0, 1.0),
                (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf), (np.nan, np.nan, np.nan), (np.inf, -np.inf, np.nan), (-FLT_MAX, 1.0, 1.0), (3e38, 3e38, 3e38)):
        px.append(F32(list(rgb) + [1.0]))
    out = np.stack(px).astype(F32)
    out[:, 3] = np.arange(len(out)) % 7  # (.w is not read)
    # every edge, and the float either side of it, is among the luminances, and so is every kind of bin
    counts, l = luminance(out, passes)
    have = set(bits(l[counts]).tolist())
    for k in range(-17, 18):
        e = F32(2.0 ** k)
        for t in (np.nextafter(e, F32(0)), e, np.nextafter(e, F32(np.inf))):
            assert int(bits(F32([t]))[0]) in have, (k, t)
    b = bin_of(l[counts])
    assert {0, 1, 17, 512, 513} <= set(b.tolist()) and (~counts).sum() == 5
    _POOLS[passes] = out
    return out


def noise(n, passes, seed):
    """log-uniform luminances over 2^-20 .. 2^20, in random hues"""
    rng = np.random.default_rng(seed)
    f = np.empty((n, 4), F32)
    f[:, :3] = (2.0 ** rng.uniform(-20, 20, (n, 1)) * rng.uniform(0.2, 1.8, (n, 3)) * passes).astype(F32)
    f[:, 3] = 1.0
    return f


def frames_for(W, H, passes):
    """name -> (H, W, 4): the pool in as many frames as it takes (a large frame holds it whole, the rest noise), a constant frame (all
    lanes in one bin), noise, and a frame in which nothing counts."""
    n = W * H
    p = pool(passes)
    frames = {}
    for i in range(0, len(p), n):
        part = p[i:i + n]
        frames["pool%d" % (i // n)] = np.concatenate([part, noise(n - len(part), passes, 7 * n + i)]).reshape(H, W, 4)
    c = np.empty((H, W, 4), F32)
    c[..., :3] = F32([0.7, 0.25, 1.3]) * F32(passes)
    c[..., 3] = 1.0
    frames["constant"] = c
    frames["noise"] = noise(n, passes, n).reshape(H, W, 4)
    frames["all_nan"] = np.full((H, W, 4), np.nan, F32)
    return frames


def _rects(W, H):
    return ((W + 63) // 64) * ((H + 3) // 4)


def second_stride_shapes():
    """kajo_meter_groups is the plan: a workgroup takes the 64x4 rectangles g, g + groups, g + 2 groups, ..., four of them a trip. The
    smallest frames (fewest pixels, one and two columns of rectangles) at which the first workgroup takes a second rectangle, and at
    which it takes a second trip."""
    L = capi.lib()
    cap = L.kajo_meter_groups(1 << 14, 1 << 14)
    shapes = []
    for per_group in (1, 4):
        for W in (1, 65):
            cols = (W + 63) // 64
            H = 4 * (per_group * cap // cols) + 1
            assert _rects(W, H) > per_group * L.kajo_meter_groups(W, H) and _rects(W, H - 1) <= per_group * L.kajo_meter_groups(W, H - 1), (W, H)
            shapes.append((W, H))
    return shapes


SHAPES = [(1, 1), (2, 1), (7, 5), (41, 23), (65, 9), (130, 70)]


def _check_shape(scenes, W, H):
    with HipRenderer(scenes["spheres_a43"], W, H, spp=4, exact=True) as r:
        for passes in (1, 3):
            for name, frame in frames_for(W, H, passes).items():
                _upload([r], frame, passes)
                check_words(r.meter(), frame, passes, (W, H, passes, name))


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_histogram_matches_the_restatement_word_for_word(scenes, shape):
    _check_shape(scenes, *shape)


@pytest.mark.parametrize("which", range(4), ids=["stride_1col", "stride_2col", "trip_1col", "trip_2col"])
def test_histogram_where_a_workgroup_takes_a_second_rectangle_and_a_second_trip(scenes, which):
    _check_shape(scenes, *second_stride_shapes()[which])


def _meter_params(**kw):
    p = capi.KajoMeterParams()
    capi.lib().kajo_hip_default_meter_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _result_dict(r):
    return {k: getattr(r, k) for k in RESULT_INTS + RESULT_FLOATS}


def _same_result(a, b):
    return all(a[k] == b[k] for k in RESULT_INTS) and all(bits(F32([a[k]]))[0] == bits(F32([b[k]]))[0] for k in RESULT_FLOATS)


def _metered_gathered(root, gathered, W, H, d, g, m, tone):
    """kajo_hip_present_metered_gathered_argb8_device on `root` -> (argb8, result dict)."""
    import torch
    L = capi.lib()
    out = torch.empty(W * H, dtype=torch.int32, device="cuda")
    src = None if gathered is None else C.c_void_p(gathered.data_ptr())
    ref = lambda p: None if p is None else C.byref(p)
    result = capi.KajoMeterResult()
    capi.check(L.kajo_hip_present_metered_gathered_argb8_device(root._h, src, ref(d), ref(g), ref(m), C.byref(tone), C.c_void_p(out.data_ptr()),
                                                                C.byref(result)))
    root.wait()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(H, W), _result_dict(result)


def test_any_source_any_owner_count(scenes):
    """The same words from the handle's tiles, from its composed frame, on a second call and on a twin handle; from gathered buffers
    of 1, 2, 3 and 8 owners composed on the root; and through the gathered twin, which reads the gathered tile buffers themselves
    and hands out the evaluation only: every integer field and, probed at nine percentiles, the whole cumulative histogram. A ragged
    frame, so that tiles are cut by the edges."""
    from test_meter_cpu import evaluate
    from test_hip_tonemap import _gathered, _tone_params
    sc = scenes["spheres_a43"]
    W, H, passes = 200, 77, 3
    frame = frames_for(W, H, passes)["pool0"]
    want, nonfinite = restate(frame, passes)
    probes = (2.0 ** -24, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.995, 1.0)
    with HipRenderer(sc, W, H, spp=4, exact=True) as r, HipRenderer(sc, W, H, spp=4, exact=True) as twin:
        _upload([r], frame, passes)
        _upload([twin], frame, passes)
        first = r.meter()
        check_words(first, frame, passes, "tiles")
        for what, got in (("second call", r.meter()), ("twin", twin.meter())):
            assert np.array_equal(got[0], first[0]) and _same_result(got[1], first[1]), what
        assert np.array_equal(bits(r.radiance()), bits(frame))  # composes the float frame: the call now reads it, row-major
        got = r.meter()
        check_words(got, frame, passes, "composed")
        assert _same_result(got[1], first[1])
    for count in (1, 2, 3, 8):
        owners = [HipRenderer(sc, W, H, spp=4, exact=True, tile_index=k, tile_count=count) for k in range(count)]
        try:
            _upload(owners, frame, passes)
            gathered = _gathered(owners)
            for q in probes:
                _, res = _metered_gathered(owners[0], gathered, W, H, None, None, _meter_params(percentile=q, whitePercentile=q), _tone_params())
                e = evaluate(want, percentile=q, white_percentile=q)
                assert res["pixels"] == W * H and res["nonfinite"] == nonfinite, (count, q, res)
                for k in ("under", "over", "metered", "minBin", "maxBin"):
                    assert res[k] == e[k], (count, q, k, res[k], e[k])
                assert bits(F32([res["anchorL"]]))[0] == bits(F32([e["anchorL"]]))[0] == bits(F32([res["whiteL"]]))[0], (count, q, res, e)
            owners[0].compose(gathered.data_ptr())
            got = owners[0].meter()
            check_words(got, frame, passes, "%d owners, composed" % count)
            assert _same_result(got[1], first[1]), count
        finally:
            for o in owners:
                o.close()


def test_histogram_behind_the_existing_stages(scenes):
    """With despeckle, denoise and glare in front, the histogram is the restatement's over the float frame the existing entry points
    return for the same parameters."""
    sc = scenes["spheres_a43"]
    ds, dn, gl = dict(factor=2.0, rank=2, floor=0.01), dict(iterations=3), dict(levels=4, strength=0.25)
    with HipRenderer(sc, 100, 75, spp=4, aov=True, exact=True) as r:
        r.render(3)
        check_words(r.meter(), r.radiance(), 3, "accumulation")
        check_words(r.meter(despeckle=ds), r.despeckle(**ds)["radiance"], 3, "despeckle")
        check_words(r.meter(denoise=dn), r.denoise(**dn)["radiance"], 3, "denoise")
        check_words(r.meter(glare=gl), r.glare(**gl), 3, "glare")
        check_words(r.meter(denoise=dn, glare=gl), r.glare(denoise=dn, **gl), 3, "denoise + glare")
        # the whole chain has no float read-back of its own: it is metered twice, and its last stage must have changed the counts
        a, b = r.meter(despeckle=ds, denoise=dn, glare=gl), r.meter(despeckle=ds, denoise=dn, glare=gl)
        assert np.array_equal(a[0], b[0]) and _same_result(a[1], b[1])
        assert not np.array_equal(a[0], r.meter(despeckle=ds, denoise=dn)[0])


@pytest.fixture(scope="module")
def owners3(scenes):
    """spheres.json 16:9 at 160x90, 4 spp x 2 passes, dealt to three EXACT owners on one GPU, and their gathered buffers"""
    from test_hip_tonemap import _gathered
    owners = [HipRenderer(scenes["spheres_a169"], 160, 90, spp=4, exact=True, tile_index=k, tile_count=3) for k in range(3)]
    for o in owners:
        o.render(2)
    yield owners, _gathered(owners)
    for o in owners:
        o.close()


CASES = [dict(tone=dict(curve="reinhard"), meter=dict(auto_white=True)),
         dict(tone=dict(curve="aces", exposure=0.5), meter=dict(percentile=0.7, key=0.3)),
         dict(tone=dict(curve="reinhard", white=4.0, exposure=-1.0), meter=dict()),
         dict(tone=dict(), meter=dict(percentile=0.9, white_percentile=0.5, auto_white=True))]


@pytest.mark.parametrize("build", ["fast", "exact", "strict"])
def test_metered_present_is_the_plain_present_with_the_patched_tone(scenes, build, owners3):
    from test_hip_glare import _glare_params
    from test_hip_despeckle import _despeckle_params
    L = capi.lib()
    W, H = 160, 90
    ds, gl = dict(factor=2.0, rank=2, floor=0.01), dict(levels=4, strength=0.25)
    ref = lambda p: None if p is None else C.byref(p)
    with HipRenderer(scenes["spheres_a169"], W, H, spp=4, **BUILDS[build]) as r:
        r.render(2)
        for case in CASES:
            for stages in (dict(), dict(despeckle=ds, glare=gl)):
                img, res = r.present(meter=case["meter"], **stages, **case["tone"])
                hist, measured = r.meter(**stages, **case["meter"])
                assert _same_result(res, measured), (case, res, measured)
                m, t = r._meter_params(**case["meter"]), r._tone_params(**case["tone"])
                result = capi.KajoMeterResult(**{k: measured[k] for k in RESULT_INTS + RESULT_FLOATS})
                patched = capi.KajoToneParams()
                capi.check(L.kajo_hip_meter_tone(C.byref(result), C.byref(m), C.byref(t), C.byref(patched)))
                assert patched.exposure == min(max(F32(t.exposure) + F32(measured["exposure"]), F32(-32)), F32(32))
                s = None if "despeckle" not in stages else r._despeckle_params(**ds)
                g = None if "glare" not in stages else r._glare_params(**gl)
                plain = np.empty((H, W), np.uint32)
                capi.check(L.kajo_hip_present_argb8(r._h, ref(s), None, ref(g), C.byref(patched), plain.ctypes.data_as(C.c_void_p), None))
                assert np.array_equal(img, plain), (build, case, stages)
                # meter == NULL: kajo_hip_present_argb8 itself
                none = np.empty((H, W), np.uint32)
                capi.check(L.kajo_hip_present_metered_argb8(r._h, ref(s), None, ref(g), None, C.byref(t), none.ctypes.data_as(C.c_void_p), None))
                assert np.array_equal(none, r.present(**stages, **case["tone"])[0])
                if build == "exact":
                    # the gathered twin over three owners: the one-owner image and measurement
                    owners, gathered = owners3
                    got, gres = _metered_gathered(owners[0], gathered, W, H, s, g, m, t)
                    assert np.array_equal(got, img) and _same_result(gres, res), (case, stages)
                    own, ores = _metered_gathered(r, None, W, H, s, g, m, t)
                    assert np.array_equal(own, img) and _same_result(ores, res)
        if build == "exact":
            owners, gathered = owners3
            t = r._tone_params(curve="aces")
            got, _ = _metered_gathered(owners[0], gathered, W, H, None, _glare_params(**gl), None, t)  # meter == NULL: the present twin
            assert np.array_equal(got, r.present(glare=gl, curve="aces")[0])
    assert _despeckle_params is not None


def test_metered_exposure_and_white_on_a_rendered_frame(scenes):
    """spheres.json 16:9 at 160x90, 4 spp x 2 passes, defaults. The anchor is the centre of the bin that holds the median of the metered
    luminances (the ceil(n / 2)-th smallest); a bin spans a factor (m + 1) / m of a stop's sixteenth, m = 16..31, so the median lies
    within a factor 1 +- 1/33 of the centre at the worst (half a bin, m = 16) and median * 2^exposure within that of the key; 1/32
    leaves the roundings of the centre, the logarithm and the product (a few 1e-7) their room. With auto white: whiteL is the centre of
    the bin that holds the ceil(0.995 n)-th smallest, so at most n - ceil(0.995 n) <= ceil(0.005 n) pixels lie in higher bins, and those
    above whiteL inside its own bin are at most the bin's count."""
    with HipRenderer(scenes["spheres_a169"], 160, 90, spp=4, exact=True) as r:
        r.render(2)
        F = r.radiance()
        hist, res = r.meter()
        check_words((hist, res), F, 2, "rendered")
        counts, l = luminance(F, 2)
        metered = np.sort(l[counts & (bin_of(l) >= 1)].astype(F64))
        n = metered.size
        assert n == res["metered"] and n > 160 * 90 // 2
        median = metered[math.ceil(0.5 * n) - 1]
        ratio = median * 2.0 ** F64(res["exposure"]) / F64(F32(0.18))
        print("median %.6g, anchor %.6g, exposure %.6f EV, median * 2^exposure / key = %.6f" % (median, res["anchorL"], res["exposure"], ratio))
        assert 1 - 1 / 32 <= ratio <= 1 + 1 / 32, ratio
        white_bin = int(bin_of(F32([res["whiteL"]]))[0])
        above = int((metered > F64(res["whiteL"])).sum())
        print("whiteL %.6g (bin %d, %d pixels), %d of %d metered pixels above it" % (res["whiteL"], white_bin, hist[white_bin], above, n))
        assert above <= math.ceil(0.005 * n) + int(hist[white_bin])
        img, pres = r.present(meter=dict(auto_white=True), curve="reinhard")
        assert _same_result(pres, res)
        assert not np.array_equal(img, r.present(curve="reinhard")[0])
        assert (res["maxBin"] - res["minBin"] + 1) / 16 > 4  # the lights are stops above the walls


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_metering_leaves_the_handle_as_it_was(scenes, build):
    """radiance(), aov() and counters() (kernelMs included) of a handle that metered and presented are those of a twin that never did;
    so are the passes rendered afterwards."""
    from test_hip_tonemap import _tone_params
    sc = scenes["spheres_a43"]
    with HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as a, \
            HipRenderer(sc, 100, 75, spp=4, aov=True, counters=True, **BUILDS[build]) as b:
        a.render(3).wait()
        b.render(3).wait()
        ms = a.counters()["kernelMs"]
        a.meter()
        a.meter(despeckle=dict(), denoise=dict(iterations=2), glare=dict())
        a.present(meter=dict(auto_white=True), despeckle=dict(), glare=dict(), curve="reinhard", exposure=1.0)
        a.present(meter=dict(), denoise=dict(iterations=3), curve="aces")
        _metered_gathered(a, None, 100, 75, None, None, _meter_params(), _tone_params("reinhard"))
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
        assert np.array_equal(a.meter()[0], b.meter()[0])


def test_states_on_a_device(scenes):
    import torch
    L = capi.lib()
    sc = scenes["spheres_a43"]
    m, t = _meter_params(), capi.KajoToneParams()
    L.kajo_hip_default_tone_params(C.byref(t))
    with HipRenderer(sc, 64, 48, spp=4, exact=True) as r:
        out = torch.empty(64 * 48, dtype=torch.int32, device="cuda")
        for call in (lambda: L.kajo_hip_meter(r._h, None, None, None, C.byref(m), None, None),
                     lambda: L.kajo_hip_present_metered_argb8(r._h, None, None, None, C.byref(m), C.byref(t), None, None),
                     lambda: L.kajo_hip_present_metered_gathered_argb8_device(r._h, None, None, None, C.byref(m), C.byref(t),
                                                                              C.c_void_p(out.data_ptr()), None)):
            assert call() == capi.KAJO_E_STATE and "nothing rendered" in L.kajo_hip_last_error().decode()
        r.render(1)
        assert L.kajo_hip_meter(r._h, None, None, None, C.byref(m), None, None) == 0  # hist and result may both be NULL
        dn = capi.KajoDenoiseParams()
        L.kajo_hip_default_denoise_params(C.byref(dn))
        assert L.kajo_hip_meter(r._h, None, C.byref(dn), None, C.byref(m), None, None) == capi.KAJO_E_STATE  # no AOVs to guide the denoiser
    with HipRenderer(sc, 64, 48, spp=4, exact=True, tile_index=0, tile_count=2) as part:
        part.render(1)
        assert L.kajo_hip_meter(part._h, None, None, None, C.byref(m), None, None) == capi.KAJO_E_STATE  # a share of the frame, not composed


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("gpus", [["--gpus", "1"], ["--gpus", "3", "--same-device"]])
def test_driver_meters_as_the_c_abi(tmp_path, gpus):
    """kajo_render --meter-exposure 0.5 --meter-white 0.995 --tonemap reinhard: the pixels of HipRenderer.present(meter=...) on the same
    frame, one owner and three gathered on one device; the --json fields are the result's; --hdr stays the accumulation / P; without
    the options, the image written today."""
    scene = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
    out, raw, hdr = str(tmp_path / "o.png"), str(tmp_path / "o.raw"), str(tmp_path / "o.pfm")
    base = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "--json", *gpus]
    p = subprocess.run(base + ["-o", out, "--raw", raw, "--hdr", hdr, "--meter-exposure", "0.5", "--meter-white", "0.995", "--tonemap", "reinhard",
                               "--exposure", "0.25", scene], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    acc = np.fromfile(raw, np.float32).reshape(54, 96, 4)
    png = read_png(out)
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    with HipRenderer(sc, 96, 54, exact=True) as r:
        r.render(2)
        assert np.array_equal(bits(r.radiance()), bits(acc))
        px, res = r.present(meter=dict(percentile=0.5, white_percentile=0.995, auto_white=True), curve="reinhard", exposure=0.25)
        plain, _ = r.present(curve="reinhard", exposure=0.25)
    assert not np.array_equal(px, plain)
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (px >> shift) & 255), k
    for field, key in (("meter_exposure", "exposure"), ("meter_white", "whiteL"), ("meter_anchor", "anchorL")):
        assert F32(stats[field]) == F32(res[key]), (field, stats[field], res[key])
    assert (stats["meter_metered"], stats["meter_under"], stats["meter_over"]) == (res["metered"], res["under"], res["over"])
    assert stats["meter_stops"] == (res["maxBin"] - res["minBin"] + 1) / 16
    assert np.array_equal(bits(read_pfm(hdr)), bits(acc[..., :3] / F32(2)))
    none = str(tmp_path / "n.png")
    p = subprocess.run(base + ["-o", none, "--tonemap", "reinhard", "--exposure", "0.25", scene], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "meter_exposure" not in p.stdout
    png = read_png(none)
    for k, shift in enumerate((16, 8, 0)):
        assert np.array_equal(png[..., k], (plain >> shift) & 255), k
