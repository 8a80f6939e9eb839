"""Histogram metering (include/kajo_hip.h kajo_hip_meter*, kajo_amd/csrc/meter.hip) without a GPU: the structs, constants and entry
points as the header declares them, in the product and the tools' twin; the documented defaults; the pure host half --
kajo_hip_meter_evaluate against `evaluate`, a numpy restatement of the header's definition, every field exactly (the exposure, a
logarithm, within 1e-6 of numpy's), and kajo_hip_meter_tone; every refusal that comes before a device is looked at, and their order
(despeckle, glare, meter, tone, denoise, handle); what the compiler made of the kernels (nothing spilled, no scratch, no FLAT
instruction, no global or buffer atomic, vector stores; registers, occupancy and LDS pinned); and the driver's refusals. The compile
command is the Makefile's own (`make -n`)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import devicecode
from kajo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
ENTRY_POINTS = ("kajo_hip_default_meter_params", "kajo_hip_meter_evaluate", "kajo_hip_meter_tone", "kajo_hip_meter",
                "kajo_hip_present_metered_argb8", "kajo_hip_present_metered_gathered_argb8_device")
# kernel -> (VGPRs, LDS bytes): what hipcc makes of them; registers pinned to within VGPR_ROOM, as for the despeckle
KERNELS = {"kajo_meter_hist": (38, 2060), "kajo_meter_sum": (38, 1024)}
VGPR_ROOM = 2
BINS = 514
BASE = (127 - 16) << 4
F32, F64 = np.float32, np.float64


def _header():
    return open(os.path.join(ROOT, "include", "kajo_hip.h")).read()


def edge(b):
    """lower edge of inner bin b = 1..513: the float with the bits (b - 1 + base) << 19"""
    return np.array([(b - 1 + BASE) << 19], np.uint32).view(F32)[0]


def centre(b):
    return edge(513) if b >= 513 else F32((F64(edge(b)) + F64(edge(b + 1))) / F64(2))


def value(hist, n, q):
    rank = min(n, max(1, int(np.ceil(F64(F32(q)) * F64(n)))))
    cum = np.cumsum(hist[1:].astype(np.int64))
    return centre(1 + int(np.searchsorted(cum, rank, side="left")))


def evaluate(hist, percentile=0.5, key=0.18, white_percentile=0.995):
    """include/kajo_hip.h, 'Evaluation', in numpy: the fields kajo_hip_meter_evaluate writes."""
    hist = np.asarray(hist, np.uint32)
    n = int(hist[1:].astype(np.int64).sum())
    filled = np.flatnonzero(hist[1:]) + 1
    out = dict(under=int(hist[0]), over=int(hist[513]), metered=n, anchorL=F32(0), whiteL=F32(0), exposure=F32(0),
               minBin=int(filled[0]) if n else 0, maxBin=int(filled[-1]) if n else 0)
    if n:
        out["anchorL"] = value(hist, n, percentile)
        out["whiteL"] = value(hist, n, white_percentile)
        out["exposure"] = F32(np.log2(F64(F32(key)) / F64(out["anchorL"])))
    return out


def _params(cls, default, **kw):
    p = cls()
    getattr(capi.lib(), default)(C.byref(p))
    for k, v in kw.items():
        if k.startswith("reserved"):
            p.reserved[int(k[len("reserved"):])] = v
        else:
            setattr(p, k, v)
    return p


def _meter(**kw):
    return _params(capi.KajoMeterParams, "kajo_hip_default_meter_params", **kw)


def _despeckle(**kw):
    return _params(capi.KajoDespeckleParams, "kajo_hip_default_despeckle_params", **kw)


def _glare(**kw):
    return _params(capi.KajoGlareParams, "kajo_hip_default_glare_params", **kw)


def _tone(**kw):
    return _params(capi.KajoToneParams, "kajo_hip_default_tone_params", **kw)


def _denoise(**kw):
    return _params(capi.KajoDenoiseParams, "kajo_hip_default_denoise_params", **kw)


def _ref(p):
    return None if p is None else C.byref(p)


def run_evaluate(hist, L=None, **kw):
    L = L or capi.lib()
    hist = np.ascontiguousarray(hist, np.uint32)
    assert hist.shape == (BINS,)
    r = capi.KajoMeterResult()
    r.pixels, r.nonfinite = 1234567, 89
    rc = L.kajo_hip_meter_evaluate(hist.ctypes.data_as(C.c_void_p), C.byref(_meter(**kw)), C.byref(r))
    assert rc == 0, L.kajo_hip_last_error()
    assert (r.pixels, r.nonfinite, r.reserved) == (1234567, 89, 0)  # left as the caller set them
    return r


def check_evaluate(hist, **kw):
    got = run_evaluate(hist, **kw)
    want = evaluate(hist, **{dict(whitePercentile="white_percentile").get(k, k): v for k, v in kw.items()})
    for k in ("under", "over", "metered", "minBin", "maxBin"):
        assert getattr(got, k) == want[k], (k, getattr(got, k), want[k], kw)
    for k in ("anchorL", "whiteL"):
        assert F32(getattr(got, k)).view(np.uint32) == F32(want[k]).view(np.uint32), (k, getattr(got, k), want[k], kw)
    assert abs(F64(got.exposure) - F64(want["exposure"])) <= 1e-6, (got.exposure, want["exposure"], kw)
    return got


def test_header_structs_constants_binding_and_libraries_agree():
    header = _header()
    assert C.sizeof(capi.KajoMeterParams) == 32 and C.sizeof(capi.KajoMeterResult) == 64
    for name, cls in (("KajoMeterParams", capi.KajoMeterParams), ("KajoMeterResult", capi.KajoMeterResult)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        names = [n for line in re.findall(r"^\s+\w+ ([\w, \[\]]+);", fields, re.M) for n in re.sub(r"\[\d+\]", "", line).split(", ")]
        assert names == [f for f, _ in cls._fields_], (name, names)
    assert [f for f, _ in capi.KajoMeterParams._fields_] == ["percentile", "key", "whitePercentile", "flags", "reserved"]
    assert [f for f, _ in capi.KajoMeterResult._fields_] == ["pixels", "nonfinite", "under", "over", "metered", "anchorL", "whiteL", "exposure",
                                                              "minBin", "maxBin", "reserved"]
    assert capi.KajoMeterResult.anchorL.offset == 40 and capi.KajoMeterResult.minBin.offset == 52
    assert re.search(r"#define KAJO_METER_BINS 514\b", header) and capi.KAJO_METER_BINS == 514
    assert re.search(r"#define KAJO_METER_AUTO_WHITE 1u", header) and capi.KAJO_METER_AUTO_WHITE == 1
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        assert os.path.exists(lib), lib
        nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in ENTRY_POINTS + ("kajo_meter_launch", "kajo_meter_groups"):
            assert re.search(r"\bT %s\b" % name, nm), (lib, name)
    # the structs beside them keep their sizes
    assert C.sizeof(capi.KajoToneParams) == 32 and C.sizeof(capi.KajoDespeckleParams) == 32 and C.sizeof(capi.KajoGlareParams) == 32


@pytest.mark.parametrize("which", ["product", "tune"])
def test_default_params_are_the_documented_ones(which):
    L = capi.lib() if which == "product" else C.CDLL(os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so"))
    L.kajo_hip_default_meter_params.restype = None
    L.kajo_hip_default_meter_params.argtypes = [C.POINTER(capi.KajoMeterParams)]
    p = capi.KajoMeterParams()
    p.percentile, p.key, p.whitePercentile, p.flags = 0.9, 3.0, 0.1, 1
    p.reserved[3] = 7.0
    L.kajo_hip_default_meter_params(C.byref(p))
    assert (p.percentile, p.flags) == (0.5, 0)
    assert F32(p.key) == F32(0.18) and F32(p.whitePercentile) == F32(0.995)
    assert list(p.reserved) == [0.0, 0.0, 0.0, 0.0]
    L.kajo_hip_default_meter_params(None)  # accepted
    header = _header()
    for text in ("(default 0.5:", "finite (default 0.18)", "(default 0.995)"):
        assert text in header, text
    # the twin evaluates as the product does
    hist = np.zeros(BINS, np.uint32)
    hist[[0, 100, 300, 513]] = [5, 7, 9, 1]
    L.kajo_hip_meter_evaluate.argtypes = [C.c_void_p, C.POINTER(capi.KajoMeterParams), C.POINTER(capi.KajoMeterResult)]
    r = run_evaluate(hist, L)
    assert (r.under, r.over, r.metered, r.minBin, r.maxBin) == (5, 1, 17, 100, 513) and r.anchorL == centre(300) and r.whiteL == centre(513)


def test_bin_edges_and_centres_are_the_documented_floats():
    assert edge(1) == F32(2.0 ** -16) and edge(513) == F32(2.0 ** 16) and edge(17) == F32(2.0 ** -15) and edge(2) == F32(2.0 ** -16 * (1 + 1 / 16))
    assert centre(513) == F32(65536.0)
    for b in (1, 2, 16, 17, 255, 512):
        assert F64(centre(b)) == (F64(edge(b)) + F64(edge(b + 1))) / 2  # exact in float32
        assert edge(b) < centre(b) < edge(b + 1)


def _hist(**bins):
    h = np.zeros(BINS, np.uint32)
    for b, c in bins.items():
        h[int(b[1:])] = c
    return h


def test_evaluate_crafted_histograms():
    r = check_evaluate(_hist())  # empty
    assert (r.metered, r.exposure, r.whiteL, r.anchorL, r.minBin, r.maxBin) == (0, 0.0, 0.0, 0.0, 0, 0)
    r = check_evaluate(_hist(b0=1000))  # everything in bin 0: black does not meter
    assert (r.under, r.metered, r.exposure, r.whiteL, r.minBin, r.maxBin) == (1000, 0, 0.0, 0.0, 0, 0)
    r = check_evaluate(_hist(b200=12, b0=3))  # a single inner bin
    assert r.anchorL == r.whiteL == centre(200) and (r.minBin, r.maxBin, r.metered, r.under) == (200, 200, 12, 3)
    r = check_evaluate(_hist(b513=1))  # a single count in bin 513
    assert r.anchorL == r.whiteL == F32(65536.0) and (r.over, r.minBin, r.maxBin) == (1, 513, 513)
    # two bins of ten: rank 10 is the last count of the first, rank 11 the first count of the second
    two = _hist(b100=10, b300=10)
    r = check_evaluate(two, percentile=0.5, whitePercentile=0.55)
    assert r.anchorL == centre(100) and r.whiteL == centre(300)
    r = check_evaluate(two, percentile=float(F32(0.5) + F32(2.0 ** -24)), whitePercentile=0.5)
    assert r.anchorL == centre(300) and r.whiteL == centre(100)
    r = check_evaluate(two, percentile=1.0, whitePercentile=1.0)  # q = 1: the last metered pixel
    assert r.anchorL == r.whiteL == centre(300)
    r = check_evaluate(_hist(b5=1, b100=10, b300=10), percentile=2.0 ** -24, whitePercentile=2.0 ** -24)  # q = 2^-24: rank 1
    assert r.anchorL == centre(5)
    r = check_evaluate(_hist(b40=1 << 29, b41=3, b1=1), percentile=0.5, whitePercentile=1.0)  # 2^29 counts in one bin
    assert r.metered == (1 << 29) + 4 and r.anchorL == centre(40) and r.whiteL == centre(41)
    r = check_evaluate(_hist(b40=0xffffffff, b41=0xffffffff, b42=0xffffffff), percentile=0.34, whitePercentile=0.67)  # sums beyond 32 bits
    assert r.metered == 3 * 0xffffffff and r.anchorL == centre(41) and r.whiteL == centre(42)


def test_evaluate_200_random_histograms():
    rng = np.random.default_rng(514)
    for i in range(200):
        h = np.zeros(BINS, np.uint32)
        k = int(rng.integers(1, 60))
        where = rng.integers(0, BINS, k)
        h[where] = rng.integers(1, 1 << int(rng.integers(1, 24)), k)
        q, wq = (float(F32(x)) for x in rng.uniform(1e-6, 1.0, 2))
        key = float(F32(10.0 ** rng.uniform(-3, 2)))
        check_evaluate(h, percentile=q, whitePercentile=wq, key=key)


def _tone_of(result, meter, tone):
    out = capi.KajoToneParams()
    rc = capi.lib().kajo_hip_meter_tone(_ref(result), _ref(meter), _ref(tone), C.byref(out))
    return rc, out


def test_meter_tone_compensation_clamp_white_and_two_automatic_exposures():
    r = capi.KajoMeterResult()
    r.exposure, r.whiteL = 2.5, 12.0
    tone = _tone(curve=capi.KAJO_TONE_REINHARD, exposure=-1.25, white=3.0, key=0.4)
    rc, out = _tone_of(r, _meter(), tone)
    assert rc == 0 and out.exposure == 1.25 and out.white == 3.0  # the user's EV adds; without the flag the white stays
    assert (out.curve, out.flags, F32(out.key), list(out.reserved)) == (capi.KAJO_TONE_REINHARD, 0, F32(0.4), [0.0, 0.0, 0.0])
    rc, out = _tone_of(r, _meter(flags=capi.KAJO_METER_AUTO_WHITE), tone)
    # white = whiteL * 2^exposure in binary64, rounded once: within two float32 ulps of numpy's, whose exp2 may differ in the last place
    want = F64(12.0) * np.exp2(F64(1.25))
    assert rc == 0 and out.exposure == 1.25 and abs(F64(out.white) - want) <= 2 * 2.0 ** -24 * want
    r.exposure = 3.0
    rc, out = _tone_of(r, _meter(flags=capi.KAJO_METER_AUTO_WHITE), _tone(exposure=1.0))
    assert rc == 0 and out.exposure == 4.0 and out.white == 192.0  # (a power of two is exact)
    r.whiteL = 0.0
    rc, out = _tone_of(r, _meter(flags=capi.KAJO_METER_AUTO_WHITE), _tone(white=5.0))
    assert rc == 0 and out.white == 0.0  # a whiteL of 0 gives a white of 0
    for metered, user, want in ((30.0, 10.0, 32.0), (-30.0, -10.0, -32.0), (31.0, 1.0, 32.0), (40.0, -32.0, 8.0)):
        r.exposure = metered
        rc, out = _tone_of(r, _meter(), _tone(exposure=user))
        assert rc == 0 and out.exposure == want, (metered, user, out.exposure)
    L = capi.lib()
    rc, _ = _tone_of(r, _meter(), _tone(flags=capi.KAJO_TONE_AUTO_EXPOSURE))
    assert rc == capi.KAJO_E_INVALID and "two automatic exposures" in L.kajo_hip_last_error().decode()
    for args in ((None, _meter(), _tone()), (r, _meter(), None)):
        assert _tone_of(*args)[0] == capi.KAJO_E_INVALID
    assert L.kajo_hip_meter_tone(C.byref(r), C.byref(_meter()), C.byref(_tone()), None) == capi.KAJO_E_INVALID
    assert _tone_of(r, None, _tone())[0] == capi.KAJO_E_INVALID and L.kajo_hip_last_error().decode() == "null meter parameters"
    same = _tone(exposure=1.0)  # in and out may be one struct
    r.exposure = 1.0
    assert L.kajo_hip_meter_tone(C.byref(r), C.byref(_meter()), C.byref(same), C.byref(same)) == 0 and same.exposure == 2.0


def _refusals(m, despeckle=None, glare=None, tone=None, denoise=None):
    """What each entry point that takes meter parameters answers on a NULL handle: [(rc, message)] for kajo_hip_meter,
    kajo_hip_present_metered_argb8, kajo_hip_present_metered_gathered_argb8_device, kajo_hip_meter_evaluate, kajo_hip_meter_tone."""
    L = capi.lib()
    tone = tone or _tone()
    hist = np.zeros(BINS, np.uint32)
    r, out = capi.KajoMeterResult(), capi.KajoToneParams()
    res = []
    for call in (lambda: L.kajo_hip_meter(None, _ref(despeckle), _ref(denoise), _ref(glare), _ref(m), None, None),
                 lambda: L.kajo_hip_present_metered_argb8(None, _ref(despeckle), _ref(denoise), _ref(glare), _ref(m), _ref(tone), None, None),
                 lambda: L.kajo_hip_present_metered_gathered_argb8_device(None, None, _ref(despeckle), _ref(glare), _ref(m), _ref(tone), None, None),
                 lambda: L.kajo_hip_meter_evaluate(hist.ctypes.data_as(C.c_void_p), _ref(m), C.byref(r)),
                 lambda: L.kajo_hip_meter_tone(C.byref(r), _ref(m), _ref(tone), C.byref(out))):
        rc = call()
        res.append((rc, L.kajo_hip_last_error().decode()))
    return res


BAD = [
    (dict(percentile=0.0), "percentile"), (dict(percentile=-0.5), "percentile"), (dict(percentile=1.0001), "percentile"),
    (dict(percentile=float("nan")), "percentile"), (dict(percentile=float("inf")), "percentile"),
    (dict(whitePercentile=0.0), "white percentile"), (dict(whitePercentile=2.0), "white percentile"), (dict(whitePercentile=float("nan")), "white percentile"),
    (dict(key=0.0), "key"), (dict(key=-1.0), "key"), (dict(key=float("inf")), "key"), (dict(key=float("nan")), "key"),
    (dict(flags=2), "flag"), (dict(flags=0x80000001), "flag"), (dict(reserved0=1.0), "reserved"), (dict(reserved3=-2.0), "reserved"),
]


@pytest.mark.parametrize("bad,word", BAD)
def test_bad_parameters_are_refused_before_the_handle_is_looked_at(bad, word):
    for rc, msg in _refusals(_meter(**bad)):
        assert rc == capi.KAJO_E_INVALID and word in msg and "meter" in msg, (bad, rc, msg)


@pytest.mark.parametrize("ok", [dict(), dict(percentile=1.0), dict(percentile=2.0 ** -24), dict(whitePercentile=1.0), dict(key=1e-30), dict(key=1e30),
                                dict(flags=1)])
def test_good_parameters_pass_on_to_the_handle_check(ok):
    got = _refusals(_meter(**ok))
    for rc, msg in got[:3]:
        assert (rc, msg) in ((capi.KAJO_E_INVALID, "null handle"), (capi.KAJO_E_INVALID, "null argument")), (ok, rc, msg)
    assert got[3][0] == 0 and got[4][0] == 0


def test_null_meter_parameters():
    """kajo_hip_meter, _evaluate and _tone refuse them; for the two present entry points NULL means no metering: they are the present
    entry points, with their refusals."""
    meter, present, gathered, ev, tn = _refusals(None)
    assert meter == ev == tn == (capi.KAJO_E_INVALID, "null meter parameters")
    assert present == (capi.KAJO_E_INVALID, "null handle") and gathered == (capi.KAJO_E_INVALID, "null argument")
    _, present, gathered, _, _ = _refusals(None, glare=_glare(levels=13))
    assert "glare levels" in present[1] and "glare levels" in gathered[1]
    _, present, gathered, _, _ = _refusals(None, tone=_tone(flags=capi.KAJO_TONE_AUTO_EXPOSURE))  # not refused without metering
    assert present == (capi.KAJO_E_INVALID, "null handle") and gathered == (capi.KAJO_E_INVALID, "null argument")
    L = capi.lib()
    assert L.kajo_hip_meter_evaluate(None, C.byref(_meter()), C.byref(capi.KajoMeterResult())) == capi.KAJO_E_INVALID
    assert L.kajo_hip_meter_evaluate(np.zeros(BINS, np.uint32).ctypes.data_as(C.c_void_p), C.byref(_meter()), None) == capi.KAJO_E_INVALID


def test_order_of_refusals_despeckle_glare_meter_tone_denoise_handle():
    bad_s, bad_g, bad_m, bad_t, bad_d = _despeckle(rank=9), _glare(levels=13), _meter(key=0.0), _tone(curve=7), _denoise(iterations=9)
    for rc, msg in _refusals(bad_m, bad_s, bad_g, bad_t, bad_d)[:3]:
        assert rc == capi.KAJO_E_INVALID and "despeckle rank" in msg, msg
    for rc, msg in _refusals(bad_m, _despeckle(), bad_g, bad_t, bad_d)[:3]:
        assert rc == capi.KAJO_E_INVALID and "glare levels" in msg, msg
    for rc, msg in _refusals(bad_m, _despeckle(), _glare(), bad_t, bad_d)[:3]:
        assert rc == capi.KAJO_E_INVALID and "meter key" in msg, msg
    meter, present, gathered = _refusals(_meter(), _despeckle(), _glare(), bad_t, bad_d)[:3]
    assert "iterations" in meter[1] and "tone curve" in present[1] and "tone curve" in gathered[1]
    _, present, gathered = _refusals(_meter(), _despeckle(), _glare(), _tone(flags=capi.KAJO_TONE_AUTO_EXPOSURE), bad_d)[:3]
    assert "two automatic exposures" in present[1] and "two automatic exposures" in gathered[1]
    assert present[0] == gathered[0] == capi.KAJO_E_INVALID
    meter, present, gathered = _refusals(_meter(), _despeckle(), _glare(), _tone(), bad_d)[:3]
    assert "iterations" in meter[1] and "iterations" in present[1] and gathered[1] == "null argument"
    meter, present, _ = _refusals(_meter(), _despeckle(), _glare(), _tone(), _denoise())[:3]
    assert meter == present == (capi.KAJO_E_INVALID, "null handle")
    meter, present, _ = _refusals(_meter())[:3]  # every stage off
    assert meter == present == (capi.KAJO_E_INVALID, "null handle")
    L = capi.lib()
    assert L.kajo_hip_present_metered_argb8(None, None, None, None, C.byref(_meter()), None, None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_last_error().decode() == "null tone parameters"


def test_the_plan_is_exported_and_the_partials_stay_under_a_megabyte():
    L = capi.lib()
    rects = lambda W, H: ((W + 63) // 64) * ((H + 3) // 4)
    cap = L.kajo_meter_groups(1 << 14, 1 << 14)
    for W, H in ((1, 1), (64, 4), (65, 4), (64, 5), (1920, 1080), (3840, 2160), (1 << 14, 1 << 14), (1, 4 * cap), (1, 4 * cap + 1)):
        g = L.kajo_meter_groups(W, H)
        assert g == min(rects(W, H), cap) and g * (BINS + 1) * 4 <= 1000000, (W, H, g)


def _compile():
    b = devicecode.build("meter.hip")
    assert "-ffp-contract=off" in b.cmd and "--offload-arch=gfx950" in b.cmd
    return b.resources, b.asm


def test_meter_kernels_spill_nothing_and_use_no_scratch_flat_or_global_atomics():
    res, asm = _compile()
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k, (vgprs, lds) in KERNELS.items():
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        assert abs(r["VGPRs"] - vgprs) <= VGPR_ROOM and r["Occupancy"] == 8 and r["LDS Size"] == lds, (k, r)  # (full occupancy; LDS: 515 counters, the sum's 8 x 32 shares)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k  # (global_atomic_*, buffer_atomic_*: the LDS adds are ds_add_u32)
        # the rows of the partials and the result leave with vector stores, one word per lane
        assert set(re.findall(r"\n\s+(global_store_\w+|buffer_store_\w+)", body)) == {"global_store_dword"}, k
        loads = set(re.findall(r"\n\s+(global_load_\w+)", body))
        if k == "kajo_meter_hist":
            # one access per lane and pixel -- the float4, or its three colour words, .w is not used -- and LDS adds that return nothing
            assert loads and loads <= {"global_load_dwordx3", "global_load_dwordx4"}, loads
            assert "ds_add_u32" in body and "ds_add_rtn" not in body
        else:
            assert loads == {"global_load_dword"}, loads


def test_makefile_links_the_meter_into_the_product_and_the_tools_twin():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("meter.o" in l and "despeckle.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "meter.hip" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0], compiles


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--meter-exposure", "0"], "--meter-exposure must be a percentile in (0, 1]"),
    (["--meter-exposure", "1.5"], "--meter-exposure must be a percentile in (0, 1]"),
    (["--meter-exposure", "-0.5"], "--meter-exposure must be a percentile in (0, 1]"),
    (["--meter-exposure", "nan"], "--meter-exposure must be a percentile in (0, 1]"),
    (["--meter-exposure", "half"], "--meter-exposure must be a percentile in (0, 1]"),
    (["--tonemap", "reinhard", "--meter-white", "0"], "--meter-white must be a percentile in (0, 1]"),
    (["--tonemap", "reinhard", "--meter-white", "2"], "--meter-white must be a percentile in (0, 1]"),
    (["--tonemap", "reinhard", "--meter-white", "inf"], "--meter-white must be a percentile in (0, 1]"),
    (["--meter-white", "0.99"], "--meter-white sets the white point of --tonemap reinhard"),
    (["--tonemap", "aces", "--meter-white", "0.99"], "--meter-white sets the white point of --tonemap reinhard"),
    (["--meter-exposure", "0.5", "--auto-exposure"], "--meter-exposure and --auto-exposure are two automatic exposures"),
    (["--tonemap", "reinhard", "--meter-white", "0.99", "--auto-exposure"], "--meter-exposure and --auto-exposure are two automatic exposures"),
    (["--meter-exposure", "0.5", "--key", "0"], "--key must be a finite number > 0"),
    (["--meter-exposure", "0.5", "--three-arg"], "the meter options need the backend's options"),
])
def test_driver_refuses_bad_meter_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_meter_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--meter-exposure Q", "--meter-white Q", "meter_stops"):
        assert opt in text, opt
