"""Local tone mapping (include/kajo_hip.h kajo_hip_local*, kajo_amd/csrc/local.hip) without a GPU: the struct, constants and entry
points as the header declares them, in the product and the tools' twin; the documented defaults; every refusal that comes before a
device is looked at, and their order across the stages (despeckle, glare, local, meter, tone, denoise, handle); the driver's refusals;
and properties of the numpy restatement the GPU tests hold the kernels to (tests/local_replay.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kajo_amd import capi
from local_replay import DEFAULTS, restate, span, synthetic_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
ENTRY_POINTS = ("kajo_hip_default_local_params", "kajo_hip_local", "kajo_hip_present_local_argb8",
                "kajo_hip_present_local_gathered_argb8_device", "kajo_hip_local_pivot")
F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")


def _params(cls, default, **kw):
    p = cls()
    getattr(capi.lib(), default)(C.byref(p))
    for k, v in kw.items():
        if k.startswith("reserved") and k != "reserved":
            p.reserved[int(k[len("reserved"):])] = v
        else:
            setattr(p, k, v)
    return p


def _local(**kw):
    return _params(capi.KajoLocalParams, "kajo_hip_default_local_params", **kw)


def _despeckle(**kw):
    return _params(capi.KajoDespeckleParams, "kajo_hip_default_despeckle_params", **kw)


def _glare(**kw):
    return _params(capi.KajoGlareParams, "kajo_hip_default_glare_params", **kw)


def _meter(**kw):
    return _params(capi.KajoMeterParams, "kajo_hip_default_meter_params", **kw)


def _tone(**kw):
    return _params(capi.KajoToneParams, "kajo_hip_default_tone_params", **kw)


def _denoise(**kw):
    return _params(capi.KajoDenoiseParams, "kajo_hip_default_denoise_params", **kw)


def _ref(p):
    return None if p is None else C.byref(p)


def _error():
    return (capi.lib().kajo_hip_last_error() or b"").decode()


def test_header_struct_constants_binding_and_libraries_agree():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    assert C.sizeof(capi.KajoLocalParams) == 32
    fields = re.search(r"typedef struct KajoLocalParams \{(.*?)\} KajoLocalParams;", header, re.S).group(1)
    names = re.findall(r"^\s+\w+ (\w+);", fields, re.M)
    assert names == [f for f, _ in capi.KajoLocalParams._fields_] == ["iterations", "flags", "compression", "detail", "sigmaRange", "pivot",
                                                                      "pivotPercentile", "reserved"]
    assert re.search(r"#define KAJO_LOCAL_PIVOT_METERED 1u", header) and capi.KAJO_LOCAL_PIVOT_METERED == 1
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        L = C.CDLL(lib)
        for name in ENTRY_POINTS:
            assert hasattr(L, name), (lib, name)
    version = capi.lib().kajo_hip_version()
    assert b"gfx950" in version and b"aov-matte" in version and b"local" in version


def test_defaults():
    p = capi.KajoLocalParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    capi.lib().kajo_hip_default_local_params(C.byref(p))
    assert (p.iterations, p.flags, p.reserved) == (5, 0, 0.0)
    assert F32(p.compression) == F32(0.6) and p.detail == 1.0 and p.sigmaRange == 2.0 and p.pivotPercentile == 0.5
    assert F32(p.pivot) == F32(np.log2(0.18))
    capi.lib().kajo_hip_default_local_params(None)  # NULL is accepted


BAD_FIELDS = [
    (dict(iterations=-1), "local iterations must be in [0, 8]"),
    (dict(iterations=9), "local iterations must be in [0, 8]"),
    (dict(flags=2), "unknown local flag"),
    (dict(flags=0x80000001), "unknown local flag"),
    (dict(compression=0.0), "local compression must be finite and in (0, 1]"),
    (dict(compression=-0.5), "local compression must be finite and in (0, 1]"),
    (dict(compression=1.0001), "local compression must be finite and in (0, 1]"),
    (dict(compression=NAN), "local compression must be finite and in (0, 1]"),
    (dict(compression=INF), "local compression must be finite and in (0, 1]"),
    (dict(detail=-0.1), "local detail must be finite and in [0, 4]"),
    (dict(detail=4.5), "local detail must be finite and in [0, 4]"),
    (dict(detail=NAN), "local detail must be finite and in [0, 4]"),
    (dict(detail=INF), "local detail must be finite and in [0, 4]"),
    (dict(sigmaRange=0.0), "local range sigma must be finite and positive"),
    (dict(sigmaRange=-1.0), "local range sigma must be finite and positive"),
    (dict(sigmaRange=NAN), "local range sigma must be finite and positive"),
    (dict(sigmaRange=INF), "local range sigma must be finite and positive"),
    (dict(pivot=-16.5), "local pivot must be finite and in [-16, 16]"),
    (dict(pivot=17.0), "local pivot must be finite and in [-16, 16]"),
    (dict(pivot=NAN), "local pivot must be finite and in [-16, 16]"),
    (dict(pivot=-INF), "local pivot must be finite and in [-16, 16]"),
    (dict(pivotPercentile=0.0), "local pivot percentile must be finite and in (0, 1]"),
    (dict(pivotPercentile=1.5), "local pivot percentile must be finite and in (0, 1]"),
    (dict(pivotPercentile=NAN), "local pivot percentile must be finite and in (0, 1]"),
    (dict(flags=1, pivotPercentile=INF), "local pivot percentile must be finite and in (0, 1]"),
    (dict(reserved=1.0), "local reserved fields must be 0"),
    (dict(reserved=NAN), "local reserved fields must be 0"),
]


def _calls(local, despeckle=None, denoise=None, glare=None, meter=None, tone=None):
    """the three entry points that take the stage's parameters, with a NULL handle: -> [(name, rc, message)]"""
    L = capi.lib()
    tone = tone if tone is not None else _tone()
    dst = C.c_void_p(16)  # (never written: every call here is refused before a device is looked at)
    out = []
    rc = L.kajo_hip_local(None, _ref(despeckle), _ref(denoise), _ref(glare), _ref(local), None)
    out.append(("local", rc, _error()))
    rc = L.kajo_hip_present_local_argb8(None, _ref(despeckle), _ref(denoise), _ref(glare), _ref(local), _ref(meter), C.byref(tone), None, None)
    out.append(("present", rc, _error()))
    rc = L.kajo_hip_present_local_gathered_argb8_device(None, None, _ref(despeckle), _ref(glare), _ref(local), _ref(meter), C.byref(tone), dst, None)
    out.append(("gathered", rc, _error()))
    return out


@pytest.mark.parametrize("fields,message", BAD_FIELDS, ids=["%s" % sorted(f.items()) for f, _ in BAD_FIELDS])
def test_every_refusal_comes_before_the_handle(fields, message):
    for name, rc, text in _calls(_local(**fields)):
        assert rc == capi.KAJO_E_INVALID and text == message, (name, rc, text)


def test_the_edges_of_the_ranges_are_accepted_and_a_null_struct_is_not():
    for fields in (dict(iterations=0), dict(iterations=8), dict(compression=1.0), dict(compression=1e-6), dict(detail=0.0), dict(detail=4.0),
                   dict(sigmaRange=1e-6), dict(pivot=-16.0), dict(pivot=16.0), dict(pivotPercentile=1.0), dict(flags=1)):
        for name, rc, text in _calls(_local(**fields)):
            assert rc == capi.KAJO_E_INVALID and text in ("null handle", "null argument"), (fields, name, text)
    L = capi.lib()
    assert L.kajo_hip_local(None, None, None, None, None, None) == capi.KAJO_E_INVALID and _error() == "null local parameters"
    pivot = C.c_float()
    assert L.kajo_hip_local_pivot(None, C.byref(pivot)) == capi.KAJO_E_INVALID
    # local == NULL in the chain entries is the metered call: its refusals, not this stage's
    assert L.kajo_hip_present_local_argb8(None, None, None, None, None, None, C.byref(_tone()), None, None) == capi.KAJO_E_INVALID
    assert _error() == "null handle"
    assert L.kajo_hip_present_local_argb8(None, None, None, None, None, C.byref(_meter(key=0.0)), C.byref(_tone()), None, None) == capi.KAJO_E_INVALID
    assert _error() == "meter key must be finite and positive"


def test_the_order_of_refusals_across_the_stages():
    """despeckle, glare, local, meter, tone, denoise, handle: each stage's bad parameters are reported while everything after it is bad
    too."""
    bad = dict(despeckle=_despeckle(rank=9), glare=_glare(levels=99), local=_local(detail=9.0), meter=_meter(key=-1.0),
               tone=_tone(exposure=99.0), denoise=_denoise(iterations=99))
    good = dict(despeckle=_despeckle(), glare=_glare(), local=_local(), meter=_meter(), tone=_tone(), denoise=_denoise())
    messages = dict(despeckle="despeckle rank must be in [1, 4]", glare="glare levels must be in [0, 12]",
                    local="local detail must be finite and in [0, 4]", meter="meter key must be finite and positive",
                    tone="tone exposure must be finite and in [-32, 32]", denoise="denoise iterations must be in [0, 8]")
    order = ["despeckle", "glare", "local", "meter", "tone", "denoise"]
    for i, first in enumerate(order):
        args = {k: (good[k] if order.index(k) < i else bad[k]) for k in order}
        for name, rc, text in _calls(**args):
            assert rc == capi.KAJO_E_INVALID, (first, name)
            # (kajo_hip_local takes no meter and no tone; the gathered twin no denoiser)
            takes = dict(local=("despeckle", "glare", "local", "denoise"), present=order, gathered=("despeckle", "glare", "local", "meter", "tone"))[name]
            want = next((messages[k] for k in order[i:] if k in takes), None)
            assert text == (want or ("null argument" if name == "gathered" else "null handle")), (first, name, text)
    for name, rc, text in _calls(**good):
        assert rc == capi.KAJO_E_INVALID and text in ("null handle", "null argument"), (name, text)
    # the metered exposure and the tone parameters' automatic exposure: refused with the tone parameters, before the denoiser's
    for name, rc, text in _calls(local=_local(), meter=_meter(), tone=_tone(flags=capi.KAJO_TONE_AUTO_EXPOSURE), denoise=bad["denoise"])[1:]:
        assert rc == capi.KAJO_E_INVALID and "two automatic exposures" in text, (name, text)


def test_makefile_links_the_stage_into_the_product_and_the_tools_twin():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("local.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "local.hip" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0] and "gfx950" in compiles[0], compiles


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--local-contrast", "0"], "local compression must be finite and in (0, 1]"),
    (["--local-contrast", "1.5"], "local compression must be finite and in (0, 1]"),
    (["--local-contrast", "nan"], "local compression must be finite and in (0, 1]"),
    (["--local-contrast", "low"], "local compression must be finite and in (0, 1]"),
    (["--local-contrast", "0.6", "--local-detail", "-1"], "local detail must be finite and in [0, 4]"),
    (["--local-contrast", "0.6", "--local-detail", "4.5"], "local detail must be finite and in [0, 4]"),
    (["--local-contrast", "0.6", "--local-range", "0"], "local range sigma must be finite and positive"),
    (["--local-contrast", "0.6", "--local-range", "inf"], "local range sigma must be finite and positive"),
    (["--local-contrast", "0.6", "--local-iterations", "9"], "local iterations must be in [0, 8]"),
    (["--local-contrast", "0.6", "--local-iterations", "-1"], "local iterations must be in [0, 8]"),
    (["--local-contrast", "0.6", "--local-iterations", "2x"], "local iterations must be in [0, 8]"),
    (["--local-contrast", "0.6", "--local-pivot", "17"], "local pivot must be finite and in [-16, 16]"),
    (["--local-contrast", "0.6", "--local-pivot", "median"], "local pivot must be finite and in [-16, 16]"),
    (["--local-contrast", "0.6", "--local-pivot", "meteredx"], "local pivot must be finite and in [-16, 16]"),
    (["--local-contrast", "0.6", "--local-pivot", "metered:0"], "local pivot percentile must be finite and in (0, 1]"),
    (["--local-contrast", "0.6", "--local-pivot", "metered:1.5"], "local pivot percentile must be finite and in (0, 1]"),
    (["--local-contrast", "0.6", "--local-pivot", "metered:"], "local pivot percentile must be finite and in (0, 1]"),
    (["--local-detail", "2"], "shape the stage that --local-contrast turns on"),
    (["--local-pivot", "metered"], "shape the stage that --local-contrast turns on"),
    (["--local-contrast", "0.6", "--three-arg"], "the local tone mapping options need the backend's options"),
])
def test_driver_refuses_bad_local_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_local_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--local-contrast C", "--local-detail D", "--local-range STOPS", "--local-iterations K", "--local-pivot STOPS|metered[:Q]",
                "local_pivot"):
        assert opt in text, opt
    assert text.index("--local-contrast C") > text.index("    -v  ")  # appended: the lines that were there stay where they were


# -- the restatement itself ---------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _constant_formula(m, L, compression, pivot):
    """m * 2^((c - 1)(L - pivot)): what a frame whose base layer equals its log luminance maps to"""
    return m * np.exp2((F64(F32(compression)) - 1.0) * (L - F64(F32(pivot))))


def test_restatement_copy_case():
    for name, F in synthetic_frames(41, 23, 3).items():
        r = restate(F, 3, compression=1.0, detail=1.0, iterations=4)
        assert np.array_equal(_bits(r["out"]), _bits(F)), name


def test_restatement_constant_frame():
    P = 4
    c = F32([0.7, 0.25, 1.3])
    F = np.empty((9, 13, 4), F32)
    F[..., :3] = c * F32(P)
    F[..., 3] = 2.0
    for K in (0, 1, 5, 8):
        for comp in (0.4, 0.6):
            for detail in (0.0, 1.0, 2.0):
                r = restate(F, P, iterations=K, compression=comp, detail=detail)
                want = _constant_formula(r["m"].astype(F64), r["L"][..., None], comp, DEFAULTS["pivot"]) * P
                assert np.allclose(r["out"][..., :3], want, rtol=1e-12, atol=0), (K, comp, detail)
                assert np.array_equal(r["out"][..., 3], F[..., 3])


def test_restatement_zero_iterations_is_the_power_curve():
    P = 3
    F = synthetic_frames(41, 23, P)["checker"]
    for comp, detail, pivot in ((0.4, 1.0, -2.0), (0.6, 2.0, 1.5), (1.0, 0.0, 0.0)):
        r = restate(F, P, iterations=0, compression=comp, detail=detail, pivot=pivot)
        assert np.array_equal(r["B"], r["L"])
        # B = L: the detail layer is zero whatever its factor, and L' - L = (c - 1)(L - pivot): l -> l^c about the pivot
        want = _constant_formula(r["m"].astype(F64), r["L"][..., None], comp, pivot) * P
        assert np.allclose(r["out"][..., :3], want, rtol=1e-12, atol=0), (comp, detail, pivot)


def test_restatement_step_frame_has_no_halo():
    """left 0.01, right 100, sigmaRange 2: the cross-edge weight is 2^-(13.29 / 2)^2 < 2^-44, so each side comes out constant and equal
    to the constant-frame formula to 1e-9 relative -- no halo, where a linear blur would smear the edge over 2^K pixels."""
    P = 2
    H, W = 24, 40
    F = np.ones((H, W, 4), F32)
    F[:, :W // 2, :3] = F32(0.01) * P
    F[:, W // 2:, :3] = F32(100.0) * P
    for K in (1, 3, 5, 8):
        for comp in (0.4, 0.6):
            r = restate(F, P, iterations=K, compression=comp, sigma_range=2.0)
            want = _constant_formula(r["m"].astype(F64), r["L"][..., None], comp, DEFAULTS["pivot"]) * P
            rel = np.abs(r["out"][..., :3] - want) / want
            assert rel.max() <= 1e-9, (K, comp, rel.max())
            for side in (r["out"][:, :W // 2, :3], r["out"][:, W // 2:, :3]):
                assert np.ptp(side.reshape(-1, 3), axis=0).max() <= 1e-9 * side.max(), (K, comp)


def test_restatement_never_spreads_a_poisoned_pixel():
    P = 3
    for W, H in ((7, 5), (41, 23)):
        F = synthetic_frames(W, H, P)["poisoned"]
        for K in (0, 1, 5, 8):
            r = restate(F, P, iterations=K, compression=0.4, detail=2.0, sigma_range=0.5)
            c = r["counts"]
            assert 4 <= (~c).sum() <= 6 and c.sum() >= 29
            assert np.array_equal(_bits(r["out"][~c]), _bits(F[~c])), K  # the pixels that do not count: the bits they went in with
            assert np.isfinite(r["out"][c][:, :3]).all(), K              # no neighbour became non-finite
            assert np.array_equal(r["out"][..., 3], F[..., 3].astype(F64))
            assert np.isnan(r["B"][~c]).all() and np.isfinite(r["B"][c]).all()
        # a negative channel counts: it is clamped for the luminance and scaled by g like the others
        neg = (F[..., :3] < 0).any(-1) & c
        assert neg.any() and (r["out"][neg][:, :3].min(-1) < 0).all()


def test_compression_shrinks_the_span_of_the_checkerboard():
    """compression < 1 strictly shrinks maxBin - minBin of the meter's histogram (restated from the header in local_replay.meter_bins)
    on the checkerboard spanning 1e-3 .. 1e3, at every K."""
    P = 3
    F = synthetic_frames(41, 23, P)["checker"]
    before = span(F, P)
    assert before > 16 * 15  # (over fifteen stops)
    for K in (0, 1, 3, 5, 8):
        for comp in (0.4, 0.6, 0.9):
            out = restate(F, P, iterations=K, compression=comp)["out"].astype(F32)
            after = span(out, P)
            assert 0 < after < before, (K, comp, after, before)
    assert span(restate(F, P, compression=1.0, detail=1.0)["out"].astype(F32), P) == before
