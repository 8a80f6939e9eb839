"""The grade (include/kajo_hip.h "The grade", kajo_amd/csrc/grade.hip, grade_math.h) without a GPU: the structs, constants and entry
points as the header declares them, in the product and the tools' twin; the defaults; every refusal that comes before a device is
looked at, and their order across the stages (despeckle, grade, lens, glare, local, meter, tone, view, denoise, handle); the host's
kajo_hip_grade_pixels against the binary64 restatement within the derived allowance and against the float32 one word for word
(tests/grade_replay.py); the white balance helpers; the Makefile's plan; the kernels' budgets from the compiler's remarks; and the
arithmetic under AddressSanitizer + UBSan in a program of its own (tools/grade_san.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import devicecode
from kajo_amd import capi
from kajo_amd.renderer import grade_neutral, grade_params, grade_pixels, grade_white_balance
from grade_replay import XYZ_TO_SRGB, fill, illuminant_rgb, planckian_xy, restate32, restate64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
ENTRY_POINTS = ("kajo_hip_default_grade_params", "kajo_hip_grade_pixels", "kajo_hip_grade_white_balance", "kajo_hip_grade_neutral",
                "kajo_hip_grade", "kajo_hip_present_grade_argb8", "kajo_hip_present_grade_gathered_argb8_device")
F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
LIBS = [capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _default(cls, name, L=None):
    p = cls()
    getattr(L or capi.lib(), name)(C.byref(p))
    return p


def _grade(**kw):
    return grade_params(**kw)


def _ref(p):
    return None if p is None else C.byref(p)


def _error(L=None):
    L = L or capi.lib()
    L.kajo_hip_last_error.restype = C.c_char_p
    return (L.kajo_hip_last_error() or b"").decode()


def test_header_structs_constants_binding_and_libraries_agree():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    assert C.sizeof(capi.KajoGradeOp) == 48 and C.sizeof(capi.KajoGradeRegion) == 128 and C.sizeof(capi.KajoGradeParams) == 576
    want = dict(KajoGradeOp=["slope", "offset", "power", "saturation", "reserved"],
                KajoGradeRegion=["op", "objects", "n", "amount", "reserved"],
                KajoGradeParams=["global", "nRegions", "flags", "reserved", "regions"])
    for name, fields in want.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        names = re.findall(r"^\s+\w+ (\w+)(?:\[\w+\])?;", body, re.M)
        assert names == fields == [f.rstrip("_") for f, _ in getattr(capi, name)._fields_], (name, names)
    O, R, P = capi.KajoGradeOp, capi.KajoGradeRegion, capi.KajoGradeParams
    assert (O.slope.offset, O.offset.offset, O.power.offset, O.saturation.offset, O.reserved.offset) == (0, 12, 24, 36, 40)
    assert (R.op.offset, R.objects.offset, R.n.offset, R.amount.offset, R.reserved.offset) == (0, 48, 112, 116, 120)
    assert (P.global_.offset, P.nRegions.offset, P.flags.offset, P.reserved.offset, P.regions.offset) == (0, 48, 52, 56, 64)
    assert re.search(r"#define KAJO_GRADE_MAX_REGIONS 4\b", header) and capi.KAJO_GRADE_MAX_REGIONS == 4
    assert re.search(r"#define KAJO_GRADE_REGION_OBJECTS 16\b", header) and capi.KAJO_GRADE_REGION_OBJECTS == 16
    for text in ("48 bytes", "128 bytes", "576 bytes", "THE IDENTITY CASE", "Nothing is clamped above".lower()):
        assert text in header or text in header.lower(), text
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in LIBS:
        L = C.CDLL(lib)
        for name in ENTRY_POINTS:
            assert hasattr(L, name), (lib, name)
    assert b"grade" in capi.lib().kajo_hip_version().split(b";")[-1]


def test_defaults():
    p = capi.KajoGradeParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    capi.lib().kajo_hip_default_grade_params(C.byref(p))
    ops = [p.global_] + [r.op for r in p.regions]
    for op in ops:
        assert list(op.slope) == [1.0] * 3 and list(op.offset) == [0.0] * 3 and list(op.power) == [1.0] * 3
        assert op.saturation == 1.0 and list(op.reserved) == [0.0] * 2
    assert p.nRegions == 0 and p.flags == 0 and list(p.reserved) == [0, 0]
    for r in p.regions:
        assert r.amount == 1.0 and r.n == 0 and list(r.objects) == [0] * 16 and list(r.reserved) == [0, 0]
    capi.lib().kajo_hip_default_grade_params(None)  # NULL is accepted


def _bad_cases():
    """(a function that spoils default params, the message)"""
    slope = "grade slope must be finite and in [0, 65536]"
    offset = "grade offset must be finite and in [-65536, 65536]"
    power = "grade power must be finite and in [1/8, 8]"
    sat = "grade saturation must be finite and in [0, 4]"
    res = "grade reserved fields must be 0"
    ident = "object id out of range: 0 (the background) .. the number of planes and spheres"
    cases = []

    def op_cases(get, what):
        for c, v in ((0, -1e-3), (1, 65536.5), (2, NAN), (0, INF)):
            cases.append(("%s slope[%d]=%r" % (what, c, v), lambda p, c=c, v=v: get(p).slope.__setitem__(c, v), slope))
        for c, v in ((0, -65537.0), (1, 65537.0), (2, NAN), (1, -INF)):
            cases.append(("%s offset[%d]=%r" % (what, c, v), lambda p, c=c, v=v: get(p).offset.__setitem__(c, v), offset))
        for c, v in ((0, 0.1249), (1, 8.001), (2, NAN), (0, 0.0), (2, INF)):
            cases.append(("%s power[%d]=%r" % (what, c, v), lambda p, c=c, v=v: get(p).power.__setitem__(c, v), power))
        for v in (-0.01, 4.01, NAN, INF):
            cases.append(("%s saturation=%r" % (what, v), lambda p, v=v: setattr(get(p), "saturation", v), sat))
        for i, v in ((0, 1.0), (1, NAN)):
            cases.append(("%s reserved[%d]=%r" % (what, i, v), lambda p, i=i, v=v: get(p).reserved.__setitem__(i, v), res))

    op_cases(lambda p: p.global_, "global")

    def region(p, k=0):
        p.nRegions = max(p.nRegions, k + 1)
        for r in p.regions[:p.nRegions]:
            if r.n == 0:
                r.n = 1
        return p.regions[k]

    op_cases(lambda p: region(p, 0).op, "region0")
    op_cases(lambda p: region(p, 3).op, "region3")
    cases.append(("nRegions=-1", lambda p: setattr(p, "nRegions", -1), "grade regions must number 0 to 4"))
    cases.append(("nRegions=5", lambda p: setattr(p, "nRegions", 5), "grade regions must number 0 to 4"))
    cases.append(("flags=1", lambda p: setattr(p, "flags", 1), "unknown grade flag"))
    cases.append(("flags=2^31", lambda p: setattr(p, "flags", 0x80000000), "unknown grade flag"))
    cases.append(("reserved[0]", lambda p: p.reserved.__setitem__(0, 1), res))
    cases.append(("reserved[1]", lambda p: p.reserved.__setitem__(1, 7), res))
    cases.append(("n=0", lambda p: setattr(region(p, 1), "n", 0), "a grade region selects 1 to 16 objects"))
    cases.append(("n=17", lambda p: setattr(region(p, 0), "n", 17), "a grade region selects 1 to 16 objects"))
    cases.append(("id=-1", lambda p: region(p, 2).objects.__setitem__(0, -1), ident))
    for v in (-0.01, 1.01, NAN, INF):
        cases.append(("amount=%r" % v, lambda p, v=v: setattr(region(p, 1), "amount", v), "grade region amount must be finite and in [0, 1]"))
    cases.append(("region reserved", lambda p: region(p, 0).reserved.__setitem__(1, 1), res))
    return cases


BAD = _bad_cases()


def _calls(L, grade, despeckle=None, denoise=None, lens=None, glare=None, local=None, meter=None, tone=None, view=None):
    """the entry points that take the stage's parameters, with a NULL handle: -> [(name, rc, message)]"""
    tone = tone if tone is not None else _default(capi.KajoToneParams, "kajo_hip_default_tone_params", L)
    out = []
    rc = L.kajo_hip_grade(None, _ref(despeckle), _ref(denoise), _ref(grade), None)
    out.append(("grade", rc, _error(L)))
    rc = L.kajo_hip_present_grade_argb8(None, _ref(despeckle), _ref(denoise), _ref(grade), _ref(lens), _ref(glare), _ref(local), _ref(meter),
                                        C.byref(tone), _ref(view), None, None)
    out.append(("present", rc, _error(L)))
    rc = L.kajo_hip_present_grade_gathered_argb8_device(None, None, _ref(despeckle), _ref(grade), _ref(glare), _ref(local), _ref(meter),
                                                        C.byref(tone), _ref(view), None, None)
    out.append(("gathered", rc, _error(L)))
    rgb = (C.c_float * 3)(0.5, 0.25, 0.125)
    masks = (C.c_float * 4)(1, 1, 1, 1)
    rc = L.kajo_hip_grade_pixels(_ref(grade), rgb, masks, 1, rgb)
    out.append(("pixels", rc, _error(L)))
    return out


@pytest.mark.parametrize("lib", LIBS, ids=["product", "tune"])
def test_every_refusal_comes_before_the_handle(lib):
    L = C.CDLL(lib)
    for what, spoil, message in BAD:
        p = _default(capi.KajoGradeParams, "kajo_hip_default_grade_params", L)
        spoil(p)
        for name, rc, text in _calls(L, p):
            assert rc == capi.KAJO_E_INVALID and text == message, (what, name, rc, text)
    for name, rc, text in _calls(L, None)[:1] + _calls(L, None)[3:]:
        assert rc == capi.KAJO_E_INVALID and text == "null grade parameters", (name, text)


def test_the_edges_of_the_ranges_are_accepted_and_null_means_the_existing_call():
    L = capi.lib()
    edges = [dict(slope=0.0), dict(slope=65536.0), dict(offset=-65536.0), dict(offset=65536.0), dict(power=0.125), dict(power=8.0),
             dict(saturation=0.0), dict(saturation=4.0), dict(regions=[dict(objects=range(16), amount=0.0)]),
             dict(regions=[dict(objects=[0], amount=1.0)] * 4)]
    for e in edges:
        p = _grade(**e)
        for name, rc, text in _calls(L, p):
            if name == "pixels":
                assert rc == 0, (e, text)
            elif name == "gathered" and p.nRegions:
                assert rc == capi.KAJO_E_INVALID and "whole frame's coverage tables" in text, (e, text)
            else:
                assert rc == capi.KAJO_E_INVALID and text in ("null handle", "null argument"), (e, name, text)
    # a region that is not in use is not read
    p = _grade()
    p.regions[2].n = 99
    p.regions[2].op.slope[0] = NAN
    assert L.kajo_hip_grade(None, None, None, C.byref(p), None) == capi.KAJO_E_INVALID and _error() == "null handle"
    # grade == NULL in the chain entries: kajo_hip_present_view_argb8's refusals and its twin's
    tone = _default(capi.KajoToneParams, "kajo_hip_default_tone_params")
    local = _default(capi.KajoLocalParams, "kajo_hip_default_local_params")
    local.detail = 9.0
    for view in (None, _default(capi.KajoViewParams, "kajo_hip_default_view_params")):
        a = L.kajo_hip_present_grade_argb8(None, None, None, None, None, None, C.byref(local), None, C.byref(tone), _ref(view), None, None)
        ea = _error()
        b = L.kajo_hip_present_view_argb8(None, None, None, None, None, C.byref(local), None, C.byref(tone), _ref(view), None, None)
        assert (a, ea) == (b, _error()) == (capi.KAJO_E_INVALID, "local detail must be finite and in [0, 4]")
        a = L.kajo_hip_present_grade_gathered_argb8_device(None, None, None, None, None, None, None, C.byref(tone), _ref(view), None, None)
        ea = _error()
        b = L.kajo_hip_present_view_gathered_argb8_device(None, None, None, None, None, None, C.byref(tone), _ref(view), None, None)
        assert (a, ea) == (b, _error()) and a == capi.KAJO_E_INVALID


@pytest.mark.parametrize("lib", LIBS, ids=["product", "tune"])
def test_the_order_of_refusals_across_the_stages(lib):
    """despeckle, grade, lens, glare, local, meter, tone, view, denoise, handle: each stage's bad parameters are reported while everything
    after it is bad too."""
    L = C.CDLL(lib)
    def d(cls, name, **kw):
        p = _default(cls, name, L)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    mk = dict(despeckle=lambda **kw: d(capi.KajoDespeckleParams, "kajo_hip_default_despeckle_params", **kw),
              lens=lambda **kw: d(capi.KajoLensParams, "kajo_hip_default_lens_params", **kw),
              glare=lambda **kw: d(capi.KajoGlareParams, "kajo_hip_default_glare_params", **kw),
              local=lambda **kw: d(capi.KajoLocalParams, "kajo_hip_default_local_params", **kw),
              meter=lambda **kw: d(capi.KajoMeterParams, "kajo_hip_default_meter_params", **kw),
              tone=lambda **kw: d(capi.KajoToneParams, "kajo_hip_default_tone_params", **kw),
              view=lambda **kw: d(capi.KajoViewParams, "kajo_hip_default_view_params", **kw),
              denoise=lambda **kw: d(capi.KajoDenoiseParams, "kajo_hip_default_denoise_params", **kw))
    bad_grade = _grade()
    bad_grade.global_.saturation = 9.0
    bad = dict(despeckle=mk["despeckle"](rank=9), grade=bad_grade, lens=mk["lens"](maxRadius=99), glare=mk["glare"](levels=99),
               local=mk["local"](detail=9.0), meter=mk["meter"](key=-1.0), tone=mk["tone"](exposure=99.0), view=mk["view"](outW=8, outH=0),
               denoise=mk["denoise"](iterations=99))
    good = dict(despeckle=mk["despeckle"](flags=0), grade=_grade(saturation=0.5), lens=mk["lens"](flags=0), glare=mk["glare"](flags=0),
                local=mk["local"](flags=0), meter=mk["meter"](flags=0), tone=mk["tone"](flags=0), view=mk["view"](outW=8, outH=8),
                denoise=mk["denoise"](flags=0))
    messages = dict(despeckle="despeckle rank must be in [1, 4]", grade="grade saturation must be finite and in [0, 4]",
                    lens="lens max radius must be in [1, 16]", glare="glare levels must be in [0, 12]",
                    local="local detail must be finite and in [0, 4]", meter="meter key must be finite and positive",
                    tone="tone exposure must be finite and in [-32, 32]", view="view output size must be in [1, 16384]",
                    denoise="denoise iterations must be in [0, 8]")
    order = ["despeckle", "grade", "lens", "glare", "local", "meter", "tone", "view", "denoise"]
    takes = dict(grade=("despeckle", "grade", "denoise"), present=order,
                 gathered=("despeckle", "grade", "glare", "local", "meter", "tone", "view"), pixels=("grade",))
    for i, first in enumerate(order):
        args = {k: (good[k] if order.index(k) < i else bad[k]) for k in order}
        for name, rc, text in _calls(L, **args):
            want = next((messages[k] for k in order[i:] if k in takes[name]), None)
            if name == "pixels" and want is None:
                assert rc == 0
                continue
            assert rc == capi.KAJO_E_INVALID, (first, name)
            assert text == (want or ("null argument" if name == "gathered" else "null handle")), (first, name, text)
    # the metered exposure and the tone parameters' automatic exposure: refused with the tone parameters, before the view's and the denoiser's
    tone = mk["tone"](flags=capi.KAJO_TONE_AUTO_EXPOSURE)
    name, rc, text = _calls(L, grade=good["grade"], meter=good["meter"], tone=tone, view=bad["view"], denoise=bad["denoise"])[1]
    assert rc == capi.KAJO_E_INVALID and "two automatic exposures" in text, (name, text)
    # regions on the gathered twin: refused with the stage's parameters, in front of the null handle
    regions = _grade(regions=[dict(objects=[1])])
    name, rc, text = _calls(L, grade=regions)[2]
    assert rc == capi.KAJO_E_INVALID and "whole frame's coverage tables" in text


def test_makefile_compiles_the_stage_once_and_links_it_twice():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("grade.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "grade.hip" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0] and "-fno-slp-vectorize" in compiles[0] and "gfx950" in compiles[0]
    head = open(os.path.join(CSRC, "Makefile")).read().split("HIPCC")[0]  # the header comment
    assert "grade.hip" in head and "grade_math.h" in head


BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--grade-slope", "1,2"], "take three numbers R,G,B"),
    (["--grade-offset", "1"], "take three numbers R,G,B"),
    (["--grade-slope", "1,-0.5,1"], "grade slope must be finite and in [0, 65536]"),
    (["--grade-slope", "1,red,1"], "grade slope must be finite and in [0, 65536]"),
    (["--grade-slope", "1,inf,1"], "grade slope must be finite and in [0, 65536]"),
    (["--grade-offset", "0,0,70000"], "grade offset must be finite and in [-65536, 65536]"),
    (["--grade-power", "0.1,1,1"], "grade power must be finite and in [1/8, 8]"),
    (["--grade-power", "1,1,9"], "grade power must be finite and in [1/8, 8]"),
    (["--grade-saturation", "4.5"], "grade saturation must be finite and in [0, 4]"),
    (["--grade-saturation", "vivid"], "grade saturation must be finite and in [0, 4]"),
    (["--white-balance", "1000"], "white balance temperature must be in [1667, 25000] kelvin"),
    (["--white-balance", "warm"], "white balance temperature must be in [1667, 25000] kelvin"),
    (["--white-balance", "1700"], "white balance temperature is outside sRGB"),
    (["--white-balance", "5000,1.5"], "white balance tint must be in [-1, 1]"),
    (["--white-balance", "5000,green"], "white balance tint must be in [-1, 1]"),
    (["--white-balance", "25000", "--grade-slope", "65536,1,1"], "grade slope must be finite and in [0, 65536]"),
    (["--white-balance", "3200", "--white-balance-at", "3,4"], "two white balances"),
    (["--white-balance-at", "5"], "--white-balance-at X,Y must be a pixel of the frame"),
    (["--white-balance-at", "-1,3"], "--white-balance-at X,Y must be a pixel of the frame"),
    (["-w", "64", "-h", "32", "--white-balance-at", "64,3"], "--white-balance-at X,Y must be a pixel of the frame"),
    (["--grade-region", "slope=2"], "--grade-region IDS:key=v[:key=v...] takes"),
    (["--grade-region", "1,x:slope=2"], "--grade-region IDS:key=v[:key=v...] takes"),
    (["--grade-region", ",".join(map(str, range(17))) + ":slope=2"], "--grade-region IDS:key=v[:key=v...] takes"),
    (["--grade-region", "1:gain=2"], "--grade-region IDS:key=v[:key=v...] takes"),
    (["--grade-region", "1:slope"], "--grade-region IDS:key=v[:key=v...] takes"),
    (["--grade-region", "1:slope=1,2"], "--grade-region IDS:key=v[:key=v...] takes"),
    (["--grade-region", "1:amount=1.5"], "grade region amount must be finite and in [0, 1]"),
    (["--grade-region", "1:power=16"], "grade power must be finite and in [1/8, 8]"),
    (["--grade-region", "1:saturation=-1"], "grade saturation must be finite and in [0, 4]"),
    (["--grade-region", "1"] * 5, "--grade-region can be given four times at the most"),
    (["--grade-region", "1:slope=2", "--gpus", "3"], "--grade-region needs the whole frame's mattes"),
    (["--grade-saturation", "0.5", "--three-arg"], "the grade options need the backend's options (without --three-arg)"),
])
def test_driver_refuses_bad_grade_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_grade_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--grade-slope R,G,B", "--grade-offset R,G,B", "--grade-power R,G,B", "--grade-saturation S", "--white-balance KELVIN[,TINT]",
                "--white-balance-at X,Y", "--grade-region IDS:key=v[:key=v...]", "grade_*"):
        assert opt in text, opt
    assert text.index("--grade-slope R,G,B") > text.index("--supersample K") > text.index("    -v  ")  # appended


# -- kajo_hip_grade_pixels against the restatements ---------------------------------------------------------------------------------

def _pixels(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    m = np.exp(rng.uniform(np.log(1e-6), np.log(3e3), (n, 3))).astype(F32)
    edge = F32([0.0, -0.0, 1e-45, 1e-40, 1.1754944e-38, 1.0, 65536.0, 3.0e38, -1.0, -1e-40, 0.18])
    m[:edge.size, 0] = edge
    m[edge.size:2 * edge.size, 2] = edge
    m[40] = [NAN, 1, 1]
    m[41] = [1, INF, 1]
    m[42] = [1, 1, -INF]
    masks = rng.integers(0, 65, (n, 4)).astype(F32) / F32(64)
    masks[::3, 1] = 0
    masks[::5] = 0
    masks[1::7] = 1
    return m, masks


REGION_OPS = [dict(slope=[2.0, 0.5, 0.0], saturation=0.0), dict(offset=[0.05, -0.02, 0.1], power=[2.2, 1.0, 0.125]),
              dict(slope=0.25, power=8.0, saturation=4.0), dict(slope=[1.5, 1.0, 0.75], offset=-0.01, saturation=1.7)]
SPECS = {
    "white_balance": dict(slope=[1.9, 1.0, 0.6]),
    "slope_0": dict(slope=[0.0, 1.0, 2.0], offset=[0.1, 0.0, -0.5]),
    "saturation_0": dict(saturation=0.0),
    "saturation_4": dict(slope=1.2, offset=[-0.05, 0.0, 0.02], saturation=4.0),
    "power_eighth": dict(power=0.125),
    "power_2.2": dict(slope=0.9, power=[2.2, 1.0, 2.2], saturation=0.6),
    "power_8": dict(power=8.0, offset=0.001),
    "one_region": dict(slope=[1.1, 1.0, 0.9], regions=[dict(objects=[1], amount=1.0, **REGION_OPS[0])]),
    "four_regions": dict(saturation=1.3, regions=[dict(objects=[k + 1], amount=a, **op) for k, (a, op) in
                                                  enumerate(zip((0.0, 0.5, 1.0, 0.5), REGION_OPS))]),
    "four_regions_no_power": dict(saturation=0.7, regions=[dict(objects=[k + 1], amount=a, **{k_: v for k_, v in op.items() if k_ != "power"})
                                                           for k, (a, op) in enumerate(zip((1.0, 0.5, 0.0, 1.0), REGION_OPS))]),
}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_grade_pixels_against_the_restatements(name):
    spec = SPECS[name]
    m, masks = _pixels()
    k = len(spec.get("regions", ()))
    mk = np.ascontiguousarray(masks[:, :k])
    got = grade_pixels(m, mk if k else None, **spec)
    want = restate64(spec, m, mk.astype(F64))
    c = want["counts"]
    assert c.sum() == len(m) - 3 and np.array_equal(bits(got[~c]), bits(m[~c]))
    c = want["ranged"]  # (the few values that leave float32's range on the way are restate32's to check)
    assert c.sum() >= 0.9 * len(m)
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(F64) - want["out64"])[c]
        ok = err <= want["allowance"][c]
        share = float(np.max(np.where(err > 0, err / want["allowance"][c], 0.0), initial=0.0))
    print("%s: largest share of the allowance %.4f" % (name, share))
    assert ok.all(), (name, share, m[c][~ok.all(-1)][:4], got[c][~ok.all(-1)][:4], want["out64"][c][~ok.all(-1)][:4])
    full = fill(spec)
    if all(p == 1.0 for op in [full] + full["regions"] for p in op["power"]):
        assert np.array_equal(bits(got), bits(restate32(spec, m, mk))), name
    # the same words for any number of pixels at a time, in place too
    one = np.concatenate([grade_pixels(m[i:i + 1], mk[i:i + 1] if k else None, **spec) for i in range(0, 60)])
    assert np.array_equal(bits(one), bits(got[:60]))


def test_identity_params_return_the_input_words():
    m, masks = _pixels()
    assert np.array_equal(bits(grade_pixels(m)), bits(m))
    assert np.array_equal(bits(grade_pixels(m, slope=1.0, offset=-0.0, power=1.0, saturation=1.0)), bits(m))
    # one region with the default op is not the identity case, yet changes nothing that is positive
    got = grade_pixels(m, masks[:, :1].copy(), regions=[dict(objects=[0])])
    pos = np.isfinite(m).all(-1) & (m >= 0).all(-1)
    assert np.array_equal(got[pos], m[pos])
    # a mask of 0 keeps c bit for bit through a region
    # (where the region's op stays finite: 0 * inf is a NaN under the rule as under any other)
    z = np.zeros((len(m), 2), F32)
    tame = ~(np.abs(m) > 1e4).any(-1)
    assert np.array_equal(bits(grade_pixels(m, z, saturation=0.5, regions=[dict(objects=[1], **REGION_OPS[1]), dict(objects=[2], **REGION_OPS[2])])[tame]),
                          bits(grade_pixels(m, saturation=0.5)[tame]))
    assert grade_pixels(np.zeros((0, 3), F32)).shape == (0, 3)


# -- white balance --------------------------------------------------------------------------------------------------------------------

def test_white_balance():
    x, y = planckian_xy(6500)
    assert abs(x - 0.3135) <= 1e-4 and abs(y - 0.3237) <= 1e-4, (x, y)
    lum = F64([0.2126, 0.7152, 0.0722])
    reds = []
    for T in (1950, 2222, 2223, 2800, 3200, 4000, 4001, 5000, 6500, 10000, 25000):
        g = grade_white_balance(T).astype(F64)
        lit = illuminant_rgb(T) * g
        assert np.abs(lit / lit.mean() - 1).max() <= 1e-6, (T, lit)
        assert abs(float(lum @ g) - 1) <= 1e-6, T
        reds.append(g[0])
    assert all(a < b for a, b in zip(reds, reds[1:])), reds  # the red gain rises with T
    # the tint: stops of green gain in front of the normalisation
    g0, g1 = grade_white_balance(5000).astype(F64), grade_white_balance(5000, 0.5).astype(F64)
    assert abs((g1[1] / g1[0]) / (g0[1] / g0[0]) - 2 ** 0.5) <= 1e-6 and abs(float(lum @ g1) - 1) <= 1e-6
    # the ends of the range: 25000 K is inside sRGB, 1667 K's blue is not
    assert np.isfinite(grade_white_balance(25000.0)).all()
    assert illuminant_rgb(1667)[2] <= 1e-3
    gains = (C.c_float * 3)()
    L = capi.lib()
    for T, tint, message in ((1667.0, 0.0, "white balance temperature is outside sRGB"), (1800.0, 0.0, "white balance temperature is outside sRGB"),
                             (1666.9, 0.0, "white balance temperature must be in [1667, 25000] kelvin"),
                             (25000.1, 0.0, "white balance temperature must be in [1667, 25000] kelvin"),
                             (NAN, 0.0, "white balance temperature must be in [1667, 25000] kelvin"),
                             (5000.0, 1.01, "white balance tint must be in [-1, 1]"), (5000.0, NAN, "white balance tint must be in [-1, 1]")):
        assert L.kajo_hip_grade_white_balance(T, tint, C.byref(gains)) == capi.KAJO_E_INVALID and _error() == message, (T, tint, _error())
    assert L.kajo_hip_grade_white_balance(5000.0, 0.0, None) == capi.KAJO_E_INVALID
    assert XYZ_TO_SRGB.shape == (3, 3)


def test_neutral():
    assert np.array_equal(grade_neutral([0.4, 0.4, 0.4]), F32([1, 1, 1]))
    px = F64([0.8, 0.3, 0.05])
    g = grade_neutral(px).astype(F64)
    lit = px * g
    assert np.abs(lit / lit.mean() - 1).max() <= 1e-6 and abs(float(F64([0.2126, 0.7152, 0.0722]) @ g) - 1) <= 1e-6
    L = capi.lib()
    gains = (C.c_float * 3)()
    for bad in ([0.0, 1, 1], [1, -1.0, 1], [1, 1, NAN], [INF, 1, 1]):
        src = (C.c_float * 3)(*bad)
        assert L.kajo_hip_grade_neutral(C.byref(src), C.byref(gains)) == capi.KAJO_E_INVALID
        assert _error() == "a neutral needs three finite positive channels"
    # the gains go into the slope in binary64, rounded once
    p = grade_params(slope=[0.7, 1.3, 1.1], white_balance=g.astype(F32))
    assert list(p.global_.slope) == [float(F32(a * float(b))) for a, b in zip((0.7, 1.3, 1.1), g.astype(F32))]


# -- the kernels' budgets -------------------------------------------------------------------------------------------------------------

# kernel -> (VGPRs at most, waves per SIMD): what the build produces. Neither uses LDS statically: the regions' bitsets are dynamic
# LDS, at most 4 x (nObjects + 1) bits
KERNELS = {"kajo_grade_global": (22, 8), "kajo_grade_regions": (42, 8)}


def test_grade_kernels_keep_their_budgets():
    b = devicecode.build("grade.hip")
    assert "-ffp-contract=off" in b.cmd and "--offload-arch=gfx950" in b.cmd
    res, text = b.resources, b.asm
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k, (vgprs, waves) in KERNELS.items():
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["AGPRs"] == 0, (k, r)
        assert r["VGPRs"] <= vgprs and r["Occupancy"] == waves and r["LDS Size"] == 0, (k, r)
    # no FLAT access, and what a pixel moves: one 16-byte load and one 16-byte store, plus the table's four loads with regions
    code = [l.split()[0] for l in text.splitlines() if l.startswith("\t") and not l.startswith("\t.")]
    assert code and not [op for op in code if op.startswith("flat_") or op.startswith("scratch_")]
    stores = [op for op in code if op.startswith("global_store") or op.startswith("buffer_store")]
    assert len(stores) >= 2 and set(stores) == {"global_store_dwordx4"}, stores  # every pixel leaves as one 16-byte store
    assert not [op for op in code if "atomic" in op]


# -- the arithmetic under the sanitizers ----------------------------------------------------------------------------------------------

def test_grade_math_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "grade_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tools", "grade_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert ": ok" in p.stdout
