"""The view (include/kajo_hip.h "The view", kajo_amd/csrc/view.hip) without a GPU: the struct, the constants and the entry points as the
header declares them, in the product and the tools' twin; the defaults; every refusal that needs no handle, and their order across the
stages (despeckle, lens, glare, local, meter, tone, view, denoise, handle; the view's checks against the frame need the handle and so
cannot be reached here: tests/test_hip_view.py holds them); the weight rows against a float64 restatement; the transfer tables; the
float32 restatement of the whole stage (tests/view_replay.py) on constant images and the checkerboard; the motivating number from the
oracle's frames; the Makefile's plan and the kernels' budgets from the compiler's remarks."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import devicecode
from kajo_amd import capi
from kajo_amd.renderer import view_tables, view_weights
import view_replay
from view_replay import FILTERS, restate, tables64, weights64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
ENTRY_POINTS = ("kajo_hip_default_view_params", "kajo_hip_view_weights", "kajo_hip_view_tables", "kajo_hip_view_argb8",
                "kajo_hip_present_view_argb8", "kajo_hip_present_view_gathered_argb8_device")
F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")


def _params(cls, default, **kw):
    p = cls()
    getattr(capi.lib(), default)(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _view(**kw):
    kw = dict(dict(outW=8, outH=8), **kw)
    return _params(capi.KajoViewParams, "kajo_hip_default_view_params", **kw)


def _tone(**kw):
    return _params(capi.KajoToneParams, "kajo_hip_default_tone_params", **kw)


def _ref(p):
    return None if p is None else C.byref(p)


def _error():
    return (capi.lib().kajo_hip_last_error() or b"").decode()


def test_header_struct_constants_binding_and_libraries_agree():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    assert C.sizeof(capi.KajoViewParams) == 32
    fields = re.search(r"typedef struct KajoViewParams \{(.*?)\} KajoViewParams;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f for f, _ in capi.KajoViewParams._fields_] == ["x0", "y0", "x1", "y1", "outW", "outH", "filter", "flags"]
    for name, value in (("MAX_SCALE", 64), ("MAX_TAPS", 384), ("MAX_OUT", 16384)):
        assert re.search(r"#define KAJO_VIEW_%s %d\b" % (name, value), header) and getattr(capi, "KAJO_VIEW_" + name) == value
    assert capi.KAJO_VIEW_MAX_TAPS == 2 * 3 * capi.KAJO_VIEW_MAX_SCALE  # LANCZOS3's support, stretched by the largest scale
    assert "KAJO_VIEW_NEAREST = 0, KAJO_VIEW_AREA = 1, KAJO_VIEW_TRIANGLE = 2, KAJO_VIEW_LANCZOS3 = 3" in header
    assert capi.KAJO_VIEW_FILTERS == dict(nearest=0, area=1, triangle=2, lanczos3=3)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        L = C.CDLL(lib)
        for name in ENTRY_POINTS:
            assert hasattr(L, name), (lib, name)
    assert b"view" in capi.lib().kajo_hip_version().split(b";")[-1]
    assert "kajo_hip_present_view_argb8" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_defaults():
    p = capi.KajoViewParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    capi.lib().kajo_hip_default_view_params(C.byref(p))
    assert (p.x0, p.y0, p.x1, p.y1) == (0.0, 0.0, 0.0, 0.0) and (p.outW, p.outH) == (0, 0)
    assert p.filter == capi.KAJO_VIEW_AREA and p.flags == 0
    capi.lib().kajo_hip_default_view_params(None)  # NULL is accepted


def _calls(view, despeckle=None, denoise=None, lens=None, glare=None, local=None, meter=None, tone=None):
    """the entry points that take the stage's parameters, with a NULL handle: -> [(name, rc, message)]"""
    L = capi.lib()
    tone = tone if tone is not None else _tone()
    out = []
    word = C.c_uint32()
    rc = L.kajo_hip_view_argb8(None, _ref(view), C.byref(word), C.byref(word))
    out.append(("view", rc, _error()))
    rc = L.kajo_hip_present_view_argb8(None, _ref(despeckle), _ref(denoise), _ref(lens), _ref(glare), _ref(local), _ref(meter), C.byref(tone),
                                       _ref(view), None, None)
    out.append(("present", rc, _error()))
    rc = L.kajo_hip_present_view_gathered_argb8_device(None, None, _ref(despeckle), _ref(glare), _ref(local), _ref(meter), C.byref(tone),
                                                       _ref(view), None, None)
    out.append(("gathered", rc, _error()))
    return out


RECT = "view rectangle must satisfy 0 <= x0 < x1 and 0 <= y0 < y1"
BAD_FIELDS = [
    (dict(x0=NAN, x1=4.0, y1=4.0), "view rectangle edges must be finite"),
    (dict(x1=INF, y1=4.0), "view rectangle edges must be finite"),
    (dict(y0=-INF, x1=4.0, y1=4.0), "view rectangle edges must be finite"),
    (dict(y1=NAN), "view rectangle edges must be finite"),
    (dict(x0=-0.5, x1=4.0, y1=4.0), RECT),
    (dict(x0=4.0, x1=4.0, y1=4.0), RECT),
    (dict(x0=5.0, x1=4.0, y1=4.0), RECT),
    (dict(x1=4.0, y0=-1.0, y1=4.0), RECT),
    (dict(x1=4.0, y0=4.0, y1=4.0), RECT),
    (dict(x1=4.0), RECT),  # (only three edges zero: not the whole frame)
    (dict(outW=0), "view output size must be in [1, 16384]"),
    (dict(outH=0), "view output size must be in [1, 16384]"),
    (dict(outW=-8), "view output size must be in [1, 16384]"),
    (dict(outH=16385), "view output size must be in [1, 16384]"),
    (dict(x1=513.0, y1=4.0, outW=8), "view minification must be at most 64"),
    (dict(x1=4.0, y1=64.5, outH=1), "view minification must be at most 64"),
    (dict(filter=4), "unknown view filter"),
    (dict(filter=0xFFFFFFFF), "unknown view filter"),
    (dict(flags=1), "unknown view flag"),
    (dict(flags=0x80000000), "unknown view flag"),
]


@pytest.mark.parametrize("fields,message", BAD_FIELDS, ids=["%s" % sorted(f.items()) for f, _ in BAD_FIELDS])
def test_every_refusal_comes_before_the_handle(fields, message):
    for name, rc, text in _calls(_view(**fields)):
        assert rc == capi.KAJO_E_INVALID and text == message, (name, rc, text)


def test_ff_filled_and_null_parameters_are_refused_and_the_edges_of_the_ranges_are_not():
    p = capi.KajoViewParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    for name, rc, text in _calls(p):
        assert rc == capi.KAJO_E_INVALID and text == "view rectangle edges must be finite", (name, text)  # (0xFFFFFFFF is a NaN)
    L = capi.lib()
    word = C.c_uint32()
    assert L.kajo_hip_view_argb8(None, None, C.byref(word), C.byref(word)) == capi.KAJO_E_INVALID and _error() == "null view parameters"
    for fields in (dict(outW=1, outH=1), dict(outW=16384, outH=16384), dict(x1=512.0, y1=64.0, outW=8, outH=1), dict(filter=0), dict(filter=3),
                   dict(x0=0.25, y0=0.5, x1=0.75, y1=1.0)):
        for name, rc, text in _calls(_view(**fields)):
            assert rc == capi.KAJO_E_INVALID and text == "null handle", (fields, name, text)
    # view == NULL in the chain entries is the call in front of them: its refusals, not this stage's
    assert L.kajo_hip_present_view_argb8(None, None, None, None, None, None, None, C.byref(_tone()), None, None, None) == capi.KAJO_E_INVALID
    assert _error() == "null handle"
    assert L.kajo_hip_present_view_gathered_argb8_device(None, None, None, None, None, None, C.byref(_tone(exposure=99.0)), None, None,
                                                         None) == capi.KAJO_E_INVALID
    assert _error() == "tone exposure must be finite and in [-32, 32]"


def test_the_order_of_refusals_across_the_stages():
    """despeckle, lens, glare, local, meter, tone, view, denoise, handle: each stage's bad parameters are reported while everything after
    it is bad too. (The view's checks against W and H come behind the null handle: a NULL handle cannot reach them.)"""
    P = lambda cls, name, **kw: _params(cls, "kajo_hip_default_%s_params" % name, **kw)
    bad = dict(despeckle=P(capi.KajoDespeckleParams, "despeckle", rank=9), lens=P(capi.KajoLensParams, "lens", maxRadius=99),
               glare=P(capi.KajoGlareParams, "glare", levels=99), local=P(capi.KajoLocalParams, "local", detail=9.0),
               meter=P(capi.KajoMeterParams, "meter", key=-1.0), tone=_tone(exposure=99.0), view=_view(filter=9),
               denoise=P(capi.KajoDenoiseParams, "denoise", iterations=99))
    good = dict(despeckle=P(capi.KajoDespeckleParams, "despeckle"), lens=P(capi.KajoLensParams, "lens"), glare=P(capi.KajoGlareParams, "glare"),
                local=P(capi.KajoLocalParams, "local"), meter=P(capi.KajoMeterParams, "meter"), tone=_tone(), view=_view(),
                denoise=P(capi.KajoDenoiseParams, "denoise"))
    messages = dict(despeckle="despeckle rank must be in [1, 4]", lens="lens max radius must be in [1, 16]",
                    glare="glare levels must be in [0, 12]", local="local detail must be finite and in [0, 4]",
                    meter="meter key must be finite and positive", tone="tone exposure must be finite and in [-32, 32]",
                    view="unknown view filter", denoise="denoise iterations must be in [0, 8]")
    order = ["despeckle", "lens", "glare", "local", "meter", "tone", "view", "denoise"]
    takes = dict(view=("view",), present=order, gathered=("despeckle", "glare", "local", "meter", "tone", "view"))
    for i, first in enumerate(order):
        args = {k: (good[k] if order.index(k) < i else bad[k]) for k in order}
        for name, rc, text in _calls(**args):
            assert rc == capi.KAJO_E_INVALID, (first, name)
            want = next((messages[k] for k in order[i:] if k in takes[name]), None)
            assert text == (want or "null handle"), (first, name, text)
    for name, rc, text in _calls(**good):
        assert rc == capi.KAJO_E_INVALID and text == "null handle", (name, text)
    # the two automatic exposures are refused with the tone parameters: before the view's
    name, rc, text = _calls(view=bad["view"], meter=good["meter"], tone=_tone(flags=capi.KAJO_TONE_AUTO_EXPOSURE))[1]
    assert rc == capi.KAJO_E_INVALID and "two automatic exposures" in text, (name, text)


# -- the weight rows -----------------------------------------------------------------------------------------------------------------

SRC_N = (1, 2, 7, 41, 65, 130, 4096)


def _axis_cases():
    for n in SRC_N:
        outs = {1, n, 2 * n + 1, math.ceil(n / 8.5), math.ceil(n / 64)}  # (srcN / 64 rounded up: the largest scale an outN gives)
        if n // 2 >= 1:
            outs.add(n // 2)
        rects = [(0.0, float(n))]
        if n >= 2:
            rects.append((0.25, n - 0.5))
        rects.append((n * 0.5 - 0.375, n * 0.5 + 0.25) if n > 1 else (0.125, 0.75))  # (inside one or two pixels)
        for a0, a1 in rects:
            for out_n in sorted(outs):
                if (a1 - a0) / out_n <= 64:
                    yield n, a0, a1, out_n


AXIS_CASES = list(_axis_cases())


def _ulp(x):
    return np.spacing(np.abs(F32(x)))


@pytest.mark.parametrize("filter", FILTERS)
def test_weights_against_the_float64_restatement(filter):
    """first and count identical; every weight within 1 float32 ulp of the restatement's -- not 0: sin and the division may differ in the
    last binary64 place between the C library and numpy, which can move a value across a float32 rounding boundary; every row sums to 1
    within count * 2^-24 (the binary64 quotients sum to 1 and each float32 rounding moves a weight by at most half an ulp of a value
    that is at most about 1: 2^-24 at the most, negative lobes included); no row reaches outside the axis."""
    for n, a0, a1, out_n in AXIS_CASES:
        first, count, w = view_weights(n, a0, a1, out_n, filter)
        want = weights64(n, a0, a1, out_n, filter)
        assert w.shape == (out_n, count.max()) and count.min() >= 1 and count.max() <= capi.KAJO_VIEW_MAX_TAPS
        assert first.min() >= 0 and (first + count).max() <= n, (n, a0, a1, out_n)
        assert [int(f) for f in first] == [f for f, _ in want], (n, a0, a1, out_n)
        assert [int(c) for c in count] == [len(r) for _, r in want], (n, a0, a1, out_n)
        for i, (_, row) in enumerate(want):
            got = w[i, :count[i]]
            ref = np.array(row, F64)
            assert np.all(np.abs(got.astype(F64) - ref) <= _ulp(ref)), (n, a0, a1, out_n, i)
            assert not w[i, count[i]:].any()
            assert abs(got.astype(F64).sum() - 1.0) <= count[i] * 2.0 ** -24, (n, a0, a1, out_n, i)
            if filter == "nearest":
                assert count[i] == 1 and got[0] == 1.0


def test_weights_exact_cases():
    for n in SRC_N:
        for filter in FILTERS:  # the identity: one weight 1.0 at first == i
            first, count, w = view_weights(n, 0.0, float(n), n, filter)
            assert np.array_equal(first, np.arange(n)) and (count == 1).all() and (w == 1.0).all() and w.shape == (n, 1), (n, filter)
        for K in (2, 3, 4, 8, 64):  # AREA at an integer ratio: K weights of exactly float32(1 / K)
            if n % K == 0:
                first, count, w = view_weights(n, 0.0, float(n), n // K, "area")
                assert np.array_equal(first, np.arange(n // K) * K) and (count == K).all() and (w == F32(1.0 / K)).all(), (n, K)
    first, count, w = view_weights(4096, 0.0, 4096.0, 64, "lanczos3")  # the longest rows there are
    assert count.max() == capi.KAJO_VIEW_MAX_TAPS == 384
    first, count, w = view_weights(4096, 0.0, 4096.0, 8193, "area")  # magnifying: at most two pixels
    assert count.max() == 2


def test_weights_size_query_and_refusals():
    L = capi.lib()
    assert L.kajo_hip_view_weights(130, 0.0, 130.0, 16, capi.KAJO_VIEW_LANCZOS3, None, None, None, 0) == 16 * view_weights(130, 0, 130, 16, "lanczos3")[2].shape[1]
    first, count = np.zeros(16, np.int32), np.zeros(16, np.int32)
    w = np.zeros(4, F32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.kajo_hip_view_weights(130, 0.0, 130.0, 16, 3, p(first), p(count), p(w), 4) == capi.KAJO_E_INVALID
    assert _error() == "weights array too small"
    assert L.kajo_hip_view_weights(130, 0.0, 130.0, 16, 3, p(first), None, None, 0) == capi.KAJO_E_INVALID and _error() == "null argument"
    for args in ((0, 0.0, 1.0, 1, 1), (8, 0.0, 8.0, 0, 1), (8, 0.0, 8.0, 16385, 1), (8, -1.0, 8.0, 4, 1), (8, 0.0, 8.5, 4, 1), (8, 4.0, 4.0, 4, 1),
                 (8, NAN, 8.0, 4, 1), (130, 0.0, 130.0, 2, 1), (8, 0.0, 8.0, 4, 4)):
        assert L.kajo_hip_view_weights(*args, None, None, None, 0) == capi.KAJO_E_INVALID and _error() == "invalid view axis", args


# -- the transfer tables -------------------------------------------------------------------------------------------------------------

def test_tables():
    lin, thr = view_tables()
    lin64, thr64 = tables64()
    # (pow may differ in the last binary64 place between the C library and numpy: 1 float32 ulp, as for the weights)
    assert np.all(np.abs(lin.astype(F64) - lin64) <= _ulp(lin64)) and np.all(np.abs(thr.astype(F64) - thr64) <= _ulp(thr64))
    assert lin[0] == 0.0 and lin[255] == 1.0
    merged = np.empty(511, F32)
    merged[0::2], merged[1::2] = lin, thr  # lin[0] < t[1] < lin[1] < ... < t[255] < lin[255]
    assert np.all(np.diff(merged.astype(F64)) > 0)
    # far from both neighbours in units of float rounding: the room that keeps a constant image constant under weights that sum to 1
    # within count * 2^-24 (count <= 384: 2.3e-5 relative)
    gap = np.minimum(lin[1:] - thr, np.append(thr[1:], np.inf) - lin[1:]).astype(F64)
    assert np.all(gap / lin[1:] > 1e-3), (gap / lin[1:]).min()
    assert np.array_equal(np.searchsorted(thr, lin, side="right"), np.arange(256))  # encode(lin[c]) == c
    assert [int(float(v) ** (1 / 2.2) * 255 + .5) for v in lin] == list(range(256))  # ... and so is the chain's own quantiser
    capi.lib().kajo_hip_view_tables(None, None)


# -- the restatement of the whole stage ----------------------------------------------------------------------------------------------

def _word(c):
    return np.uint32(0xFF000000 | c << 16 | c << 8 | c)


@pytest.mark.parametrize("filter", FILTERS)
def test_a_constant_image_comes_back_constant(filter):
    """every code, every filter, the ratios of the axis list (one image holds all 256 codes as 256 constant bands is NOT the same thing:
    each code gets an image of its own, of one row, viewed along x; the vertical pass of a one-row image is one weight of 1.0)"""
    lin, thr = view_tables()
    codes = np.arange(256)
    for n, a0, a1, out_n in AXIS_CASES:
        first, count, w = view_weights(n, a0, a1, out_n, filter)
        acc = np.zeros((256, out_n), F32)
        for k in range(w.shape[1]):
            acc = np.where(k < count, acc + w[:, k] * lin[:, None], acc)
        assert np.array_equal(np.searchsorted(thr, acc, side="right"), np.broadcast_to(codes[:, None], acc.shape)), (n, a0, a1, out_n)
    for c in (0, 1, 127, 254, 255):  # ... and through restate() itself, both passes
        img = np.full((23, 41), _word(c), np.uint32)
        for ow, oh in ((1, 1), (20, 11), (83, 47), (5, 3), (41, 23)):
            assert (restate(img, ow, oh, None, filter) == _word(c)).all(), (c, ow, oh)
        assert (restate(img, 41, 23, (0.25, 0.5, 40.5, 22.25), filter) == _word(c)).all()


def test_checkerboard_two_to_one_is_one_code():
    """each output pixel averages two black and two white ones: 0.5 (lin[255] + lin[0]) = 0.5 exactly at both passes, and
    encode(0.5) = int(255 * 0.5 ** (1 / 2.2) + .5) = 186"""
    lin, thr = view_tables()
    code = int(np.searchsorted(thr, F32(0.5), side="right"))
    assert code == 186 == int(255 * 0.5 ** (1 / 2.2) + .5)
    img = view_replay.test_images(40, 22)["checker"]
    assert (restate(img, 20, 11) == _word(186)).all()


def test_the_copy_case_is_the_identity_under_the_definition():
    img = view_replay.test_images(41, 23)["random"]
    for filter in FILTERS:
        assert np.array_equal(restate(img, 41, 23, None, filter), img)


# -- the motivating number -----------------------------------------------------------------------------------------------------------

def test_supersampling_and_the_lights_edges(scenes):
    """spheres.json 16:9 at 160x90, clamp curve, exposure 0, 128 samples per pixel, from the oracle's frames (its own quantiser is the
    clamp curve at exposure 0) and the restatement of the view. Measured: the boundary holds 500 pixels; those of them whose largest
    channel code lies in 16..239: plain 385, --supersample 2 463, --supersample 4 459. Most of the boundary by this definition is the
    dark side's neighbours, which are intermediate in the plain render already, so the count starts high; the supersampled views move
    the rest. The direction is asserted, as the figures show it with room to spare (a fifth more, two thirds of what was left to
    gain); no ratio is."""
    from oraclelib import OracleLib, available
    if not available("oracle"):
        pytest.skip("oracle library not built")
    O = OracleLib("oracle")

    def frame(K):
        accum = O.create(scenes["spheres_a169"], 0).render(160 * K, 90 * K, S=128, passes=1)
        return O.resolve(accum, 1).reshape(90 * K, 160 * K) | np.uint32(0xFF000000)

    largest = lambda p: np.maximum(np.maximum((p >> 16) & 255, (p >> 8) & 255), p & 255).astype(int)
    plain = frame(1)
    pad = np.pad(largest(plain), 1, mode="edge")
    nb = np.stack([pad[dy:dy + 90, dx:dx + 160] for dy in range(3) for dx in range(3)])
    boundary = (nb == 255).any(0) & (nb < 128).any(0)
    counts = {}
    for K in (1, 2, 4):
        m = largest(plain if K == 1 else restate(frame(K), 160, 90))
        counts[K] = int(((m >= 16) & (m <= 239) & boundary).sum())
    print("boundary %d pixels; intermediate codes: plain %d, x2 %d, x4 %d" % (boundary.sum(), counts[1], counts[2], counts[4]))
    assert boundary.sum() > 0
    assert counts[2] >= counts[1] and counts[4] >= counts[1]


# -- the driver ----------------------------------------------------------------------------------------------------------------------

BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
RECT_TEXT = "view rectangle must satisfy 0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height"


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--output-size", "0x45"], "view output size must be in [1, 16384]"),
    (["--output-size", "80x16385"], "view output size must be in [1, 16384]"),
    (["--output-size", "80"], "view output size must be in [1, 16384]"),
    (["--output-size", "80x45x2"], "view output size must be in [1, 16384]"),
    (["--output-size", "wide"], "view output size must be in [1, 16384]"),
    (["-w", "640", "-h", "480", "--output-size", "9x480"], "view minification must be at most 64"),
    (["-w", "640", "-h", "480", "--output-size", "640x7"], "view minification must be at most 64"),
    (["--view", "0,0,10"], RECT_TEXT),
    (["--view", "0,0,10,10,10"], RECT_TEXT),
    (["--view", "5,0,5,10"], RECT_TEXT),
    (["--view", "-1,0,5,10"], RECT_TEXT),
    (["--view", "0,0,nan,10"], RECT_TEXT),
    (["-w", "64", "-h", "32", "--view", "0,0,64.5,32"], RECT_TEXT),
    (["-w", "64", "-h", "32", "--view", "0,0,64,33"], RECT_TEXT),
    (["--view-filter", "cubic"], "--view-filter must be nearest, area, triangle or lanczos3"),
    (["--supersample", "1"], "--supersample K must be in 2..8"),
    (["--supersample", "9"], "--supersample K must be in 2..8"),
    (["--supersample", "2x"], "--supersample K must be in 2..8"),
    (["--supersample", "2", "--output-size", "80x45"], "--supersample and --output-size are two output sizes: give one"),
    (["--supersample", "2", "--view-filter", "lanczos3"], "--view-filter must be area with it"),
    (["--output-size", "80x45", "--three-arg"], "the view options need the options constructor (without --three-arg)"),
])
def test_driver_refuses_bad_view_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_view_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--output-size WxH", "--view X0,Y0,X1,Y1", "--view-filter nearest|area|triangle|lanczos3", "--supersample K", "view_out_w",
                "view_scale_y", "stay at the rendered size"):
        assert opt in text, opt
    assert text.index("--output-size WxH") > text.index("--lens-max-radius R")  # appended


# -- the build -----------------------------------------------------------------------------------------------------------------------

def test_makefile_compiles_the_stage_once_and_links_it_twice():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("view.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "view.hip" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0] and "gfx950" in compiles[0], compiles
    assert "view.hip" in open(os.path.join(CSRC, "Makefile")).read().split("HIPCC")[0]  # the header comment


# kernel -> (VGPRs, waves per SIMD, LDS bytes per workgroup): what the build produces, held exactly. rows: lin[256] + sw[16][64] floats;
# columns: the thresholds, 255 + one pad
KERNELS = {"kajo_view_rows": (35, 8, 5120), "kajo_view_columns": (11, 8, 1024)}


def test_view_kernels_keep_their_budgets():
    b = devicecode.build("view.hip")
    assert "-ffp-contract=off" in b.cmd and "--offload-arch=gfx950" in b.cmd
    res = b.resources
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k, (vgprs, waves, lds) in KERNELS.items():
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["AGPRs"] == 0, (k, r)
        assert r["VGPRs"] == vgprs and r["Occupancy"] == waves and r["LDS Size"] == lds, (k, r)
