"""The float view (include/kajo_hip.h "The float view", kajo_amd/csrc/encode_view.cpp, encode_view_host.h) without a GPU: the entry
points as the header declares them, in the product and the tools' twin; kajo_hip_encode_view_pixels against tests/encode_view_replay.py
word for word; the copy case, NEAREST's gather, Lanczos's overshoot; every refusal and their order on a NULL handle; the Makefile's
plan, the kernels' budgets from the compiler's remarks, the host code under the sanitizers; the driver's new option."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import devicecode
from kajo_amd import capi
from kajo_amd.renderer import encode_params, encode_pixels, encode_view_pixels, view_params
import encode_view_replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
ENTRY_POINTS = ("kajo_hip_encode_view", "kajo_hip_encode_view_present", "kajo_hip_encode_view_present_gathered_device", "kajo_hip_encode_view_pixels")
F32 = np.float32
FILTERS = ("nearest", "area", "triangle", "lanczos3")


def _error():
    return (capi.lib().kajo_hip_last_error() or b"").decode()


def _ref(p):
    return None if p is None else C.byref(p)


def _tone(**kw):
    p = capi.KajoToneParams()
    capi.lib().kajo_hip_default_tone_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _view(**kw):
    p = capi.KajoViewParams()
    capi.lib().kajo_hip_default_view_params(C.byref(p))
    p.outW, p.outH = 4, 3
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_header_binding_and_libraries_agree():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        L = C.CDLL(lib)
        for name in ENTRY_POINTS + ("kajo_encode_view_launch", "kajo_encode_view_chunk"):
            assert hasattr(L, name), (lib, name)
    assert b"encode-view" in capi.lib().kajo_hip_version().split(b";")[-1]
    assert "The float view" in header and header.index("The float view") > header.index("/* The encode:")
    assert "6s" in open(os.path.join(ROOT, "DESIGN.md")).read() and "--encode-view" in open(os.path.join(ROOT, "README.md")).read()
    # the ARGB8 chain's names and their recorded refusals are what they were
    assert not [n for n in ENTRY_POINTS if n.startswith("kajo_hip_present_")]


# -- the host twin against the replay ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (41, 23), (130, 70)], ids=lambda s: "%dx%d" % s)
def test_encode_view_pixels_is_the_replay_word_for_word(shape):
    """means over many binades with NaN, +-Inf, negatives, -0 and values above 65504 among them, a bright pixel on an edge and a constant;
    the covering set of (format, transfer, flags); the four filters; the four output sizes"""
    W, H = shape
    frames = R.frames(W, H)
    assert np.isnan(frames["wild"]).any() or W * H < 8
    n = 0
    for config, cfg in R.CONFIGS.items():
        e, tone = R.encode_kwargs(cfg)
        for filt in FILTERS:
            for size, (out_w, out_h, rect) in R.out_sizes(W, H).items():
                for name in ("wild", "bright_edge", "const_2"):
                    got = encode_view_pixels(frames[name], e, dict(out_w=out_w, out_h=out_h, rect=rect, filter=filt), **tone)
                    want = R.restate(cfg, frames[name], out_w, out_h, rect, filt)
                    assert got.dtype == want.dtype and got.shape == (out_h, out_w)
                    assert np.array_equal(got, want), (config, filt, size, name, np.argwhere(got != want)[:4])
                    n += 1
    assert n == 6 * 4 * 4 * 3


@pytest.mark.parametrize("shape", [(4096, 1), (1, 4096)], ids=lambda s: "%dx%d" % s)
def test_the_largest_rows(shape):
    """4096 -> 64: scale 64, LANCZOS3's rows have the view's 384 taps"""
    W, H = shape
    out_w, out_h = (64, 1) if H == 1 else (1, 64)
    mean = R.frames(W, H)["wild"]
    for config in ("rgba16_pq600_dither", "rgba16f_scene", "argb8_gamma22_dither"):
        e, tone = R.encode_kwargs(R.CONFIGS[config])
        for filt in FILTERS:
            got = encode_view_pixels(mean, e, dict(out_w=out_w, out_h=out_h, filter=filt), **tone)
            assert np.array_equal(got, R.restate(R.CONFIGS[config], mean, out_w, out_h, None, filt)), (config, filt)


def test_the_copy_case_a_null_view_and_nearest_without_dither():
    W, H = 41, 23
    mean = R.frames(W, H)["wild"]
    for config, cfg in R.CONFIGS.items():
        e, tone = R.encode_kwargs(cfg)
        plain = encode_pixels(mean, e, row_width=W, **tone).reshape(H, W)
        assert np.array_equal(plain, R.plain(cfg, mean))
        assert np.array_equal(encode_view_pixels(mean, e, None, **tone), plain)
        for filt in FILTERS:
            # what the library returns (the plain encode) and what the definition gives (the identity) are one image
            for rect in (None, (0.0, 0.0, float(W), float(H))):
                assert np.array_equal(encode_view_pixels(mean, e, dict(rect=rect, filter=filt), **tone), plain), (config, filt)
            assert np.array_equal(R.restate(cfg, mean, W, H, None, filt), plain), (config, filt)
        if not e["dither"]:
            for out_w, out_h, rect in ((21, 12, None), (83, 47, None), (30, 11, (2.5, 1.25, 39.0, 20.5))):
                x0, y0, x1, y1 = rect or (0.0, 0.0, float(W), float(H))
                fx = np.floor(x0 + (np.arange(out_w) + 0.5) * ((x1 - x0) / out_w)).astype(int)
                fy = np.floor(y0 + (np.arange(out_h) + 0.5) * ((y1 - y0) / out_h)).astype(int)
                got = encode_view_pixels(mean, e, dict(out_w=out_w, out_h=out_h, rect=rect, filter="nearest"), **tone)
                assert np.array_equal(got, plain[fy][:, fx]), (config, out_w, out_h)


def test_a_lanczos_overshoot_next_to_a_step_stays_in_range():
    """a 0 / 1 step: r undershoots 0 and overshoots 1 beside it; q is clamped, the codes lie in [0, M] and reach both ends"""
    W, H = 48, 6
    mean = np.zeros((H, W, 3), F32)
    mean[:, W // 2:] = 1.0
    r = R.resample(R.front(R.CONFIGS["rgba16_linear"][:5] + (0, 0.0, 0.0), mean), 2 * W + 1, H, None, "lanczos3")
    assert r.min() < 0 and r.max() > 1  # (the case shows something)
    for fmt, top in (("argb8", 255), ("rgb10a2", 1023), ("rgba16", 65535)):
        for transfer in ("gamma22", "srgb", "linear"):
            for dither in (False, True):
                e = dict(format=fmt, transfer=transfer, dither=dither, dither_seed=5)
                cfg = (capi.KAJO_ENCODE_FORMATS[fmt], capi.KAJO_TRANSFERS[transfer], int(dither), 1000.0, 5, 0, 0.0, 0.0)
                got = encode_view_pixels(mean, e, dict(out_w=2 * W + 1, out_h=H, filter="lanczos3"))
                assert np.array_equal(got, R.restate(cfg, mean, 2 * W + 1, H, None, "lanczos3"))
                c = R.channels(cfg, got)
                assert c.min() == 0 and c.max() == top, (fmt, transfer, dither)
    half = encode_view_pixels(mean, dict(format="rgba16f"), dict(out_w=2 * W + 1, out_h=H, filter="lanczos3"))
    c = R.channels(R.CONFIGS["rgba16f"], half)
    assert c.min() == 0 and c.max() == 0x3C00
    scene = encode_view_pixels(mean * F32(70000.0), dict(format="rgba16f", scene=True), dict(out_w=2 * W + 1, out_h=H, filter="lanczos3"))
    assert R.channels(R.CONFIGS["rgba16f_scene"], scene).max() == 0x7BFF  # 65504


# -- the refusals --------------------------------------------------------------------------------------------------------------------

def _calls(encode, tone, view, meter=None, denoise=None, despeckle=None):
    """the entry points with a NULL handle, and the host twin over a 4 x 3 frame: -> [(name, rc, message)]"""
    L = capi.lib()
    buf = (C.c_uint64 * 64)()
    mean = (C.c_float * 36)()
    out = []
    rc = L.kajo_hip_encode_view(None, _ref(encode), _ref(tone), _ref(view), buf)
    out.append(("stage", rc, _error()))
    rc = L.kajo_hip_encode_view_present(None, _ref(despeckle), _ref(denoise), None, None, None, None, _ref(meter), _ref(tone), _ref(view), _ref(encode), buf,
                                        None)
    out.append(("present", rc, _error()))
    rc = L.kajo_hip_encode_view_present_gathered_device(None, None, _ref(despeckle), None, None, None, _ref(meter), _ref(tone), _ref(view), _ref(encode),
                                                        buf, None)
    out.append(("gathered", rc, _error()))
    rc = L.kajo_hip_encode_view_pixels(_ref(encode), _ref(tone), _ref(view), mean, 4, 3, buf)
    out.append(("pixels", rc, _error() if rc else ""))
    return out


def test_every_refusal_and_their_order():
    L = capi.lib()
    good_e, good_t, good_v = encode_params(), _tone(), _view()
    bad_t, bad_v, bad_e = _tone(exposure=99.0), _view(filter=9), encode_params(format=9)
    auto = _tone(flags=capi.KAJO_TONE_AUTO_EXPOSURE)
    TONE, VIEW, ENCODE = "tone exposure must be finite and in [-32, 32]", "unknown view filter", "unknown encode format"
    # what is accepted reaches the handle; the host twin succeeds
    for name, rc, text in _calls(good_e, good_t, good_v):
        if name == "pixels":
            assert rc == 0
        else:
            assert rc == capi.KAJO_E_INVALID and text == ("null argument" if name == "gathered" else "null handle"), (name, text)
    # tone, then view, then encode, then the automatic exposure the encode cannot take
    for name, rc, text in _calls(bad_e, bad_t, bad_v):
        assert rc == capi.KAJO_E_INVALID and text == TONE, (name, text)
    for name, rc, text in _calls(bad_e, good_t, bad_v) + _calls(bad_e, auto, bad_v):
        assert rc == capi.KAJO_E_INVALID and text == VIEW, (name, text)
    for name, rc, text in _calls(bad_e, good_t, good_v) + _calls(bad_e, auto, good_v):
        assert rc == capi.KAJO_E_INVALID and text == ENCODE, (name, text)
    for name, rc, text in _calls(good_e, auto, good_v):
        assert rc == capi.KAJO_E_INVALID and "takes no automatic exposure" in text, (name, text)
    for name, rc, text in _calls(None, good_t, good_v):
        assert rc == capi.KAJO_E_INVALID and text == "null encode parameters", (name, text)
    for name, rc, text in _calls(good_e, None, bad_v):
        assert rc == capi.KAJO_E_INVALID and text == "null tone parameters", (name, text)
    # every refusal of the view's own parameters, as the 8-bit view words them
    for fields, text in ((dict(x0=float("nan")), "view rectangle edges must be finite"),
                         (dict(x0=2.0, x1=1.0, y1=1.0), "view rectangle must satisfy 0 <= x0 < x1 and 0 <= y0 < y1"),
                         (dict(outW=0), "view output size must be in [1, 16384]"), (dict(outH=16385), "view output size must be in [1, 16384]"),
                         (dict(x1=130.0, y1=1.0, outW=2), "view minification must be at most 64"), (dict(filter=4), VIEW), (dict(flags=1), "unknown view flag")):
        for name, rc, got in _calls(good_e, good_t, _view(**fields)):
            assert rc == capi.KAJO_E_INVALID and got == text, (fields, name, got)
    # the stages in front come first, the denoiser's parameters behind the encode's, the two automatic exposures with the tone's
    despeckle = capi.KajoDespeckleParams()
    L.kajo_hip_default_despeckle_params(C.byref(despeckle))
    despeckle.rank = 9
    for name, rc, text in _calls(bad_e, bad_t, bad_v, despeckle=despeckle)[1:3]:
        assert text == "despeckle rank must be in [1, 4]", (name, text)
    denoise = capi.KajoDenoiseParams()
    L.kajo_hip_default_denoise_params(C.byref(denoise))
    denoise.iterations = 99
    assert _calls(bad_e, good_t, good_v, denoise=denoise)[1][2] == ENCODE
    assert _calls(good_e, auto, good_v, denoise=denoise)[1][2].startswith("the encode takes no automatic exposure")
    assert _calls(good_e, good_t, good_v, denoise=denoise)[1][2] == "denoise iterations must be in [0, 8]"
    meter = capi.KajoMeterParams()
    L.kajo_hip_default_meter_params(C.byref(meter))
    for name, rc, text in _calls(bad_e, auto, bad_v, meter=meter)[1:3]:
        assert rc == capi.KAJO_E_INVALID and "two automatic exposures" in text, (name, text)
    # a NULL view: the encoded entry points' own answers
    for name, rc, text in _calls(bad_e, good_t, None):
        assert rc == capi.KAJO_E_INVALID and text == ENCODE, (name, text)
    for name, rc, text in _calls(good_e, good_t, None)[:3]:
        assert text == ("null argument" if name == "gathered" else "null handle"), (name, text)
    # the host twin's own arguments, then the view against the frame: last
    mean, buf = (C.c_float * 36)(), (C.c_uint64 * 64)()
    outside = _view(x1=5.0, y1=3.0)
    call = lambda v, m, w, h, o: L.kajo_hip_encode_view_pixels(C.byref(good_e), C.byref(good_t), _ref(v), m, w, h, o)
    assert call(outside, mean, 0, 3, buf) == capi.KAJO_E_INVALID and _error() == "width and height must be at least 1"
    assert call(outside, None, 4, 3, buf) == capi.KAJO_E_INVALID and _error() == "null argument"
    assert call(outside, mean, 4, 3, None) == capi.KAJO_E_INVALID and _error() == "null argument"
    assert call(outside, mean, 4, 3, buf) == capi.KAJO_E_INVALID and _error() == "view rectangle must lie inside the frame"
    assert call(_view(outW=1, outH=1), (C.c_float * (130 * 3))(), 130, 1, buf) == capi.KAJO_E_INVALID and _error() == "view minification must be at most 64"
    assert call(_view(x1=4.0, y1=3.0), mean, 4, 3, buf) == 0
    with pytest.raises(ValueError):
        encode_view_pixels(np.zeros((5, 3), F32))
    assert view_params(7, 5).outW == 7 and view_params(7, 5, filter="lanczos3").filter == capi.KAJO_VIEW_LANCZOS3


# -- the build -----------------------------------------------------------------------------------------------------------------------

def test_makefile_compiles_the_unit_once_and_links_it_twice():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("encode_view.o" in l and "encode.o" in l and "view.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "/encode_view.cpp" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0] and "gfx950" in compiles[0] and "-x hip" in compiles[0], compiles
    encode = next(l for l in plan.splitlines() if l.startswith("hipcc") and "/encode.cpp" in l)
    assert compiles[0].replace("encode_view", "encode") == encode  # compiled as encode.cpp is: the same division, the same contraction
    assert "encode_view.cpp" in open(os.path.join(CSRC, "Makefile")).read().split("HIPCC")[0]  # the header comment
    text = open(os.path.join(CSRC, "encode_view.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["encode_math.h", "render_args.h"]
    assert not re.search(r"\b(powf?|expf?|exp2f?|logf?|log2f?|fmaf?|__fmaf_\w+|__ocml\w*|__builtin_\w*(pow|exp|log|fma)\w*)\s*\(", text)
    assert "atomic" not in re.sub(r"//.*", "", text)
    host = open(os.path.join(CSRC, "encode_view_host.h")).read()
    assert re.findall(r'#include "([^"]+)"', host) == ["encode_host.h", "view_weights.h"] and "hip" not in re.sub(r"//.*", "", host).lower()


def test_the_kernels_keep_their_budgets():
    """no scratch, no spill; the LDS the source's comment states: rows 3 planes x 4 rows x 256 floats + 64 (first, end) pairs = 12800 bytes,
    columns the table, 32776 bytes; the registers and the occupancy of this build (gfx950, -O3), pinned as tests/test_view_cpu.py pins
    the view's"""
    b = devicecode.build("encode_view.cpp")
    res, body = b.resources, b.asm
    assert sorted(res) == ["kajo_encode_view_columns", "kajo_encode_view_rows"], sorted(res)
    print(res)
    for k in res.values():
        assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["ScratchSize"] == 0 and k["AGPRs"] == 0, k
    rows, columns = res["kajo_encode_view_rows"], res["kajo_encode_view_columns"]
    chunk = C.CDLL(capi.LIB_PATH).kajo_encode_view_chunk()
    assert chunk == 256 and rows["LDS Size"] == 3 * 4 * chunk * 4 + 2 * 64 * 4 == 12800
    assert columns["LDS Size"] == 4 * capi.KAJO_ENCODE_TABLE_WORDS == 32776
    assert (rows["VGPRs"], rows["Occupancy"]) == (78, 6) and (columns["VGPRs"], columns["Occupancy"]) == (20, 4), res
    head = open(os.path.join(CSRC, "encode_view.cpp")).read().split("#include")[0]
    assert "12800" in head and "32776" in head
    # the planes and the table are read from LDS, a pixel is written by one store; no atomics, nothing through FLAT or scratch
    ops = set(re.findall(r"^\s+((?:ds|global|flat|scratch|buffer)_\w+)", body, re.M))
    assert not [o for o in ops if o.startswith(("flat_", "scratch_", "buffer_")) or "atomic" in o or "_add" in o], ops
    assert {"global_store_dword", "global_store_dwordx2", "global_store_dwordx4"} == {o for o in ops if o.startswith("global_store")}, ops


def test_host_code_under_the_sanitizers(tmp_path):
    """tools/encode_view_san.cpp: the definition over the edge inputs and the largest tap rows, compiled with -fsanitize=address,undefined,
    on the CPU, as tests/test_encode_cpu.py runs tools/encode_san.cpp"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "encode_view_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tools", "encode_view_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and ": ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    # its checksum is the library's over the same inputs: the same lines, two compilers
    m = re.search(r"checksum ([0-9a-f]{16})", p.stdout)
    vals = np.array([0.0, -0.0, 1e-45, 1e-40, 1.17549435e-38, 2.0 ** -33, 2.0 ** -32, 1e-6, 0.18, 0.5, 0.99999994, 1.0, 1.0000001, 3.5, 65504.0, 65520.0,
                     1e30, 3.4e38, -1.0, -1e-40, -3.4e38, np.nan, np.inf, -np.inf], F32)
    N = len(vals)
    mean = np.stack([np.repeat(vals, N), np.full(N * N, 0.25, F32), np.tile(vals, N)], 1).reshape(N, N, 3)
    i = np.arange(4096)
    line = np.stack([vals[i % N], np.full(4096, 0.25, F32), vals[(i // N) % N]], 1)
    total = 0
    for fmt in range(4):
        for transfer in range(4):
            for flags in range(4):
                e = capi.KajoEncodeParams(fmt, transfer, flags, 1000.0, 12345)
                if capi.lib().kajo_hip_encode_bytes(C.byref(e), 1, 1, C.byref(C.c_size_t())) != 0:
                    continue
                for curve, exposure, white in (("clamp", 0.0, 0.0), ("reinhard", 2.0, 4.0), ("aces", -1.0, 0.0)):
                    tone = dict(curve=curve, exposure=exposure, white=white)
                    images = []
                    for filt in range(4):
                        images.append(encode_view_pixels(mean, e, dict(rect=(0.25, 0.5, N - 0.25, N - 0.5), filter=filt), **tone))
                        images.append(encode_view_pixels(mean, e, dict(out_w=5, out_h=7, filter=filt), **tone))
                        images.append(encode_view_pixels(mean, e, dict(out_w=2 * N + 1, out_h=2 * N + 1, filter=filt), **tone))
                    images.append(encode_view_pixels(line.reshape(1, 4096, 3), e, dict(out_w=64, out_h=1, filter="lanczos3"), **tone))
                    images.append(encode_view_pixels(line.reshape(4096, 1, 3), e, dict(out_w=1, out_h=64, filter="lanczos3"), **tone))
                    for image in images:
                        for w in image.reshape(-1).tolist():
                            total = (total * 1099511628211 + w) & 0xFFFFFFFFFFFFFFFF
    assert m and int(m.group(1), 16) == total


# -- the driver ----------------------------------------------------------------------------------------------------------------------

BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")


@pytest.mark.parametrize("args,message", [
    (["--encode-view"], "--encode-view needs a view option"),
    (["--encode-view", "--png16", "p.png"], "--encode-view needs a view option"),
    (["--encode-view", "--dither"], "--encode-view needs a view option"),
    (["--encode-view", "--supersample", "2"], "--encode-view needs --png16 or --dither"),
    (["--encode-view", "--output-size", "80x45", "--view-filter", "lanczos3"], "--encode-view needs --png16 or --dither"),
    (["--encode-view", "--supersample", "2", "--dither", "--three-arg"], "the encode options need the options constructor (without --three-arg)"),
    (["--encode-view", "--supersample", "2", "--png16", "p.png", "--auto-exposure"], "use --meter-exposure"),
    (["--encode-view", "--supersample", "9", "--png16", "p.png"], "--supersample K must be in 2..8"),
    # without the switch the driver refuses what it refused
    (["--dither", "--supersample", "2"], "--dither and a view option are not combined"),
])
def test_driver_refuses_before_opening_a_device(tmp_path, args, message):
    assert os.path.exists(BIN), BIN
    p = subprocess.run([BIN, *args, "-o", str(tmp_path / "o.png")], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


def test_driver_parses_the_option_and_lists_it_last():
    """accepted command lines get as far as the device: without one the driver ends with the backend's refusal (2), with one with a frame
    (0); never with a refusal of the options (1)"""
    assert os.path.exists(BIN), BIN
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for word in ("--encode-view ", "encode_view_out_w", "encode_view_out_h", "The float view"):
        assert word in text, word
    assert text.index("--encode-view ") > text.index("--dither-seed N")  # appended behind the old ones
    with tempfile.TemporaryDirectory() as d:
        for args in (["--supersample", "2", "--png16", "p.png", "--encode-view"], ["--output-size", "16x8", "--dither", "--encode-view"],
                     ["--view", "1,1,20,12", "--view-filter", "lanczos3", "--dither", "--dither-seed", "3", "--png16", "p.png", "--encode-view"]):
            p = subprocess.run([BIN, "-w", "32", "-h", "16", "--passes", "1", "--no-preview", *args, "-o", "o.png"], capture_output=True, text=True,
                               timeout=120, cwd=d)
            assert p.returncode in (0, 2), (args, p.returncode, p.stderr)
