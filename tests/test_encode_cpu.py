"""The encode (include/kajo_hip.h "The encode", kajo_amd/csrc/encode.cpp, encode_math.h, encode_host.h) without a GPU: the struct, the
constants and the entry points as the header declares them, in the product and the tools' twin; the defaults; every refusal in the
header's order on a NULL handle; the transfer tables against tests/encode_replay.py word for word, the accuracy sweep that chose E and
its failure at E / 2, the codes' monotony; kajo_hip_encode_pixels against the replay word for word on the edge inputs; the dither on a
slow ramp; the Makefile's plan, the kernel's budget from the compiler's remarks, the host code under the sanitizers; the driver's new
options and its 16-bit PNG writer."""
import ctypes as C
import os
import re
import shutil
import subprocess
import struct
import tempfile
import zlib

import numpy as np
import pytest

import devicecode
from kajo_amd import capi
from kajo_amd.renderer import encode_params, encode_pixels, encode_table
import encode_replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
ENTRY_POINTS = ("kajo_hip_default_encode_params", "kajo_hip_encode_bytes", "kajo_hip_encode_table", "kajo_hip_encode_pixels", "kajo_hip_encode",
                "kajo_hip_encode_present", "kajo_hip_encode_present_gathered_device")
F32, F64 = np.float32, np.float64
TABLED = (("gamma22", R.GAMMA22), ("srgb", R.SRGB), ("pq", R.PQ))
PEAKS = (1000.0, 203.0)


def _error():
    return (capi.lib().kajo_hip_last_error() or b"").decode()


def _tone(**kw):
    p = capi.KajoToneParams()
    capi.lib().kajo_hip_default_tone_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _encode(**kw):
    p = capi.KajoEncodeParams()
    capi.lib().kajo_hip_default_encode_params(C.byref(p))
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    return p


def _ref(p):
    return None if p is None else C.byref(p)


def test_header_struct_constants_binding_and_libraries_agree():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    assert C.sizeof(capi.KajoEncodeParams) == 32
    fields = re.search(r"typedef struct KajoEncodeParams \{(.*?)\} KajoEncodeParams;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f for f, _ in capi.KajoEncodeParams._fields_] == ["format", "transfer", "flags", "peakNits", "ditherSeed", "reserved"]
    for name, value in (("ENCODE_ARGB8", 0), ("ENCODE_RGB10A2", 1), ("ENCODE_RGBA16", 2), ("ENCODE_RGBA16F", 3), ("TRANSFER_GAMMA22", 0),
                        ("TRANSFER_SRGB", 1), ("TRANSFER_PQ", 2), ("TRANSFER_LINEAR", 3), ("ENCODE_DITHER", 1), ("ENCODE_SCENE", 2)):
        assert re.search(r"#define KAJO_%s %du\b" % (name, value), header) and getattr(capi, "KAJO_" + name) == value, name
    words = 2 * ((32 << R.LOG2E) + 1)
    assert re.search(r"#define KAJO_ENCODE_TABLE_WORDS %d\b" % words, header) and capi.KAJO_ENCODE_TABLE_WORDS == words == 8194
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        L = C.CDLL(lib)
        for name in ENTRY_POINTS:
            assert hasattr(L, name), (lib, name)
    assert b"encode" in capi.lib().kajo_hip_version().split(b";")[-1]
    assert "kajo_hip_encode_present" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "6q" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_defaults():
    p = capi.KajoEncodeParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    capi.lib().kajo_hip_default_encode_params(C.byref(p))
    assert (p.format, p.transfer, p.flags, p.peakNits, p.ditherSeed, list(p.reserved)) == (0, 0, 0, 1000.0, 0, [0, 0, 0])
    capi.lib().kajo_hip_default_encode_params(None)  # NULL is accepted


def _calls(encode, tone=None, meter=None, denoise=None):
    """the entry points that take the stage's parameters, with a NULL handle: -> [(name, rc, message)]"""
    L = capi.lib()
    tone = tone if tone is not None else _tone()
    out = []
    buf = (C.c_uint64 * 4)()
    rc = L.kajo_hip_encode(None, _ref(encode), C.byref(tone), buf)
    out.append(("encode", rc, _error()))
    rc = L.kajo_hip_encode_present(None, None, _ref(denoise), None, None, None, None, _ref(meter), C.byref(tone), _ref(encode), buf, None)
    out.append(("present", rc, _error()))
    rc = L.kajo_hip_encode_present_gathered_device(None, None, None, None, None, None, _ref(meter), C.byref(tone), _ref(encode), buf, None)
    out.append(("gathered", rc, _error()))
    return out


def _host_calls(encode, tone=None):
    """... and the two pure host ones, which go on where the others stop at the handle: -> [(name, rc, message)]"""
    L = capi.lib()
    tone = tone if tone is not None else _tone()
    mean = (C.c_float * 3)(0.25, 0.5, 0.75)
    buf = (C.c_uint64 * 1)()
    rc = L.kajo_hip_encode_pixels(_ref(encode), C.byref(tone), mean, 1, 0, 0, 1, buf)
    out = [("pixels", rc, _error() if rc else "")]
    size = C.c_size_t()
    rc = L.kajo_hip_encode_bytes(_ref(encode), 3, 2, C.byref(size))
    out.append(("bytes", rc, _error() if rc else ""))
    return out


HALF_LINEAR = "the half-float format stores linear values: its transfer must be linear"
PEAK_TEXT = "encode peak luminance must be finite and in (0, 10000] nits"
# in the header's order; each row is bad in its own field and in every field checked after it that can be bad beside it
BAD_FIELDS = [
    (dict(format=4, transfer=9, flags=4, reserved=0), "unknown encode format"),
    (dict(format=0xFFFFFFFF), "unknown encode format"),
    (dict(transfer=4, flags=0x80000000, reserved=1), "unknown encode transfer"),
    (dict(flags=4, reserved=2), "unknown encode flag"),
    (dict(flags=0x80000001), "unknown encode flag"),
    (dict(reserved=0, format=3, transfer=0), "encode reserved fields must be 0"),
    (dict(reserved=2), "encode reserved fields must be 0"),
    (dict(format=3, transfer=0, flags=1), HALF_LINEAR),
    (dict(format=3, transfer=2, peakNits=-1.0), HALF_LINEAR),
    (dict(format=0, transfer=3, flags=2), "scene-linear output needs the half-float format"),
    (dict(format=2, transfer=2, flags=3, peakNits=0.0), "scene-linear output needs the half-float format"),
    (dict(format=3, transfer=3, flags=1), "dither is for the integer formats"),
    (dict(format=3, transfer=3, flags=3), "dither is for the integer formats"),
    (dict(transfer=2, peakNits=0.0), PEAK_TEXT),
    (dict(transfer=2, peakNits=10000.5), PEAK_TEXT),
    (dict(transfer=2, peakNits=float("nan")), PEAK_TEXT),
    (dict(transfer=2, peakNits=float("inf")), PEAK_TEXT),
]


@pytest.mark.parametrize("fields,message", BAD_FIELDS, ids=["%s" % sorted(f.items()) for f, _ in BAD_FIELDS])
def test_every_refusal_comes_before_the_handle(fields, message):
    for name, rc, text in _calls(_encode(**fields)) + _host_calls(_encode(**fields)):
        assert rc == capi.KAJO_E_INVALID and text == message, (name, rc, text)


def test_null_parameters_the_tone_s_refusals_and_the_edges_of_the_ranges():
    L = capi.lib()
    for name, rc, text in _calls(None) + _host_calls(None):
        assert rc == capi.KAJO_E_INVALID and text == "null encode parameters", (name, text)
    # what is accepted reaches the handle, and the host calls succeed
    for fields in (dict(), dict(format=1, transfer=1, flags=1), dict(format=2, transfer=2, peakNits=10000.0), dict(transfer=2, peakNits=1e-3),
                   dict(format=3, transfer=3), dict(format=3, transfer=3, flags=2), dict(transfer=0, peakNits=-5.0),  # (peakNits: PQ only)
                   dict(format=2, transfer=3, flags=1, ditherSeed=0xFFFFFFFF)):
        for name, rc, text in _calls(_encode(**fields)):
            assert rc == capi.KAJO_E_INVALID and text == ("null argument" if name == "gathered" else "null handle"), (fields, name, text)
        for name, rc, text in _host_calls(_encode(**fields)):
            assert rc == 0, (fields, name, text)
    # the tone parameters come first, as they do in front of the view; the encode's; then the automatic exposure the stage cannot take
    bad_encode = _encode(format=9)
    for name, rc, text in _calls(bad_encode, tone=_tone(exposure=99.0)) + _host_calls(bad_encode, tone=_tone(exposure=99.0))[:1]:
        assert rc == capi.KAJO_E_INVALID and text == "tone exposure must be finite and in [-32, 32]", (name, text)
    auto = _tone(flags=capi.KAJO_TONE_AUTO_EXPOSURE)
    for name, rc, text in _calls(bad_encode, tone=auto) + _host_calls(bad_encode, tone=auto)[:1]:
        assert rc == capi.KAJO_E_INVALID and text == "unknown encode format", (name, text)
    for name, rc, text in _calls(_encode(), tone=auto) + _host_calls(_encode(), tone=auto)[:1]:
        assert rc == capi.KAJO_E_INVALID and "takes no automatic exposure" in text and "metered exposure" in text, (name, text)
        assert "KAJO_" not in text
    # ... before the denoiser's parameters, which come last in front of the handle
    denoise = capi.KajoDenoiseParams()
    L.kajo_hip_default_denoise_params(C.byref(denoise))
    denoise.iterations = 99
    assert _calls(bad_encode, denoise=denoise)[1][2] == "unknown encode format"
    assert _calls(_encode(), denoise=denoise)[1][2] == "denoise iterations must be in [0, 8]"
    # with a meter the two automatic exposures are the tone parameters' refusal: in front of the encode's
    meter = capi.KajoMeterParams()
    L.kajo_hip_default_meter_params(C.byref(meter))
    for name, rc, text in _calls(bad_encode, tone=auto, meter=meter)[1:]:
        assert rc == capi.KAJO_E_INVALID and "two automatic exposures" in text, (name, text)
    tone = _tone()
    assert L.kajo_hip_encode(None, C.byref(_encode()), None, None) == capi.KAJO_E_INVALID and _error() == "null tone parameters"
    # the host calls' own arguments
    size = C.c_size_t()
    assert L.kajo_hip_encode_bytes(C.byref(_encode()), 0, 4, C.byref(size)) == capi.KAJO_E_INVALID
    assert L.kajo_hip_encode_bytes(C.byref(_encode()), 4, 4, None) == capi.KAJO_E_INVALID
    for fmt, per in ((0, 4), (1, 4), (2, 8), (3, 8)):
        assert L.kajo_hip_encode_bytes(C.byref(_encode(format=fmt, transfer=3)), 7, 5, C.byref(size)) == 0 and size.value == 35 * per
    mean = (C.c_float * 3)()
    assert L.kajo_hip_encode_pixels(C.byref(_encode()), C.byref(tone), mean, 1, 0, 0, 0, mean) == capi.KAJO_E_INVALID
    assert L.kajo_hip_encode_pixels(C.byref(_encode()), C.byref(tone), None, 1, 0, 0, 1, mean) == capi.KAJO_E_INVALID
    assert L.kajo_hip_encode_pixels(C.byref(_encode()), C.byref(tone), None, 0, 0, 0, 1, None) == 0
    assert L.kajo_hip_encode_table(3, 1000.0, None, 0) == capi.KAJO_E_INVALID and _error() == "the linear transfer has no table"
    assert L.kajo_hip_encode_table(4, 1000.0, None, 0) == capi.KAJO_E_INVALID and _error() == "unknown encode transfer"
    assert L.kajo_hip_encode_table(2, 0.0, None, 0) == capi.KAJO_E_INVALID and _error() == PEAK_TEXT
    assert L.kajo_hip_encode_table(0, 0.0, None, 0) == capi.KAJO_ENCODE_TABLE_WORDS  # the size query; the peak is PQ's alone
    small = np.zeros(100, F32)
    assert L.kajo_hip_encode_table(0, 0.0, small.ctypes.data_as(C.c_void_p), small.size) == capi.KAJO_E_INVALID and _error() == "table array too small"


# -- the table -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,transfer", TABLED)
def test_table_is_the_replay_s_word_for_word(name, transfer):
    for peak in PEAKS:
        got = encode_table(name, peak)
        assert got.shape == (4097, 2)
        assert np.array_equal(got.reshape(-1).view(np.uint32), R.table(transfer, peak).view(np.uint32)), (name, peak)
    t = encode_table(name, 1000.0)
    assert np.all(np.diff(t[:, 0].astype(F64)) >= 0) and np.all(t[:-1, 1] > 0) and 0 < t[0, 0] < t[-1, 0] <= 1.0


def test_the_sweep_meets_a_quarter_code_at_e_and_not_at_half_of_it():
    """every 61st float32 in [2^-32, 1], every knot and its two neighbours: |v(y) - T64(y)| * 65535 stays below a quarter of a 16-bit
    code at E = 128 for the three tabulated transfers, and does not at E = 64: the cap binds (DESIGN.md section 6q has the figures)"""
    worst = {}
    for log2e in (R.LOG2E, R.LOG2E - 1):
        worst[log2e] = [R.sweep(log2e, transfer, peak)[0] for _, transfer in TABLED for peak in (PEAKS if transfer == R.PQ else PEAKS[:1])]
        print("E = %d: largest deviations in 16-bit codes %s" % (1 << log2e, ["%.4f" % w for w in worst[log2e]]))
    assert max(worst[R.LOG2E]) < 0.25
    assert max(worst[R.LOG2E - 1]) > 0.25 and min(worst[R.LOG2E - 1][:2]) > 0.25  # (GAMMA22 and SRGB each miss it at E / 2)


@pytest.mark.parametrize("name,transfer", TABLED + (("linear", R.LINEAR),))
def test_codes_do_not_decrease_in_y(name, transfer):
    """over the sweep's y, through the library's own kajo_hip_encode_pixels, for every format"""
    _, y, _ = R.sweep(R.LOG2E, R.GAMMA22, 1000.0, stride=257)
    y = np.concatenate([F32([0.0, 1e-45, 1e-30]), y, F32([1.0000001, 2.0, 1e9])])
    mean = np.repeat(y[:, None], 3, 1)
    for fmt, shifts, mask in (("argb8", (16, 8, 0), 255), ("rgb10a2", (20, 10, 0), 1023), ("rgba16", (0, 16, 32), 65535)):
        w = encode_pixels(mean, dict(format=fmt, transfer=name, peak_nits=1000.0)).astype(np.uint64)
        top = mask if transfer != R.PQ else int(np.floor(F32(R.table(R.PQ, 1000.0)[-2] * F32(mask)) + F32(0.5)))  # (PQ: 1000 of 10000 nits)
        for s in shifts:
            c = ((w >> np.uint64(s)) & np.uint64(mask)).astype(np.int64)
            assert np.all(np.diff(c) >= 0) and c[0] == 0 and c[-1] == top, (fmt, name)
    if transfer == R.LINEAR:
        w = encode_pixels(mean, dict(format="rgba16f"))
        c = (w & np.uint64(0xFFFF)).astype(np.int64)
        assert np.all(np.diff(c) >= 0) and c[0] == 0 and c[-1] == 0x3C00


# -- the host twin against the replay ------------------------------------------------------------------------------------------------

CURVES = [(R.CLAMP, "clamp", 0.0, 0.0), (R.REINHARD, "reinhard", 1.5, 0.0), (R.REINHARD, "reinhard", -2.25, 4.0), (R.ACES, "aces", 0.5, 0.0)]


def test_encode_pixels_is_the_replay_word_for_word_on_the_edge_inputs():
    mean = np.concatenate([R.edge_means(), R.binade_ramp()])
    assert np.isnan(mean).any() and np.isinf(mean).any() and (mean == 0).any() and (np.abs(mean[np.isfinite(mean) & (mean != 0)]) < 1e-38).any()
    n = 0
    for fmt in (R.ARGB8, R.RGB10A2, R.RGBA16, R.RGBA16F):
        for transfer in (R.GAMMA22, R.SRGB, R.PQ, R.LINEAR):
            for flags in (0, R.DITHER, R.SCENE):
                e = capi.KajoEncodeParams(fmt, transfer, flags, 600.0, 77)
                if capi.lib().kajo_hip_encode_bytes(C.byref(e), 1, 1, C.byref(C.c_size_t())) != 0:
                    continue  # (a refused combination)
                for cid, curve, exposure, white in CURVES:
                    got = encode_pixels(mean, e, x0=5, y0=9, row_width=37, curve=curve, exposure=exposure, white=white)
                    want = R.encode_pixels(fmt, transfer, flags, 600.0, 77, cid, exposure, white, mean, 5, 9, 37)
                    assert got.dtype == want.dtype and np.array_equal(got, want), (fmt, transfer, flags, curve, np.nonzero(got != want)[0][:4])
                    n += 1
    assert n == (3 * 4 * 2 + 2) * len(CURVES)


def test_the_half_rounding_is_ieee_round_to_nearest_even():
    """the integer conversion against numpy's own float32 -> float16 over every value the stage can hand it that matters: all halves,
    the midpoints between neighbours, and their float32 neighbours"""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(F64)
    mid = 0.5 * (h[:-1] + h[1:])
    v = np.concatenate([h, mid]).astype(F32)
    v = np.unique(np.concatenate([v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))]))
    v = v[(v >= 0) & (v <= 65504)]
    want = v.astype(np.float16).view(np.uint16)
    assert np.array_equal(R.half_bits(v).astype(np.uint16), want)
    got = encode_pixels(np.repeat(v[:, None], 3, 1), dict(format="rgba16f", scene=True))
    for shift in (0, 16, 32):
        assert np.array_equal(((got >> np.uint64(shift)) & np.uint64(0xFFFF)).astype(np.uint16), want)
    assert ((got >> np.uint64(48)) == 0x3C00).all()


# -- the dither ----------------------------------------------------------------------------------------------------------------------

def _ramp():
    """4096 pixels of one row rising by two 8-bit codes, 100 to 102: the window means of v * 255 then lie 1/64 of a code from a whole
    code at the nearest, the farthest from one that windows of 64 pixels on such a ramp can all be"""
    k = np.arange(4096, dtype=F64)
    y = ((100.0 + 2.0 * k / 4096.0) / 255.0).astype(F32)
    return np.repeat(y[:, None], 3, 1), y.astype(F64) * 255.0


def _channels(w):
    return np.stack([(w >> s) & 255 for s in (16, 8, 0)], 1).astype(F64)


def test_dither_brings_every_window_mean_closer():
    mean, exact = _ramp()
    target = exact.reshape(64, 64).mean(1)
    plain = _channels(encode_pixels(mean, dict(format="argb8", transfer="linear")))
    dithered = _channels(encode_pixels(mean, dict(format="argb8", transfer="linear", dither=True), x0=0, y0=0, row_width=4096))
    assert set(np.unique(plain)) == {100.0, 101.0, 102.0} and np.abs(dithered - exact[:, None]).max() < 1.0
    for ch in range(3):
        err_plain = np.abs(plain[:, ch].reshape(64, 64).mean(1) - target)
        err_dithered = np.abs(dithered[:, ch].reshape(64, 64).mean(1) - target)
        print("channel %d: largest window error plain %.4f, dithered %.4f; windows not closer: %s" %
              (ch, err_plain.max(), err_dithered.max(), np.nonzero(err_dithered >= err_plain)[0].tolist()))
        assert np.all(err_dithered < err_plain), ch


def test_dither_is_a_function_of_the_seed_and_the_frame_coordinates():
    mean, _ = _ramp()
    e = dict(format="rgb10a2", transfer="srgb", dither=True, dither_seed=7)
    a = encode_pixels(mean, e, x0=3, y0=5, row_width=128)
    assert np.array_equal(a, encode_pixels(mean, e, x0=3, y0=5, row_width=128))
    assert not np.array_equal(a, encode_pixels(mean, dict(e, dither_seed=8), x0=3, y0=5, row_width=128))
    assert not np.array_equal(a, encode_pixels(mean, e, x0=4, y0=5, row_width=128))
    # a pixel's word depends on where it is, not on how the rectangle around it is cut: rows 6 and 7 of the same block
    assert np.array_equal(a[128:384], encode_pixels(mean[128:384], e, x0=3, y0=6, row_width=128))
    assert np.array_equal(R.hash32(np.arange(5), 3, 1, 7), [int(R.hash32(x, 3, 1, 7)) for x in range(5)])


# -- the build -----------------------------------------------------------------------------------------------------------------------

def test_makefile_compiles_the_stage_once_and_links_it_twice():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("encode.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "/encode.cpp" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0] and "gfx950" in compiles[0] and "-x hip" in compiles[0], compiles
    assert "encode.cpp" in open(os.path.join(CSRC, "Makefile")).read().split("HIPCC")[0]  # the header comment
    text = open(os.path.join(CSRC, "encode.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["encode_math.h", "render_args.h"]
    assert not re.search(r"\b(powf?|expf?|exp2f?|logf?|log2f?|__ocml\w*|__builtin_\w*(pow|exp|log)\w*)\s*\(", text + open(os.path.join(CSRC, "encode_math.h")).read())


def test_the_kernel_keeps_its_budget():
    """no scratch, no spill, and the LDS the source's comment states: the table, 8194 floats"""
    b = devicecode.build("encode.cpp")
    res, body = b.resources, b.asm
    assert sorted(res) == ["kajo_encode"], sorted(res)
    k = res["kajo_encode"]
    print(k)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["ScratchSize"] == 0 and k["AGPRs"] == 0, k
    assert k["LDS Size"] == 4 * capi.KAJO_ENCODE_TABLE_WORDS == 32776 and k["Occupancy"] >= 4, k
    assert "32776" in open(os.path.join(CSRC, "encode.cpp")).read().split("#include")[0]
    # the table is read from LDS and the pixel written by one store; no atomics, nothing through FLAT
    ops = set(re.findall(r"^\s+((?:ds|global|flat|scratch|buffer)_\w+)", body, re.M))
    assert ops <= {"ds_read_b32", "ds_read_b64", "ds_read2_b32", "ds_write_b64", "global_load_dwordx2", "global_load_dwordx3", "global_load_dwordx4",
                   "global_store_dword", "global_store_dwordx2"}, ops
    assert {"global_store_dword", "global_store_dwordx2"} <= ops


def test_host_code_under_the_sanitizers(tmp_path):
    """tools/encode_san.cpp: the table and the definition over the edge inputs, compiled with -fsanitize=address,undefined, on the CPU"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "encode_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tools", "encode_san.cpp"), "-o", exe]
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
    mean = np.stack([np.repeat(vals, len(vals)), np.full(len(vals) ** 2, 0.25, F32), np.tile(vals, len(vals))], 1)
    total = 0
    for fmt in range(4):
        for transfer in range(4):
            for flags in range(4):
                e = capi.KajoEncodeParams(fmt, transfer, flags, 1000.0, 12345)
                if capi.lib().kajo_hip_encode_bytes(C.byref(e), 1, 1, C.byref(C.c_size_t())) != 0:
                    continue
                for curve, exposure, white in (("clamp", 0.0, 0.0), ("reinhard", 2.0, 4.0), ("aces", -1.0, 0.0)):
                    for w in encode_pixels(mean, e, x0=7, y0=3, row_width=5, curve=curve, exposure=exposure, white=white):
                        total = (total * 1099511628211 + int(w)) & 0xFFFFFFFFFFFFFFFF
    assert m and int(m.group(1), 16) == total


# -- the driver ----------------------------------------------------------------------------------------------------------------------

BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
HOST_LIB = os.path.join(ROOT, "kajo_amd", "libkajo_host.so")
PEAK_OPTION = "--peak-nits: encode peak luminance must be finite and in (0, 10000] nits"


def read_png16(path):
    """a 16-bit RGB PNG by a few lines of zlib: -> ((H, W, 3) uint16 samples, {chunk type: data} of the other chunks)"""
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks, idat = 8, {}, b""
    while at < len(blob):
        n, kind = struct.unpack(">I4s", blob[at:at + 8])
        data = blob[at + 8:at + 8 + n]
        assert struct.unpack(">I", blob[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data), kind
        if kind == b"IDAT":
            idat += data
        else:
            chunks[kind] = data
        at += 12 + n
    W, H, depth, colour, compression, flt, interlace = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
    assert (depth, colour, compression, flt, interlace) == (16, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 6 * W)
    assert (raw[:, 0] == 0).all()  # filter type none on every scanline
    return np.ascontiguousarray(raw[:, 1:]).view(">u2").astype(np.uint16).reshape(H, W, 3), chunks


@pytest.mark.parametrize("pq", [False, True], ids=["plain", "pq"])
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (300, 91)], ids=lambda s: "%dx%d" % s)
def test_the_png_writer_s_16_bit_output_gives_back_the_samples(tmp_path, shape, pq):
    """Image.cpp writePng16 through libkajo_host.so: every sample comes back, high byte first in the file; the alpha word is not written;
    the cICP chunk (1, 16, 0, 1) is there for a PQ signal, in front of the image data, and only then (300x91: more than one stored block)"""
    assert os.path.exists(HOST_LIB), HOST_LIB
    L = C.CDLL(HOST_LIB)
    W, H = shape
    rgba = np.random.default_rng(W * H).integers(0, 65536, (H, W, 4), dtype=np.uint16)
    rgba.reshape(-1, 4)[:4, :3] = [[0, 0xFFFF, 0x0102], [0xFF00, 0x00FF, 0x8000], [1, 256, 257], [0xABCD, 0x1234, 0xFFFE]][:min(4, W * H)]
    path = str(tmp_path / "o.png")
    assert L.kajo_host_write_png16(path.encode(), W, H, rgba.ctypes.data_as(C.c_void_p), int(pq)) == 0
    got, chunks = read_png16(path)
    assert np.array_equal(got, rgba[..., :3])
    assert (chunks.get(b"cICP") == bytes([1, 16, 0, 1])) if pq else (b"cICP" not in chunks)
    blob = open(path, "rb").read()
    assert not pq or blob.index(b"IHDR") < blob.index(b"cICP") < blob.index(b"IDAT")
    assert L.kajo_host_write_png16(str(tmp_path / "none" / "o.png").encode(), W, H, rgba.ctypes.data_as(C.c_void_p), 0) != 0


@pytest.mark.parametrize("args,message", [
    (["--transfer", "pq"], "--transfer and --peak-nits belong to --png16"),
    (["--peak-nits", "500"], "--transfer and --peak-nits belong to --png16"),
    (["--png16", "p.png", "--transfer", "linear"], "--transfer must be gamma22, srgb or pq"),
    (["--png16", "p.png", "--transfer", "PQ"], "--transfer must be gamma22, srgb or pq"),
    (["--png16", "p.png", "--peak-nits", "500"], "--peak-nits belongs to --transfer pq"),
    (["--png16", "p.png", "--transfer", "srgb", "--peak-nits", "500"], "--peak-nits belongs to --transfer pq"),
    (["--png16", "p.png", "--transfer", "pq", "--peak-nits", "0"], PEAK_OPTION),
    (["--png16", "p.png", "--transfer", "pq", "--peak-nits", "10000.5"], PEAK_OPTION),
    (["--png16", "p.png", "--transfer", "pq", "--peak-nits", "nan"], PEAK_OPTION),
    (["--png16", "p.png", "--transfer", "pq", "--peak-nits", "bright"], PEAK_OPTION),
    (["--dither-seed", "3"], "--dither-seed belongs to --dither"),
    (["--dither", "--dither-seed", "-1"], "--dither-seed N must be in 0..4294967295"),
    (["--dither", "--dither-seed", "4294967296"], "--dither-seed N must be in 0..4294967295"),
    (["--dither", "--dither-seed", "7x"], "--dither-seed N must be in 0..4294967295"),
    (["--dither", "--output-size", "80x45"], "--dither and a view option are not combined"),
    (["--dither", "--supersample", "2"], "--dither and a view option are not combined"),
    (["--dither", "--auto-exposure"], "take no --auto-exposure"),
    (["--png16", "p.png", "--auto-exposure"], "use --meter-exposure"),
    (["--png16", "p.png", "--three-arg"], "the encode options need the options constructor (without --three-arg)"),
    (["--dither", "--three-arg"], "the encode options need the options constructor (without --three-arg)"),
])
def test_driver_refuses_bad_encode_options_before_opening_a_device(tmp_path, args, message):
    assert os.path.exists(BIN), BIN
    p = subprocess.run([BIN, *args, "-o", str(tmp_path / "o.png")], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


def test_driver_parses_good_encode_options_and_lists_them():
    """accepted options get as far as the device: without one the driver ends with the backend's refusal (2), with one with a frame (0);
    never with a refusal of the options (1)"""
    assert os.path.exists(BIN), BIN
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--png16 FILE.png", "--transfer gamma22|srgb|pq", "--peak-nits N", "--dither ", "--dither-seed N", "encode_format", "encode_transfer",
                "encode_peak_nits", "encode_dither", "cICP"):
        assert opt in text, opt
    assert text.index("--png16 FILE.png") > text.index("--noise-map FILE")  # appended
    with tempfile.TemporaryDirectory() as d:
        for args in (["--png16", "p.png"], ["--png16", "p.png", "--transfer", "srgb"], ["--png16", "p.png", "--transfer", "pq", "--peak-nits", "10000"],
                     ["--dither"], ["--dither", "--dither-seed", "4294967295", "--png16", "p.png", "--meter-exposure", "0.5"]):
            p = subprocess.run([BIN, "-w", "32", "-h", "16", "--passes", "1", "--no-preview", *args, "-o", "o.png"], capture_output=True, text=True,
                               timeout=120, cwd=d)
            assert p.returncode in (0, 2), (args, p.returncode, p.stderr)
