"""Exposure, tone curves and automatic exposure (include/kajo_hip.h kajo_hip_tonemap_argb8, kajo_amd/csrc/tonemap.inc.hip) without a GPU:
the constants, the struct and the entry points as the header declares them, the documented defaults, every refusal that comes before a
device is looked at, what the compiler made of the kernels (nothing spilled, no scratch, no FLAT instruction, no atomic, no scalar store),
and the driver's refusals of bad option values. The compile command is the Makefile's own (`make -n`)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from kajo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
ENTRY_POINTS = ("kajo_hip_default_tone_params", "kajo_hip_tonemap_argb8", "kajo_hip_tonemap_gathered_argb8_device", "kajo_hip_tone_scale")
KERNELS = ("kajo_tone_logavg_tiles", "kajo_tone_logavg_frame", "kajo_tone_scale", "kajo_tone_map_tiles", "kajo_tone_map_frame")


def _header():
    return open(os.path.join(ROOT, "include", "kajo_hip.h")).read()


def test_header_constants_struct_and_binding_agree():
    header = _header()
    for name, value in (("KAJO_TONE_CLAMP", capi.KAJO_TONE_CLAMP), ("KAJO_TONE_REINHARD", capi.KAJO_TONE_REINHARD),
                        ("KAJO_TONE_ACES", capi.KAJO_TONE_ACES)):
        m = re.search(r"#define %s (\d+)\b" % name, header)
        assert m and int(m.group(1)) == value, name
    assert (capi.KAJO_TONE_CLAMP, capi.KAJO_TONE_REINHARD, capi.KAJO_TONE_ACES) == (0, 1, 2)
    m = re.search(r"#define KAJO_TONE_AUTO_EXPOSURE (\d+)u", header)
    assert m and int(m.group(1)) == capi.KAJO_TONE_AUTO_EXPOSURE == 1
    assert C.sizeof(capi.KajoToneParams) == 32
    fields = re.search(r"typedef struct KajoToneParams \{(.*?)\} KajoToneParams;", header, re.S).group(1)
    names = re.findall(r"^\s+\w+ (\w+)(?:\[\d+\])?;", fields, re.M)
    assert names == [f for f, _ in capi.KajoToneParams._fields_]
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(r"\bT %s\b" % name, nm), name


def test_default_params_are_the_documented_ones():
    L = capi.lib()
    p = capi.KajoToneParams()
    p.curve, p.flags, p.exposure, p.white, p.key = 2, 1, 3.0, 4.0, 5.0
    p.reserved[2] = 7.0
    L.kajo_hip_default_tone_params(C.byref(p))
    assert (p.curve, p.flags, p.exposure, p.white) == (capi.KAJO_TONE_CLAMP, 0, 0.0, 0.0)
    assert p.key == pytest.approx(0.18, rel=1e-7)
    assert list(p.reserved) == [0.0, 0.0, 0.0]
    L.kajo_hip_default_tone_params(None)  # accepted


def _params(**kw):
    L = capi.lib()
    p = capi.KajoToneParams()
    L.kajo_hip_default_tone_params(C.byref(p))
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[1] = v
        else:
            setattr(p, k, v)
    return p


def _refusals(p):
    """What each of the three entry points that take parameters answers on a NULL handle with `p`."""
    L = capi.lib()
    ref = None if p is None else C.byref(p)
    out = []
    for rc in (L.kajo_hip_tonemap_argb8(None, ref, None, None, None), L.kajo_hip_tonemap_gathered_argb8_device(None, None, ref, None)):
        out.append((rc, L.kajo_hip_last_error().decode()))
    return out


BAD = [
    (dict(curve=3), "curve"), (dict(curve=-1), "curve"), (dict(flags=2), "flag"), (dict(flags=0x80000000), "flag"),
    (dict(exposure=float("nan")), "exposure"), (dict(exposure=float("inf")), "exposure"), (dict(exposure=32.5), "exposure"),
    (dict(exposure=-33.0), "exposure"), (dict(white=-1.0), "white"), (dict(white=float("inf")), "white"),
    (dict(white=float("nan")), "white"), (dict(flags=1, key=0.0), "key"), (dict(flags=1, key=-0.18), "key"),
    (dict(flags=1, key=float("nan")), "key"), (dict(flags=1, key=float("inf")), "key"), (dict(reserved=1.0), "reserved"),
]


@pytest.mark.parametrize("bad,word", BAD)
def test_bad_parameters_are_refused_before_the_handle_is_looked_at(bad, word):
    for rc, msg in _refusals(_params(**bad)):
        assert rc == capi.KAJO_E_INVALID and word in msg, (bad, rc, msg)


@pytest.mark.parametrize("ok", [dict(), dict(curve=1, white=0.0), dict(curve=2, exposure=32.0), dict(exposure=-32.0),
                                dict(key=0.0), dict(key=float("nan")), dict(flags=1, key=1e-6), dict(curve=1, white=1e30)])
def test_good_parameters_pass_on_to_the_handle_check(ok):
    """(the key is only looked at with KAJO_TONE_AUTO_EXPOSURE)"""
    for rc, msg in _refusals(_params(**ok)):
        assert (rc, msg) in ((capi.KAJO_E_INVALID, "null handle"), (capi.KAJO_E_INVALID, "null argument")), (ok, rc, msg)


def test_null_parameters_and_handles_are_refused():
    L = capi.lib()
    for rc, msg in _refusals(None):
        assert rc == capi.KAJO_E_INVALID and msg == "null tone parameters"
    assert L.kajo_hip_tone_scale(None, None) == capi.KAJO_E_INVALID
    s = C.c_float(-1.0)
    assert L.kajo_hip_tone_scale(None, C.byref(s)) == capi.KAJO_E_INVALID and s.value == -1.0
    # with denoise parameters, theirs are checked as kajo_hip_denoise checks them, still before the handle
    d = capi.KajoDenoiseParams()
    L.kajo_hip_default_denoise_params(C.byref(d))
    d.iterations = 9
    p = _params()
    assert L.kajo_hip_tonemap_argb8(None, C.byref(p), C.byref(d), None, None) == capi.KAJO_E_INVALID
    assert "iterations" in L.kajo_hip_last_error().decode()
    d.iterations = 5
    assert L.kajo_hip_tonemap_argb8(None, C.byref(p), C.byref(d), None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_last_error().decode() == "null handle"


def _compile(unit):
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("hipcc / make not available")
    obj = os.path.join(CSRC, "build", "kernel_%s.o" % unit)
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, obj], capture_output=True, text=True, check=True).stdout
    cmd = next(l for l in plan.splitlines() if l.startswith("hipcc") and "kernel_%s.hip" % unit in l).split()
    tmp = tempfile.mkdtemp(prefix="kajo_tone_res_")
    asm = os.path.join(tmp, "k.s")
    i = cmd.index("-c")
    cmd = cmd[:i] + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"] + cmd[i + 1:]
    cmd[cmd.index("-o") + 1] = asm
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
    text = open(asm).read()
    shutil.rmtree(tmp, ignore_errors=True)
    return res, text


def _body(asm, kernel):
    body = asm[asm.index("\n" + kernel + ":"):]
    return body[:body.index("s_endpgm")]


@pytest.mark.parametrize("unit", ["fast", "strict"])
def test_tone_kernels_spill_nothing_and_use_no_scratch_flat_atomics_or_scalar_stores(unit):
    res, asm = _compile(unit)
    for base in KERNELS:
        k = "%s_%s" % (base, unit)
        assert k in res, (k, sorted(res))
        r = res[k]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        body = _body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k
        assert not re.search(r"\n\s+s_(buffer_|scratch_)?store\w*", body), k
        assert not re.search(r"\n\s+s_dcache_(wb|discard)\w*", body), k
        # written with plain vector stores to global memory
        assert re.search(r"\n\s+global_store_dword", body), k
    # the reductions: a cross-lane butterfly and the float64 sums, no atomics (above)
    for base in ("kajo_tone_logavg_tiles", "kajo_tone_logavg_frame", "kajo_tone_scale"):
        body = _body(asm, "%s_%s" % (base, unit))
        assert "ds_swizzle_b32" in body and "v_add_f64" in body, base


def test_exact_unit_has_no_tone_kernels_of_its_own():
    """EXACT handles tone-map with the STRICT build's kernels, as they resolve with them."""
    res, _ = _compile("exact")
    assert not [k for k in res if k.startswith("kajo_tone")]


def test_makefile_builds_the_tone_kernels_into_the_product_and_the_tools_twin():
    """They live in the two kernel units (for the builds' own kdiv / kpow), whose objects both libraries link."""
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("kernel_fast.o" in l and "kernel_strict.o" in l for l in links), links
    for unit in ("fast", "strict"):
        assert '#include "tonemap.inc.hip"' in open(os.path.join(CSRC, "kernel_%s.hip" % unit)).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    for unit in ("fast", "strict"):
        assert re.search(r"\bT kajo_tone_%s_launch\b" % unit, nm), unit
    tune = os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")
    if os.path.exists(tune):
        nm = subprocess.run(["nm", "-D", "--defined-only", tune], capture_output=True, text=True).stdout
        assert re.search(r"\bT kajo_hip_tonemap_argb8\b", nm) and re.search(r"\bT kajo_tone_strict_launch\b", nm)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--tonemap", "filmic"], "--tonemap must be clamp, reinhard or aces"),
    (["--tonemap", "ACES"], "--tonemap must be clamp, reinhard or aces"),
    (["--exposure", "32.5"], "--exposure must be a number in -32..32"),
    (["--exposure", "-40"], "--exposure must be a number in -32..32"),
    (["--exposure", "nan"], "--exposure must be a number in -32..32"),
    (["--exposure", "2stops"], "--exposure must be a number in -32..32"),
    (["--white", "-1"], "--white must be a finite number >= 0"),
    (["--white", "inf"], "--white must be a finite number >= 0"),
    (["--key", "0"], "--key must be a finite number > 0"),
    (["--key", "-0.5"], "--key must be a finite number > 0"),
    (["--auto-exposure", "--key", "x"], "--key must be a finite number > 0"),
    (["--tonemap", "aces", "--three-arg"], "the tone options need the backend's options"),
])
def test_driver_refuses_bad_tone_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out), "--hdr", str(tmp_path / "h.pfm")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_tone_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--tonemap CURVE", "--exposure EV", "--white W", "--auto-exposure", "--key K", "--hdr FILE"):
        assert opt in text, opt
