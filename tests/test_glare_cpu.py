"""The glare (bloom) pyramid (include/kajo_hip.h kajo_hip_glare, kajo_amd/csrc/glare.hip) without a GPU: the struct and the entry points
as the header declares them, in the product and the tools' twin; the documented defaults; every refusal that comes before a device is
looked at, and their order (glare, tone, denoise, handle); what the compiler made of the kernels (nothing spilled, no scratch, no FLAT
instruction, no atomic); and the driver's refusals of bad option values. The compile command is the Makefile's own (`make -n`)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import devicecode
from kajo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
ENTRY_POINTS = ("kajo_hip_default_glare_params", "kajo_hip_glare", "kajo_hip_display_argb8", "kajo_hip_display_gathered_argb8_device")
KERNELS = ("kajo_glare_bright", "kajo_glare_reduce", "kajo_glare_expand", "kajo_glare_apply")


def _header():
    return open(os.path.join(ROOT, "include", "kajo_hip.h")).read()


def test_header_struct_binding_and_libraries_agree():
    header = _header()
    assert C.sizeof(capi.KajoGlareParams) == 32
    fields = re.search(r"typedef struct KajoGlareParams \{(.*?)\} KajoGlareParams;", header, re.S).group(1)
    names = re.findall(r"^\s+\w+ (\w+)(?:\[\d+\])?;", fields, re.M)
    assert names == [f for f, _ in capi.KajoGlareParams._fields_] == ["levels", "flags", "strength", "threshold", "reserved"]
    assert re.search(r"float reserved\[4\];", fields)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    libs = [capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")]
    for lib in libs:
        assert os.path.exists(lib), lib
        nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in ENTRY_POINTS + ("kajo_glare_launch",):
            assert re.search(r"\bT %s\b" % name, nm), (lib, name)
    # the structs beside it keep their sizes
    assert C.sizeof(capi.KajoToneParams) == 32 and C.sizeof(capi.KajoDenoiseParams) == 32


def test_default_params_are_the_documented_ones():
    L = capi.lib()
    p = capi.KajoGlareParams()
    p.levels, p.flags, p.strength, p.threshold = 3, 1, 0.7, 2.0
    p.reserved[3] = 7.0
    L.kajo_hip_default_glare_params(C.byref(p))
    assert (p.levels, p.flags, p.threshold) == (6, 0, 0.0)
    assert p.strength == pytest.approx(0.1, rel=1e-7)
    assert list(p.reserved) == [0.0, 0.0, 0.0, 0.0]
    L.kajo_hip_default_glare_params(None)  # accepted
    header = _header()
    for text in ("0..12 (default 6)", "0..1 (default 0.1)", ">= 0, finite (default 0"):
        assert text in header, text


def _glare(**kw):
    p = capi.KajoGlareParams()
    capi.lib().kajo_hip_default_glare_params(C.byref(p))
    for k, v in kw.items():
        if k.startswith("reserved"):
            p.reserved[int(k[len("reserved"):])] = v
        else:
            setattr(p, k, v)
    return p


def _tone(**kw):
    p = capi.KajoToneParams()
    capi.lib().kajo_hip_default_tone_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _denoise(**kw):
    p = capi.KajoDenoiseParams()
    capi.lib().kajo_hip_default_denoise_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ref(p):
    return None if p is None else C.byref(p)


def _refusals(g, tone=None, denoise=None):
    """What each of the three entry points that take glare parameters answers on a NULL handle: [(rc, message)] for kajo_hip_glare,
    kajo_hip_display_argb8, kajo_hip_display_gathered_argb8_device."""
    L = capi.lib()
    tone = tone or _tone()
    out = []
    for call in (lambda: L.kajo_hip_glare(None, _ref(g), _ref(denoise), None),
                 lambda: L.kajo_hip_display_argb8(None, _ref(denoise), _ref(g), _ref(tone), None, None),
                 lambda: L.kajo_hip_display_gathered_argb8_device(None, None, _ref(g), _ref(tone), None)):
        rc = call()
        out.append((rc, L.kajo_hip_last_error().decode()))
    return out


BAD = [
    (dict(levels=-1), "levels"), (dict(levels=13), "levels"), (dict(flags=1), "flag"), (dict(flags=0x80000000), "flag"),
    (dict(strength=-0.01), "strength"), (dict(strength=1.5), "strength"), (dict(strength=float("nan")), "strength"),
    (dict(strength=float("inf")), "strength"), (dict(threshold=-1.0), "threshold"), (dict(threshold=float("inf")), "threshold"),
    (dict(threshold=float("nan")), "threshold"), (dict(reserved0=1.0), "reserved"), (dict(reserved3=-2.0), "reserved"),
]


@pytest.mark.parametrize("bad,word", BAD)
def test_bad_parameters_are_refused_before_the_handle_is_looked_at(bad, word):
    for rc, msg in _refusals(_glare(**bad)):
        assert rc == capi.KAJO_E_INVALID and word in msg and "glare" in msg, (bad, rc, msg)


@pytest.mark.parametrize("ok", [dict(), dict(levels=0), dict(levels=12), dict(strength=0.0), dict(strength=1.0), dict(threshold=1e30)])
def test_good_parameters_pass_on_to_the_handle_check(ok):
    for rc, msg in _refusals(_glare(**ok)):
        assert (rc, msg) in ((capi.KAJO_E_INVALID, "null handle"), (capi.KAJO_E_INVALID, "null argument")), (ok, rc, msg)


def test_null_glare_parameters():
    """kajo_hip_glare refuses them; for the display entry points NULL means no glare, and they go on to the handle."""
    (rc, msg), display, gathered = _refusals(None)
    assert (rc, msg) == (capi.KAJO_E_INVALID, "null glare parameters")
    assert display == (capi.KAJO_E_INVALID, "null handle") and gathered == (capi.KAJO_E_INVALID, "null argument")


def test_order_of_refusals_glare_then_tone_then_denoise_then_handle():
    L = capi.lib()
    bad_g, bad_t, bad_d = _glare(levels=13), _tone(curve=7), _denoise(iterations=9)
    # everything bad: the glare parameters speak first, through every entry point
    for rc, msg in _refusals(bad_g, bad_t, bad_d):
        assert rc == capi.KAJO_E_INVALID and "glare levels" in msg, msg
    # glare good: the tone parameters (the two entry points that take them), kajo_hip_glare goes on to the denoiser's
    glare, display, gathered = _refusals(_glare(), bad_t, bad_d)
    assert "iterations" in glare[1] and "tone curve" in display[1] and "tone curve" in gathered[1], (glare, display, gathered)
    # the tone parameters' reserved words stay refused
    t = _tone()
    t.reserved[1] = 1.0
    assert all("tone reserved" in m for _, m in _refusals(_glare(), t, bad_d)[1:])
    assert L.kajo_hip_display_argb8(None, None, None, None, None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_last_error().decode() == "null tone parameters"
    # glare and tone good: the denoiser's, then the handle
    glare, display, gathered = _refusals(_glare(), _tone(), bad_d)
    assert "iterations" in glare[1] and "iterations" in display[1] and gathered[1] == "null argument"
    for rc, msg in _refusals(_glare(), _tone(), _denoise())[:2]:
        assert (rc, msg) == (capi.KAJO_E_INVALID, "null handle")


def _compile():
    b = devicecode.build("glare.hip")
    assert "-ffp-contract=off" in b.cmd and "--offload-arch=gfx950" in b.cmd
    return b.resources, b.asm


def test_glare_kernels_spill_nothing_and_use_no_scratch_flat_or_atomics():
    res, asm = _compile()
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k in KERNELS:
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        assert r["LDS Size"] == 0 and r["Occupancy"] == 8, (k, r)  # (the plain gather: full occupancy, nothing staged)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k
        # no cross-lane operation: every lane forms its own pixel
        assert not re.search(r"\n\s+(ds_\w+|v_readlane\w*|v_permlane\w*|\w+_dpp)\b", body), k
        # one access per lane and tap -- the whole float4, or its three colour words where .w is not used -- and plain 16-byte vector stores
        loads = set(re.findall(r"\n\s+(global_load_\w+)", body))
        assert loads and loads <= {"global_load_dwordx3", "global_load_dwordx4"}, (k, loads)
        assert set(re.findall(r"\n\s+(global_store_\w+)", body)) == {"global_store_dwordx4"}, k


def test_makefile_links_the_glare_into_the_product_and_the_tools_twin():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("glare.o" in l and "denoise.o" in l for l in links), links


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--glare-levels", "4"], "give them with --glare"),
    (["--glare-threshold", "1"], "give them with --glare"),
    (["--glare", "1.5"], "--glare must be a number in 0..1"),
    (["--glare", "-0.1"], "--glare must be a number in 0..1"),
    (["--glare", "nan"], "--glare must be a number in 0..1"),
    (["--glare", "lots"], "--glare must be a number in 0..1"),
    (["--glare", "0.1", "--glare-levels", "13"], "--glare-levels must be in 0..12"),
    (["--glare", "0.1", "--glare-levels", "-1"], "--glare-levels must be in 0..12"),
    (["--glare", "0.1", "--glare-levels", "4x"], "--glare-levels must be in 0..12"),
    (["--glare", "0.1", "--glare-threshold", "-1"], "--glare-threshold must be a finite number >= 0"),
    (["--glare", "0.1", "--glare-threshold", "inf"], "--glare-threshold must be a finite number >= 0"),
    (["--glare", "0.1", "--three-arg"], "the glare options need the backend's options"),
    (["--glare", "0.1", "--denoise", "d.png", "--gpus", "2"], "--denoise needs the whole frame on one GPU"),
])
def test_driver_refuses_bad_glare_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_glare_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--glare STRENGTH", "--glare-levels N", "--glare-threshold T"):
        assert opt in text, opt
