"""The despeckle stage (include/kajo_hip.h kajo_hip_despeckle, kajo_amd/csrc/despeckle.hip) without a GPU: the struct and the entry
points as the header declares them, in the product and the tools' twin; the documented defaults; every refusal that comes before a
device is looked at, and their order (despeckle, glare, tone, denoise, handle); what the compiler made of the kernels (nothing spilled,
no scratch, no FLAT instruction, no atomic; registers and occupancy pinned); and the driver's refusals of bad option values. The compile
command is the Makefile's own (`make -n`)."""
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
ENTRY_POINTS = ("kajo_hip_default_despeckle_params", "kajo_hip_despeckle", "kajo_hip_present_argb8", "kajo_hip_present_gathered_argb8_device",
                "kajo_hip_despeckle_counts")
# kernel -> (VGPRs, LDS bytes): what hipcc makes of them. The registers are pinned to within VGPR_ROOM, so that
# a change to a kernel that moves them is seen long before it costs a wave (8 waves per SIMD hold up to 64).
KERNELS = {"kajo_despeckle_clamp": (50, 16), "kajo_despeckle_repair": (37, 16), "kajo_despeckle_counts": (38, 4096)}
VGPR_ROOM = 2


def _header():
    return open(os.path.join(ROOT, "include", "kajo_hip.h")).read()


def test_header_struct_binding_and_libraries_agree():
    header = _header()
    assert C.sizeof(capi.KajoDespeckleParams) == 32
    fields = re.search(r"typedef struct KajoDespeckleParams \{(.*?)\} KajoDespeckleParams;", header, re.S).group(1)
    names = re.findall(r"^\s+\w+ (\w+)(?:\[\d+\])?;", fields, re.M)
    assert names == [f for f, _ in capi.KajoDespeckleParams._fields_] == ["factor", "rank", "floor", "flags", "reserved"]
    assert re.search(r"float reserved\[4\];", fields)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        assert os.path.exists(lib), lib
        nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in ENTRY_POINTS + ("kajo_despeckle_launch",):
            assert re.search(r"\bT %s\b" % name, nm), (lib, name)
    # the structs beside it keep their sizes
    assert C.sizeof(capi.KajoToneParams) == 32 and C.sizeof(capi.KajoDenoiseParams) == 32 and C.sizeof(capi.KajoGlareParams) == 32


def test_default_params_are_the_documented_ones():
    L = capi.lib()
    p = capi.KajoDespeckleParams()
    p.factor, p.rank, p.floor, p.flags = 9.0, 4, 2.0, 1
    p.reserved[3] = 7.0
    L.kajo_hip_default_despeckle_params(C.byref(p))
    assert (p.factor, p.rank, p.flags) == (16.0, 1, 0)
    assert p.floor == pytest.approx(0.2, rel=1e-7)
    assert list(p.reserved) == [0.0, 0.0, 0.0, 0.0]
    L.kajo_hip_default_despeckle_params(None)  # accepted
    header = _header()
    for text in ("finite (default 16)", "1..4 (default 1)", "finite (default 0.2)"):
        assert text in header, text


def _params(cls, default, **kw):
    p = cls()
    getattr(capi.lib(), default)(C.byref(p))
    for k, v in kw.items():
        if k.startswith("reserved"):
            p.reserved[int(k[len("reserved"):])] = v
        else:
            setattr(p, k, v)
    return p


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


def _refusals(d, glare=None, tone=None, denoise=None):
    """What each of the three entry points that take despeckle parameters answers on a NULL handle: [(rc, message)] for
    kajo_hip_despeckle, kajo_hip_present_argb8, kajo_hip_present_gathered_argb8_device."""
    L = capi.lib()
    tone = tone or _tone()
    out = []
    for call in (lambda: L.kajo_hip_despeckle(None, _ref(d), None, None),
                 lambda: L.kajo_hip_present_argb8(None, _ref(d), _ref(denoise), _ref(glare), _ref(tone), None, None),
                 lambda: L.kajo_hip_present_gathered_argb8_device(None, None, _ref(d), _ref(glare), _ref(tone), None)):
        rc = call()
        out.append((rc, L.kajo_hip_last_error().decode()))
    return out


BAD = [
    (dict(factor=-1.0), "factor"), (dict(factor=0.5), "factor"), (dict(factor=0.999), "factor"), (dict(factor=1e-30), "factor"),
    (dict(factor=float("nan")), "factor"), (dict(factor=float("inf")), "factor"), (dict(rank=0), "rank"), (dict(rank=5), "rank"),
    (dict(rank=-1), "rank"), (dict(floor=-0.01), "floor"), (dict(floor=float("inf")), "floor"), (dict(floor=float("nan")), "floor"),
    (dict(flags=1), "flag"), (dict(flags=0x80000000), "flag"), (dict(reserved0=1.0), "reserved"), (dict(reserved3=-2.0), "reserved"),
]


@pytest.mark.parametrize("bad,word", BAD)
def test_bad_parameters_are_refused_before_the_handle_is_looked_at(bad, word):
    for rc, msg in _refusals(_despeckle(**bad)):
        assert rc == capi.KAJO_E_INVALID and word in msg and "despeckle" in msg, (bad, rc, msg)


@pytest.mark.parametrize("ok", [dict(), dict(factor=0.0), dict(factor=1.0), dict(factor=1e30), dict(rank=1), dict(rank=4), dict(floor=0.0),
                                dict(floor=1e30)])
def test_good_parameters_pass_on_to_the_handle_check(ok):
    for rc, msg in _refusals(_despeckle(**ok)):
        assert (rc, msg) in ((capi.KAJO_E_INVALID, "null handle"), (capi.KAJO_E_INVALID, "null argument")), (ok, rc, msg)


def test_null_despeckle_parameters():
    """kajo_hip_despeckle refuses them; for the present entry points NULL means no despeckle: they are the display entry points."""
    (rc, msg), present, gathered = _refusals(None)
    assert (rc, msg) == (capi.KAJO_E_INVALID, "null despeckle parameters")
    assert present == (capi.KAJO_E_INVALID, "null handle") and gathered == (capi.KAJO_E_INVALID, "null argument")
    _, present, gathered = _refusals(None, glare=_glare(levels=13))
    assert "glare levels" in present[1] and "glare levels" in gathered[1]
    L = capi.lib()
    assert L.kajo_hip_despeckle_counts(None, None) == capi.KAJO_E_INVALID


def test_order_of_refusals_despeckle_then_glare_then_tone_then_denoise_then_handle():
    bad_s, bad_g, bad_t, bad_d = _despeckle(rank=9), _glare(levels=13), _tone(curve=7), _denoise(iterations=9)
    for rc, msg in _refusals(bad_s, bad_g, bad_t, bad_d):
        assert rc == capi.KAJO_E_INVALID and "despeckle rank" in msg, msg
    _, present, gathered = _refusals(_despeckle(), bad_g, bad_t, bad_d)
    assert "glare levels" in present[1] and "glare levels" in gathered[1]
    _, present, gathered = _refusals(_despeckle(), _glare(), bad_t, bad_d)
    assert "tone curve" in present[1] and "tone curve" in gathered[1]
    _, present, gathered = _refusals(_despeckle(), _glare(), _tone(), bad_d)
    assert "iterations" in present[1] and gathered[1] == "null argument"
    _, present, _ = _refusals(_despeckle(), _glare(), _tone(), _denoise())
    assert present == (capi.KAJO_E_INVALID, "null handle")
    L = capi.lib()
    assert L.kajo_hip_present_argb8(None, C.byref(_despeckle()), None, None, None, None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_last_error().decode() == "null tone parameters"


def _compile():
    b = devicecode.build("despeckle.hip")
    assert "-ffp-contract=off" in b.cmd and "--offload-arch=gfx950" in b.cmd
    return b.resources, b.asm


def test_despeckle_kernels_spill_nothing_and_use_no_scratch_flat_or_atomics():
    res, asm = _compile()
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k, (vgprs, lds) in KERNELS.items():
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        assert abs(r["VGPRs"] - vgprs) <= VGPR_ROOM and r["Occupancy"] == 8 and r["LDS Size"] == lds, (k, r)  # (full occupancy; LDS: the counts only)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k
        stores = set(re.findall(r"\n\s+(global_store_\w+)", body))
        if k == "kajo_despeckle_counts":
            assert stores == {"global_store_dwordx2"}, (k, stores)
            continue
        # one access per lane and tap -- the whole float4, or its three colour words where .w is not used -- one 16-byte store for the
        # pixel and one word per workgroup for its count
        loads = set(re.findall(r"\n\s+(global_load_\w+)", body))
        assert loads and loads <= {"global_load_dwordx3", "global_load_dwordx4"}, (k, loads)
        assert stores == {"global_store_dwordx4", "global_store_dword"}, (k, stores)


def test_makefile_links_the_despeckle_into_the_product_and_the_tools_twin():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("despeckle.o" in l and "glare.o" in l and "denoise.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "despeckle.hip" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0], compiles


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--despeckle-factor", "4"], "give them with --despeckle"),
    (["--despeckle-rank", "2"], "give them with --despeckle"),
    (["--despeckle-floor", "0.1"], "give them with --despeckle"),
    (["--despeckle", "--despeckle-factor", "0.5"], "--despeckle-factor must be 0 or a finite number >= 1"),
    (["--despeckle", "--despeckle-factor", "-1"], "--despeckle-factor must be 0 or a finite number >= 1"),
    (["--despeckle", "--despeckle-factor", "nan"], "--despeckle-factor must be 0 or a finite number >= 1"),
    (["--despeckle", "--despeckle-factor", "lots"], "--despeckle-factor must be 0 or a finite number >= 1"),
    (["--despeckle", "--despeckle-rank", "0"], "--despeckle-rank must be in 1..4"),
    (["--despeckle", "--despeckle-rank", "5"], "--despeckle-rank must be in 1..4"),
    (["--despeckle", "--despeckle-rank", "2x"], "--despeckle-rank must be in 1..4"),
    (["--despeckle", "--despeckle-floor", "-1"], "--despeckle-floor must be a finite number >= 0"),
    (["--despeckle", "--despeckle-floor", "inf"], "--despeckle-floor must be a finite number >= 0"),
    (["--despeckle", "--three-arg"], "the despeckle options need the backend's options"),
])
def test_driver_refuses_bad_despeckle_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_despeckle_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--despeckle ", "--despeckle-factor F", "--despeckle-rank R", "--despeckle-floor X"):
        assert opt in text, opt
