"""The A-trous denoiser (include/kajo_hip.h kajo_hip_denoise, kajo_amd/csrc/denoise.hip) without a GPU: the entry points and the flag as
the header declares them, the argument refusals that need no device, the documented defaults, what the compiler made of the kernels
(nothing spilled, no scratch, no FLAT instruction, no atomic), and the driver's refusal of --denoise on more than one GPU. The compile
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
KERNELS = ("kajo_denoise_prepare", "kajo_denoise_variance", "kajo_denoise_atrous", "kajo_denoise_remodulate")


def _header():
    return open(os.path.join(ROOT, "include", "kajo_hip.h")).read()


def test_header_exports_and_library_agree():
    header = _header()
    m = re.search(r"#define KAJO_DENOISE_NO_DEMODULATE (\d+)u", header)
    assert m and int(m.group(1)) == capi.KAJO_DENOISE_NO_DEMODULATE == 1
    for name in ("kajo_hip_default_denoise_params", "kajo_hip_denoise"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT kajo_hip_default_denoise_params\b", nm) and re.search(r"\bT kajo_hip_denoise\b", nm)
    # the struct as the header lays it out: 8 words
    assert C.sizeof(capi.KajoDenoiseParams) == 32
    fields = re.search(r"typedef struct KajoDenoiseParams \{(.*?)\} KajoDenoiseParams;", header, re.S).group(1)
    names = re.findall(r"\b(iterations|flags|sigmaLuminance|sigmaNormal|sigmaDepth|reserved)\b", fields)
    assert names == [f for f, _ in capi.KajoDenoiseParams._fields_]


def test_default_params_are_the_documented_ones():
    L = capi.lib()
    p = capi.KajoDenoiseParams()
    p.reserved[1] = 7.0
    L.kajo_hip_default_denoise_params(C.byref(p))
    assert (p.iterations, p.flags, p.sigmaLuminance, p.sigmaNormal, p.sigmaDepth) == (5, 0, 4.0, 128.0, 1.0)
    assert list(p.reserved) == [0.0, 0.0, 0.0]
    L.kajo_hip_default_denoise_params(None)  # accepted


def _params(**kw):
    L = capi.lib()
    p = capi.KajoDenoiseParams()
    L.kajo_hip_default_denoise_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _refusal(p):
    L = capi.lib()
    rc = L.kajo_hip_denoise(None, None if p is None else C.byref(p), None, None)
    return rc, L.kajo_hip_last_error().decode()


def test_null_arguments_are_refused():
    assert _refusal(None) == (capi.KAJO_E_INVALID, "null denoise parameters")
    assert _refusal(_params()) == (capi.KAJO_E_INVALID, "null handle")


@pytest.mark.parametrize("bad", [dict(iterations=-1), dict(iterations=9), dict(sigmaLuminance=-1.0), dict(sigmaNormal=float("nan")),
                                 dict(sigmaDepth=float("inf")), dict(sigmaDepth=-0.5)])
def test_out_of_range_parameters_are_refused_before_the_handle_is_looked_at(bad):
    rc, msg = _refusal(_params(**bad))
    assert rc == capi.KAJO_E_INVALID
    assert ("iterations" in msg) if "iterations" in bad else ("sigmas" in msg), msg


@pytest.mark.parametrize("ok", [dict(iterations=0), dict(iterations=8), dict(sigmaLuminance=0.0, sigmaNormal=0.0, sigmaDepth=0.0)])
def test_in_range_parameters_pass_on_to_the_handle_check(ok):
    assert _refusal(_params(**ok)) == (capi.KAJO_E_INVALID, "null handle")


def _compile():
    b = devicecode.build("denoise.hip")
    assert "-ffp-contract=off" in b.cmd
    return b.resources, b.asm


def test_denoise_kernels_spill_nothing_and_use_no_scratch_flat_or_atomics():
    res, asm = _compile()
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k in KERNELS:
        r = res[k]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k
        assert not re.search(r"\n\s+s_(buffer_)?store\w*", body), k
        # the frames are written with plain vector stores to global memory
        assert re.search(r"\n\s+global_store_dwordx4", body), k


def test_makefile_links_the_denoiser_into_the_product_and_the_tools_twin():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("denoise.o" in l for l in links), links


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("gpus", ["2", "0"])
def test_driver_refuses_denoise_on_more_than_one_gpu(tmp_path, gpus):
    """`kajo_render --denoise` reads the AOV buffers of one whole-frame handle: any --gpus other than 1 (0 = every visible GPU) is refused
    at argument parsing, before a device is opened."""
    out = tmp_path / "d.png"
    p = subprocess.run([BIN, "--denoise", str(out), "--gpus", gpus, "-o", ""], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "--denoise needs the whole frame on one GPU" in p.stderr, p.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_refuses_iterations_out_of_range(tmp_path):
    p = subprocess.run([BIN, "--denoise", str(tmp_path / "d.png"), "--denoise-iterations", "9", "-o", ""], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode != 0 and "--denoise-iterations must be in 0..8" in p.stderr, p.stderr
    assert "--denoise FILE" in subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
