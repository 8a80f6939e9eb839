"""The noise-guided denoiser (include/kajo_hip.h KAJO_DENOISE_NOISE_GUIDED, kajo_hip_denoise_guide_planes;
kajo_amd/csrc/denoise_guided.cpp) without a GPU: the flag and the entry point as the header declares them, the refusals that need no
device, how the Makefile builds and links the unit, what the compiler made of its kernel (nothing spilled, no scratch, no FLAT
instruction, no atomic), and the driver's refusal of --denoise-noise-guided without --denoise. The compile command is the Makefile's own
(`make -n`)."""
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
KERNELS = ("kajo_denoise_guided_v0",)  # (prepare, the iterations and remodulate are denoise.hip's, launched by declaration)


def _header():
    return open(os.path.join(ROOT, "include", "kajo_hip.h")).read()


def test_header_capi_and_library_agree_on_the_flag_and_the_export():
    header = _header()
    m = re.search(r"#define KAJO_DENOISE_NOISE_GUIDED (\d+)u", header)
    assert m and int(m.group(1)) == capi.KAJO_DENOISE_NOISE_GUIDED == 2
    assert capi.KAJO_DENOISE_NOISE_GUIDED & capi.KAJO_DENOISE_NO_DEMODULATE == 0
    assert re.search(r"\bint kajo_hip_denoise_guide_planes\s*\(kajo_hip_t h, const float\* mean, const float\* stderror\);", header)
    assert "kajo_hip_denoise_guide_planes" in capi.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT kajo_hip_denoise_guide_planes\b", nm)
    assert capi.lib().kajo_hip_denoise_guide_planes.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    # the parameters keep their 8 words and their fields
    assert C.sizeof(capi.KajoDenoiseParams) == 32
    fields = re.search(r"typedef struct KajoDenoiseParams \{(.*?)\} KajoDenoiseParams;", header, re.S).group(1)
    assert re.findall(r"\b(iterations|flags|sigmaLuminance|sigmaNormal|sigmaDepth|reserved)\b", fields) == \
        [f for f, _ in capi.KajoDenoiseParams._fields_]
    assert re.search(r"float reserved\[3\];", fields)


def test_guide_planes_refuse_one_null_plane_before_the_handle_and_then_a_null_handle():
    L = capi.lib()
    plane = (C.c_float * 4)()
    for mean, se in ((plane, None), (None, plane)):
        assert L.kajo_hip_denoise_guide_planes(None, mean, se) == capi.KAJO_E_INVALID
        msg = L.kajo_hip_last_error().decode()
        assert "together" in msg and "handle" not in msg, msg
    for mean, se in ((plane, plane), (None, None)):
        assert L.kajo_hip_denoise_guide_planes(None, mean, se) == capi.KAJO_E_INVALID
        assert L.kajo_hip_last_error().decode() == "null handle"


@pytest.mark.parametrize("iterations", [-1, 9])
def test_the_flag_with_out_of_range_iterations_is_refused_for_the_iterations(iterations):
    L = capi.lib()
    p = capi.KajoDenoiseParams()
    L.kajo_hip_default_denoise_params(C.byref(p))
    assert p.flags == 0  # off by default
    p.flags = capi.KAJO_DENOISE_NOISE_GUIDED
    p.iterations = iterations
    assert L.kajo_hip_denoise(None, C.byref(p), None, None) == capi.KAJO_E_INVALID
    assert "iterations" in L.kajo_hip_last_error().decode()
    p.iterations = 5
    assert L.kajo_hip_denoise(None, C.byref(p), None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_last_error().decode() == "null handle"


def test_makefile_compiles_the_unit_as_hip_without_contraction_and_links_it_into_the_product_and_the_tools_twin():
    devicecode.need_tools()
    cmd = devicecode.compile_command("denoise_guided.cpp")
    assert "-ffp-contract=off" in cmd and "-ffp-contract=fast" not in cmd
    assert cmd[cmd.index("-x") + 1] == "hip" and "--offload-arch=gfx950" in cmd
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("denoise_guided.o" in l and "denoise.o" in l for l in links), links


def test_the_units_kernels_spill_nothing_and_use_no_scratch_flat_or_atomics():
    b = devicecode.build("denoise_guided.cpp")
    res, asm = b.resources, b.asm
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k in KERNELS:
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k
        # the frame is written with plain vector stores to global memory
        assert re.search(r"\n\s+global_store_dwordx4", body), k


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_refuses_noise_guided_without_denoise(tmp_path):
    """`kajo_render --denoise-noise-guided` steers the denoiser of --denoise (or of the display chain's denoise): alone it is refused at
    argument parsing, before a device is opened, with nothing written."""
    p = subprocess.run([BIN, "--denoise-noise-guided", "-o", str(tmp_path / "x.png")], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "--denoise-noise-guided needs --denoise" in p.stderr, p.stderr
    assert not list(tmp_path.iterdir())
    assert "--denoise-noise-guided" in subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
