"""First-hit AOVs (KAJO_FLAG_AOV, include/kajo_hip.h kajo_hip_read_aov) without a GPU: the flag and the entry points as the header
declares them, the refusals that come before any device is opened, and what the compiler made of the AOV kernels -- every instance
present in both kernel translation units, nothing spilled, no scratch, no FLAT memory instruction (the rule the render kernels keep,
tests/test_kernel_resources_cpu.py). The compile command is the Makefile's own (`make -n`)."""
import os
import re
import subprocess

import pytest

import devicecode
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
INSTANCES = ("", "_big", "_big_lg", "_biglist", "_biglist_lg")


def _compile(unit):
    """(resource remarks per kernel, assembly) of kernel_<unit>.hip compiled as the Makefile compiles it (device code only)."""
    b = devicecode.build("kernel_%s.hip" % unit)
    return b.resources, b.asm


def test_header_and_binding_agree_on_the_flag():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    m = re.search(r"#define KAJO_FLAG_AOV (\d+)u", header)
    assert m and int(m.group(1)) == capi.KAJO_FLAG_AOV == 1024
    # a bit of its own among the flags
    others = [int(v) for k, v in re.findall(r"#define (KAJO_FLAG_\w+) (\d+)u", header) if k != "KAJO_FLAG_AOV"]
    assert all(v & capi.KAJO_FLAG_AOV == 0 for v in others), others
    assert "kajo_hip_read_aov" in capi.EXPORTS and "kajo_hip_aov_kernel" in capi.EXPORTS


def test_library_exports_the_aov_entry_points():
    L = capi.lib()
    assert hasattr(L, "kajo_hip_read_aov") and hasattr(L, "kajo_hip_aov_kernel")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT kajo_hip_read_aov\b", nm) and re.search(r"\bT kajo_hip_aov_kernel\b", nm)
    # null handles are refused, not dereferenced
    assert L.kajo_hip_read_aov(None, None, None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_aov_kernel(None) is None


def test_aov_on_a_tiled_handle_is_refused(scenes):
    """The AOV buffers are whole-frame buffers of one handle: the flag with tileCount != 1 is refused at create, before any device is
    looked for (so the refusal shows here too)."""
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(scenes["spheres_a1"], 64, 32, aov=True, tile_index=0, tile_count=2)
    assert e.value.code == capi.KAJO_E_INVALID and "tileCount 1" in str(e.value)


@pytest.mark.parametrize("unit", ["strict", "fast"])
def test_aov_kernels_present_spill_nothing_and_use_no_scratch_or_flat(unit):
    res, asm = _compile(unit)
    for suffix in INSTANCES:
        k = "kajo_aov_%s%s" % (unit, suffix)
        assert k in res, (k, sorted(res))
        r = res[k]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        # the sums are written with plain vector stores to global memory
        assert re.search(r"\n\s+global_store_dwordx4", body), k
    # EXACT handles run the STRICT instance: the EXACT unit has none of its own
    if unit == "strict":
        res_e, _ = _compile("exact")
        assert not [k for k in res_e if k.startswith("kajo_aov")]


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("gpus", ["2", "0"])
def test_driver_refuses_aov_on_more_than_one_gpu(tmp_path, gpus):
    """`kajo_render --aov` with any --gpus other than 1 (0 = every visible GPU) is refused at argument parsing, before a device is opened."""
    p = subprocess.run([BIN, "--aov", str(tmp_path / "x"), "--gpus", gpus, "-o", ""], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "--aov needs the whole frame on one GPU" in p.stderr, p.stderr
    assert not list(tmp_path.iterdir())
