"""Tiled AOVs (KAJO_FLAG_AOV_TILED, include/kajo_hip.h kajo_hip_compose_aov) without a GPU: the flag and the entry points as the header
declares them, the refusals that come before any device is opened, the driver's option checking, and what the compiler made of the AOV
kernels now that the tiled launch shape is an argument of the twenty existing instances: nothing spilled to scratch, and no instance
with more vector registers than before the shape was added (tests/golden/aov_kernel_vgprs.json: the figures of the commit before)."""
import json
import os
import re
import subprocess

import pytest

import devicecode
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
CLASSES = ("", "_big", "_big_lg", "_biglist", "_biglist_lg")
VARIANTS = ("", "_spec", "_matte", "_spec_matte")
NEEDS_ONE_GPU = "needs the whole frame on one GPU"


def test_the_flag_has_a_bit_of_its_own():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"#define (KAJO_FLAG_\w+) (\d+)u", header)}
    assert flags["KAJO_FLAG_AOV_TILED"] == capi.KAJO_FLAG_AOV_TILED == 8192
    assert all(v & 8192 == 0 for k, v in flags.items() if k != "KAJO_FLAG_AOV_TILED"), flags
    assert "kajo_hip_aov_tile_buffers" in capi.EXPORTS and "kajo_hip_compose_aov" in capi.EXPORTS


def test_the_flag_alone_is_refused_before_a_device_is_looked_for(scenes):
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(scenes["spheres_a1"], 64, 32, aov_tiled=True)
    assert e.value.code == capi.KAJO_E_INVALID and "AOV flag" in str(e.value)


def test_the_flag_lifts_the_one_owner_refusal(scenes):
    """With the flag, aov on two owners gets past every check of the parameters: without a GPU it ends at the device (with one, it is
    created)."""
    for kw in (dict(), dict(aov_specular=True), dict(matte=True), dict(matte=True, aov_specular=True)):
        try:
            HipRenderer(scenes["spheres_a1"], 64, 32, aov=True, aov_tiled=True, tile_index=1, tile_count=2, **kw).close()
        except capi.KajoError as e:
            assert e.code == capi.KAJO_E_NO_DEVICE and "tileCount 1" not in str(e)


def test_library_exports_the_entry_points_and_refuses_null_handles():
    L = capi.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT kajo_hip_aov_tile_buffers\b", nm) and re.search(r"\bT kajo_hip_compose_aov\b", nm)
    assert L.kajo_hip_aov_tile_buffers(None, None, None, None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_compose_aov(None, None, None) == capi.KAJO_E_INVALID


def _driver(tmp_path, scenes, args):
    pod = str(tmp_path / "scene.pod")
    if not os.path.exists(pod):
        scenes["spheres_a1"].write_pod(pod)
    return subprocess.run([BIN, "-w", "64", "-h", "32", "--passes", "1", "--spp", "4", "--scene-pod", pod, "-o", ""] + args, capture_output=True,
                          text=True, timeout=120)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_refuses_the_switch_alone(tmp_path, scenes):
    p = _driver(tmp_path, scenes, ["--aov-tiled"])
    assert p.returncode == 1 and "--aov-tiled changes where the AOVs" in p.stderr, p.stderr
    p = _driver(tmp_path, scenes, ["--aov-tiled", "--gpus", "2", "--aov", str(tmp_path / "x"), "--three-arg"])
    assert p.returncode == 1 and "--aov needs the whole frame on one GPU (--gpus 1, without --three-arg)" in p.stderr, p.stderr


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("option", ["aov", "denoise", "matte-ids", "matte-mask"])
def test_driver_takes_the_options_on_two_gpus_with_the_switch(tmp_path, scenes, option):
    """Past option checking: what is left to fail, where no GPU is visible, is the device."""
    args = ["--" + option, str(tmp_path / "out"), "--gpus", "2"] + (["--matte-objects", "3,4"] if option == "matte-mask" else [])
    p = _driver(tmp_path, scenes, args)
    assert p.returncode == 1 and NEEDS_ONE_GPU in p.stderr, p.stderr  # (without the switch: what it was)
    p = _driver(tmp_path, scenes, args + ["--aov-tiled", "--same-device"])
    assert NEEDS_ONE_GPU not in p.stderr, p.stderr
    # (2: the backend's exception for want of a device, where no GPU is visible)
    assert p.returncode == 0 or (p.returncode == 2 and "no HIP device available" in p.stderr), p.stderr


@pytest.mark.parametrize("unit", ["strict", "fast"])
def test_aov_kernels_spill_nothing_and_take_no_more_registers_than_before(unit):
    """The tiled shape is a run-time argument of the existing instances, which are every AOV kernel the library can launch: none uses
    scratch or spills a vector register, and none has more VGPRs than before the argument was added."""
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "aov_kernel_vgprs.json")))
    res = devicecode.build("kernel_%s.hip" % unit).resources
    names = ["kajo_aov_%s%s%s" % (unit, v, c) for v in VARIANTS for c in CLASSES]
    assert sorted(k for k in res if k.startswith("kajo_aov_")) == sorted(names)
    for k in names:
        r = res[k]
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        assert r["VGPRs"] <= before[k], (k, r["VGPRs"], before[k])
