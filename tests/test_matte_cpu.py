"""Object-coverage mattes (KAJO_FLAG_AOV_MATTE; include/kajo_hip.h kajo_hip_read_matte, kajo_hip_matte_mask) without a GPU: the flag and
the entry points as the header and the binding declare them, the refusals that come before a device is looked for, the driver's
refusals at argument parsing, what the compiler made of the kernels (matte.hip: nothing spilled, no scratch, no LDS, no FLAT
instruction, no atomic, 8 waves per SIMD; the twenty _matte instances of the AOV kernel: no vector register spilled, no scratch,
registers pinned), and the numpy restatement tests/test_hip_matte.py holds the kernels to (tests/matte_replay.py) on hand-made samples
and on the overflow fixture. The compile commands are the Makefile's own (`make -n`)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import stress_scene
from oraclelib import available

from matte_replay import mask_of, ranked, restate, tables
import devicecode
from devicecode import body as _body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
SEED = 0o715517
ENTRY_POINTS = ("kajo_hip_read_matte", "kajo_hip_matte_mask")
# matte.hip, kernel -> VGPRs as hipcc makes them, pinned to within VGPR_ROOM (8 waves per SIMD hold up to 64)
KERNELS = {"kajo_matte_rank": 37, "kajo_matte_mask": 31, "kajo_matte_dominant": 22}
VGPR_ROOM = 2
# The _matte instances of the AOV kernel: the VGPRs reached are the budget. The table is 16 registers held across
# the whole walk: each instance stands 16-19 above the one it is made from.
CLASSES = ("", "_big", "_big_lg", "_biglist", "_biglist_lg")
AOV_VGPRS = {
    "strict": {"_matte": (78, 91, 89, 79, 77), "_spec_matte": (90, 102, 100, 93, 90)},
    "fast": {"_matte": (70, 83, 81, 70, 68), "_spec_matte": (75, 91, 89, 78, 78)},
}


def test_header_and_binding_agree_on_the_flag():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    m = re.search(r"#define KAJO_FLAG_AOV_MATTE (\d+)u", header)
    assert m and int(m.group(1)) == capi.KAJO_FLAG_AOV_MATTE == 4096
    others = [int(v) for k, v in re.findall(r"#define (KAJO_FLAG_\w+) (\d+)u", header) if k != "KAJO_FLAG_AOV_MATTE"]
    assert capi.KAJO_FLAG_AOV in others and all(v & capi.KAJO_FLAG_AOV_MATTE == 0 for v in others), others
    m = re.search(r"#define KAJO_MATTE_SLOTS (\d+)", header)
    assert m and int(m.group(1)) == capi.KAJO_MATTE_SLOTS == 8
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(kajo_hip_t h" % name, header), name
        assert name in capi.EXPORTS
    assert b"aov-matte" in capi.lib().kajo_hip_version()


def test_prototypes_load_and_null_handles_are_refused():
    L = capi.lib()
    assert L.kajo_hip_read_matte.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    assert L.kajo_hip_matte_mask.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.kajo_hip_read_matte(None, None, None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_last_error() == b"null handle"
    objects = (C.c_int32 * 2)(1, 2)
    assert L.kajo_hip_matte_mask(None, objects, 2, None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_last_error() == b"null handle"
    assert L.kajo_hip_matte_mask(None, None, 0, None, None) == capi.KAJO_E_INVALID
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        assert os.path.exists(lib), lib
        nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in ENTRY_POINTS + ("kajo_matte_rank_launch", "kajo_matte_mask_launch"):
            assert re.search(r"\bT %s\b" % name, nm), (lib, name)


def test_the_flag_alone_is_refused_before_any_device(scenes):
    sc = scenes["spheres_a1"]
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(sc, 64, 32, matte=True)
    assert e.value.code == capi.KAJO_E_INVALID and "set the AOV flag with it" in str(e.value) and "matte" in str(e.value)
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(sc, 64, 32, flags=capi.KAJO_FLAG_AOV_MATTE)
    assert e.value.code == capi.KAJO_E_INVALID
    with pytest.raises(capi.KajoError) as e:  # (the chain's flag does not stand in for the AOV flag)
        HipRenderer(sc, 64, 32, flags=capi.KAJO_FLAG_AOV_MATTE | capi.KAJO_FLAG_AOV_SPECULAR)
    assert e.value.code == capi.KAJO_E_INVALID
    # on a tiled handle the pair is refused as KAJO_FLAG_AOV alone is
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(sc, 64, 32, aov=True, matte=True, tile_index=0, tile_count=2)
    assert e.value.code == capi.KAJO_E_INVALID and "tileCount 1" in str(e.value)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--matte-mask", "m.pfm", "--matte-objects", "3,4", "--gpus", "2"], "--matte-mask needs the whole frame on one GPU (--gpus 1, without --three-arg)"),
    (["--matte-mask", "m.pfm", "--matte-objects", "3,4", "--gpus", "0"], "--matte-mask needs the whole frame on one GPU (--gpus 1, without --three-arg)"),
    (["--matte-ids", "i.pfm", "--gpus", "2"], "--matte-ids needs the whole frame on one GPU (--gpus 1, without --three-arg)"),
    (["--matte-ids", "i.pfm", "--gpus", "0"], "--matte-ids needs the whole frame on one GPU (--gpus 1, without --three-arg)"),
    (["--matte-ids", "i.pfm", "--three-arg"], "--matte-ids needs the whole frame on one GPU"),
    (["--matte-mask", "m.pfm", "--matte-objects", "3,,4"], "--matte-objects must be a comma-separated list"),
    (["--matte-mask", "m.pfm", "--matte-objects", "3,4,"], "--matte-objects must be a comma-separated list"),
    (["--matte-mask", "m.pfm", "--matte-objects", "3;4"], "--matte-objects must be a comma-separated list"),
    (["--matte-mask", "m.pfm", "--matte-objects", "-3"], "--matte-objects must be a comma-separated list"),
    (["--matte-mask", "m.pfm", "--matte-objects", "seven"], "--matte-objects must be a comma-separated list"),
    (["--matte-mask", "m.pfm", "--matte-objects", "1.5"], "--matte-objects must be a comma-separated list"),
    (["--matte-mask", "m.pfm", "--matte-objects", ""], "--matte-objects must be a comma-separated list"),
    (["--matte-mask", "m.pfm"], "give the two together"),
    (["--matte-objects", "3,4"], "give the two together"),
])
def test_driver_refuses_at_argument_parsing(tmp_path, args, message):
    p = subprocess.run([BIN, *args, "-o", "o.png"], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_matte_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--matte-mask FILE", "--matte-objects LIST", "--matte-ids FILE", "matte_dropped_pixels"):
        assert opt in text, opt


def _compile_matte():
    b = devicecode.build("matte.hip")
    assert "-ffp-contract=off" in b.cmd and "--offload-arch=gfx950" in b.cmd
    return b.resources, b.asm


def _compile_unit(unit):
    b = devicecode.build("kernel_%s.hip" % unit)
    return b.resources, b.asm


def test_matte_kernels_spill_nothing_and_use_no_scratch_lds_flat_or_atomics():
    res, asm = _compile_matte()
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k, vgprs in KERNELS.items():
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["LDS Size"] == 0, (k, r)
        assert abs(r["VGPRs"] - vgprs) <= VGPR_ROOM and r["Occupancy"] == 8, (k, r)
        body = _body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+ds_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k
        # a pixel's table is read in 16-byte words (the compiler may cut one into 12 + 4), the bitset one word at a time; rank writes the
        # table back as four 16-byte stores, mask and dominant one word per pixel
        loads = set(re.findall(r"\n\s+(global_load_\w+)", body))
        assert "global_load_dwordx4" in loads and loads <= {"global_load_dword", "global_load_dwordx3", "global_load_dwordx4"}, (k, loads)
        stores = re.findall(r"\n\s+(global_store_\w+)", body)
        assert stores == (["global_store_dwordx4"] * 4 if k == "kajo_matte_rank" else ["global_store_dword"]), (k, stores)
    # one division per pixel, in mask alone (the IEEE quotient: the fixup ends it)
    assert len(re.findall(r"v_div_fixup_f32", _body(asm, "kajo_matte_mask"))) == 1
    assert "v_div_fixup_f32" not in _body(asm, "kajo_matte_rank") and "v_div_fixup_f32" not in _body(asm, "kajo_matte_dominant")


def test_makefile_links_the_matte_kernels_into_the_product_and_the_tools_twin():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("matte.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "matte.hip" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0], compiles


@pytest.mark.parametrize("unit", ["strict", "fast"])
def test_matte_instances_of_the_aov_kernel_spill_no_vector_register_and_use_no_scratch(unit):
    res, asm = _compile_unit(unit)
    for kind, budget in AOV_VGPRS[unit].items():
        for cls, vgprs in zip(CLASSES, budget):
            k = "kajo_aov_%s%s%s" % (unit, kind, cls)
            assert k in res, (k, sorted(res))
            r = res[k]
            print(k, r)
            assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
            assert r["VGPRs"] <= vgprs, (k, r)
            assert r["VGPRs"] >= vgprs - 8, "%s: %d VGPRs, far below the budget %d: lower it to keep the guard tight" % (k, r["VGPRs"], vgprs)
            body = _body(asm, k)
            assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
            assert not re.search(r"\n\s+scratch_\w+", body), k
            assert not re.search(r"\n\s+\w*atomic\w*", body), k
            # A, B and the table's four words of 16 bytes: read before the sample loop, written after it
            assert len(re.findall(r"\n\s+global_store_dwordx4", body)) == 6, k
    if unit == "strict":  # EXACT handles run the STRICT instances
        res_e, _ = _compile_unit("exact")
        assert not [k for k in res_e if k.startswith("kajo_aov")]


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------

def test_restatement_first_come_rule_rank_and_mask_on_hand_made_samples():
    # pixel 0: ten ids in a row, the ninth and tenth are dropped, later repeats of held ids still count; pixel 1: one id; pixel 2: the
    # background (id 0) is an id like any other, and ties
    seq = np.array([[5, 7, 0], [3, 7, 4], [9, 7, 0], [1, 7, 4], [2, 7, 2], [8, 7, 2], [6, 7, 9], [4, 7, 9], [11, 7, 9], [12, 7, 9], [5, 7, 0],
                    [11, 7, 0], [4, 7, 0]], np.int32)
    slot, count, dropped = tables(seq)
    assert slot[0].tolist() == [5, 3, 9, 1, 2, 8, 6, 4] and count[0].tolist() == [2, 1, 1, 1, 1, 1, 1, 2] and dropped[0] == 3
    assert slot[1].tolist() == [7] + [-1] * 7 and count[1].tolist() == [13] + [0] * 7 and dropped[1] == 0
    assert slot[2].tolist() == [0, 4, 2, 9] + [-1] * 4 and count[2].tolist() == [5, 2, 2, 4, 0, 0, 0, 0] and dropped[2] == 0
    assert ((count.sum(1) + dropped) == len(seq)).all()
    ids, counts = ranked(slot, count)
    assert ids.dtype == np.int32 and counts.dtype == np.uint32
    assert ids[0].tolist() == [4, 5, 1, 2, 3, 6, 8, 9] and counts[0].tolist() == [2, 2, 1, 1, 1, 1, 1, 1]
    assert ids[1].tolist() == [7] + [-1] * 7 and counts[1].tolist() == [13] + [0] * 7
    assert ids[2].tolist() == [0, 9, 2, 4, -1, -1, -1, -1] and counts[2].tolist() == [5, 4, 2, 2, 0, 0, 0, 0]
    m = mask_of(ids, counts, len(seq), [0, 2, 5, 5])
    assert m.dtype == np.float32 and m.tolist() == [np.float32(3) / np.float32(13), 0.0, np.float32(7) / np.float32(13)]
    assert mask_of(ids, counts, 0, [7]).tolist() == [0.0, 0.0, 0.0]
    assert mask_of(ids, counts, len(seq), []).tolist() == [0.0, 0.0, 0.0]


OVERFLOW = dict(w=24, h=16, spp=32, passes=(1, 2))  # tests/test_hip_matte.py's overflow case


@pytest.mark.skipif(not available("oracle"), reason="oracle/libkajo_oracle.so not built (run __graft_entry__.build())")
def test_the_overflow_fixture_overflows_by_the_oracle_alone(scenes):
    """The 1000-sphere grid scene at 24 x 16, 25 samples x 2 passes: by the oracle's trace alone some pixels see more than eight objects.
    Measured: 34 pixels of 384, up to 16 ids in one."""
    sc = stress_scene(scenes["spheres_a169"], 1000, 16)
    r = restate(sc, OVERFLOW["passes"], OVERFLOW["w"], OVERFLOW["h"], OVERFLOW["spp"], SEED)
    over = r["distinct"] > 8
    print("overflow fixture: %d pixels of %d see more than 8 ids, the most %d; %d samples dropped" %
          (over.sum(), over.size, r["distinct"].max(), r["dropped"].sum()))
    assert over.any() and r["samples"] == 50
    assert ((r["dropped"] > 0) == over).all()  # (a sample is dropped exactly where a ninth id arrives)
    assert (r["counts"].sum(-1, dtype=np.int64) + r["dropped"] == r["samples"]).all()
    assert (r["counts"][over] > 0).all()  # every slot of a full table holds something
