"""AOVs at the first non-delta hit (KAJO_FLAG_AOV_SPECULAR, include/kajo_hip.h under kajo_hip_read_aov) without a GPU: the flag as the
header and the binding declare it, the refusals that come before any device is opened, what the compiler made of the ten new kernel
instances (the budget of DESIGN.md 6d: nothing spilled, no scratch, no FLAT instruction, no atomic, at least 5 waves per SIMD), and the
definition's per-sample numpy replay (tests/aov_specular_replay.py, what tests/test_hip_aov_specular.py holds the kernels to) pinned
against the first-hit replay where the two must agree."""
import os
import re
import subprocess

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from oraclelib import OracleLib, available

import devicecode
from aov_specular_replay import describe, material_tables, replay_specular, without_delta
from framelib import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
INSTANCES = ("", "_big", "_big_lg", "_biglist", "_biglist_lg")
SEED = 0o715517


def test_header_and_binding_agree_on_the_flag():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    m = re.search(r"#define KAJO_FLAG_AOV_SPECULAR (\d+)u", header)
    assert m and int(m.group(1)) == capi.KAJO_FLAG_AOV_SPECULAR == 2048
    others = [int(v) for k, v in re.findall(r"#define (KAJO_FLAG_\w+) (\d+)u", header) if k != "KAJO_FLAG_AOV_SPECULAR"]
    assert capi.KAJO_FLAG_AOV in others and all(v & capi.KAJO_FLAG_AOV_SPECULAR == 0 for v in others), others
    m = re.search(r"#define KAJO_AOV_MAX_FOLLOW (\d+)", header)
    assert m and int(m.group(1)) == 8


def test_the_flag_alone_is_refused_before_any_device(scenes):
    sc = scenes["spheres_a1"]
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(sc, 64, 32, aov_specular=True)
    assert e.value.code == capi.KAJO_E_INVALID and "set the AOV flag with it" in str(e.value)
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(sc, 64, 32, flags=capi.KAJO_FLAG_AOV_SPECULAR)
    assert e.value.code == capi.KAJO_E_INVALID
    # on a tiled handle the pair is refused as KAJO_FLAG_AOV alone is
    with pytest.raises(capi.KajoError) as e:
        HipRenderer(sc, 64, 32, aov=True, aov_specular=True, tile_index=0, tile_count=2)
    assert e.value.code == capi.KAJO_E_INVALID and "tileCount 1" in str(e.value)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_refuses_the_modifier_alone(tmp_path):
    p = subprocess.run([BIN, "--aov-specular", "-o", str(tmp_path / "x.png")], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "--aov-specular" in p.stderr and "--aov" in p.stderr and "--denoise" in p.stderr, p.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("unit", ["strict", "fast"])
def test_new_instances_present_and_within_the_budget(unit):
    b = devicecode.build("kernel_%s.hip" % unit)
    res, asm = b.resources, b.asm
    for suffix in INSTANCES:
        k = "kajo_aov_%s_spec%s" % (unit, suffix)
        assert k in res, (k, sorted(res))
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        assert r["Occupancy"] >= 5, (k, r)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k
        assert re.search(r"\n\s+global_store_dwordx4", body), k
    if unit == "strict":  # EXACT handles run the STRICT instances
        res_e = devicecode.build("kernel_exact.hip").resources
        assert not [k for k in res_e if k.startswith("kajo_aov")]


@pytest.mark.skipif(not available("oracle"), reason="oracle/libkajo_oracle.so not built (run __graft_entry__.build())")
def test_replay_follows_the_mirror_and_the_glass_and_nothing_else(scenes):
    """spheres_a169, 48 x 32, S = 32 (25 samples), one pass. Measured: printed below (recorded in DESIGN.md 6d)."""
    sc = scenes["spheres_a169"]
    w, h, spp = 48, 32, 32
    lobe = material_tables(sc)[0]
    # the rule picks one plane by reflection (the mirror wall) and one sphere by transmission (the glass ball)
    assert sorted(lobe[lobe != 0].tolist()) == [2, 3] and (lobe[:sc.n_planes] == 2).sum() == 1 and (lobe[sc.n_planes:] == 3).sum() == 1
    A, B, stats = replay_specular(sc, [1], w, h, spp, SEED)
    print("spheres_a169 %dx%d S=%d:" % (w, h, spp), describe(stats))
    first = OracleLib("oracle").create(sc, 1).aov(w, h, spp, passes=1, seed=SEED, first_pass=1, threads=1)
    differs = (bits(A) != bits(first[0])).any(-1) | (bits(B) != bits(first[1])).any(-1)
    followed = stats["followed_per_pixel"] > 0
    assert differs.any() and followed.any() and not followed.all()
    # (a) bit for bit the first-hit sums wherever no sample met the mirror or the glass first
    assert not differs[~followed].any(), np.argwhere(differs & ~followed)[:4]
    assert 0 < stats["longest"] <= 8
    # (b) mirror and glass made diffuse: the first-hit sums everywhere
    plain = without_delta(sc)
    assert not material_tables(plain)[0].any()
    A, B, stats = replay_specular(plain, [1], w, h, spp, SEED)
    first = OracleLib("oracle").create(plain, 1).aov(w, h, spp, passes=1, seed=SEED, first_pass=1, threads=1)
    assert stats["follows"] == 0
    assert np.array_equal(bits(A), bits(first[0])) and np.array_equal(bits(B), bits(first[1]))
