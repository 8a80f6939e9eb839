"""tests/devicecode.py itself, without a compiler where none is needed: the remark parser on the remarks of a real hipcc run, the body
cut with both end markers, the compile line's lookup on a canned plan (a missing and an ambiguous source are refused), and that a unit
is compiled once."""
import pytest

import devicecode

# two functions of aux_kernels.hip as hipcc printed them (gfx950, -O3), the directory in front of the file name taken off
REMARKS = """clang++: warning: argument unused during compilation: '--hip-link' [-Wunused-command-line-argument]
kajo_amd/csrc/aux_kernels.hip:9:1: remark: Function Name: kajo_compose [-Rpass-analysis=kernel-resource-usage]
    9 | {
      | ^
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     TotalSGPRs: 19 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     VGPRs: 10 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:9:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark: Function Name: kajo_compose_aov [-Rpass-analysis=kernel-resource-usage]
   34 | {
      | ^
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     TotalSGPRs: 24 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     VGPRs: 16 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
kajo_amd/csrc/aux_kernels.hip:34:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
"""

LISTING = """\t.text
\t.globl\tkajo_a
\t.type\tkajo_a,@function
kajo_a:
; %bb.0:
\tv_add_f32 v0, v1, v2
\ts_cbranch_scc1 .LBB0_2
\ts_endpgm
.LBB0_2:
\tv_mul_f32 v0, v0, v0
\ts_endpgm
.Lfunc_end0:
\t.size\tkajo_a, .Lfunc_end0-kajo_a
\t.type\tnot_kajo_a,@function
not_kajo_a:
\tv_mov_b32 v0, 0
\ts_endpgm
.Lfunc_end1:
"""

PLAN = """mkdir -p build
hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -c /src/csrc/glare.hip -o /src/csrc/build/glare.o
hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -x hip -c /src/csrc/encode.cpp -o /src/csrc/build/encode.o
hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -x hip -c /src/csrc/encode_view.cpp -o /src/csrc/build/encode_view.o
hipcc -O3 --offload-arch=gfx950 -c /src/csrc/twice.hip -o /src/csrc/build/twice.o
hipcc -O3 --offload-arch=gfx950 -DTUNE -c /src/csrc/twice.hip -o /src/csrc/build_tune/twice.o
hipcc -shared -o libkajo_hip.so /src/csrc/build/glare.o /src/csrc/build/encode.o /src/csrc/linked_only.hip
"""


def test_parse_remarks_takes_every_numeric_key_of_every_function():
    res = devicecode.parse_remarks(REMARKS)
    common = {"AGPRs": 0, "ScratchSize": 0, "Occupancy": 8, "SGPRs Spill": 0, "VGPRs Spill": 0, "LDS Size": 0}
    assert res == {"kajo_compose": dict(common, TotalSGPRs=19, VGPRs=10), "kajo_compose_aov": dict(common, TotalSGPRs=24, VGPRs=16)}
    assert devicecode.parse_remarks("") == {}
    # a key in front of the first function belongs to none
    assert devicecode.parse_remarks("x.hip:1:1: remark:     VGPRs: 3 [-Rpass-analysis=kernel-resource-usage]\n") == {}


def test_body_ends_at_the_marker_the_caller_names():
    first = devicecode.body(LISTING, "kajo_a")
    assert first.startswith("\nkajo_a:") and first.count("v_add_f32") == 1 and "v_mul_f32" not in first and "s_endpgm" not in first
    whole = devicecode.body(LISTING, "kajo_a", end=".Lfunc_end")
    assert whole.count("s_endpgm") == 2 and "v_mul_f32" in whole and "not_kajo_a" not in whole
    # a label is looked for at the start of a line: kajo_a is not the tail of not_kajo_a
    assert "v_mov_b32" in devicecode.body(LISTING, "not_kajo_a") and "v_mov_b32" not in whole
    with pytest.raises(ValueError):
        devicecode.body(LISTING, "kajo_b")


def test_compile_command_is_the_one_compile_line_that_names_the_source():
    cmd = devicecode.compile_command("glare.hip", PLAN)
    assert cmd[0] == "hipcc" and cmd[cmd.index("-c") + 1] == "/src/csrc/glare.hip" and cmd[-1] == "/src/csrc/build/glare.o"
    # encode.cpp is not encode_view.cpp, and the other way round
    assert devicecode.compile_command("encode.cpp", PLAN)[-1].endswith("/encode.o")
    assert devicecode.compile_command("encode_view.cpp", PLAN)[-1].endswith("/encode_view.o")
    with pytest.raises(AssertionError, match="missing.hip: 0 compile lines"):
        devicecode.compile_command("missing.hip", PLAN)
    with pytest.raises(AssertionError, match="linked_only.hip: 0 compile lines"):  # (named by a link line only)
        devicecode.compile_command("linked_only.hip", PLAN)
    with pytest.raises(AssertionError, match="twice.hip: 2 compile lines.*-DTUNE"):
        devicecode.compile_command("twice.hip", PLAN)


def test_build_compiles_a_unit_once():
    first = devicecode.build("aux_kernels.hip")
    assert devicecode.build("aux_kernels.hip") is first
    assert "--offload-arch=gfx950" in first.cmd and "-c" in first.cmd and "-S" not in first.cmd  # the Makefile's own argv
    assert "kajo_compose" in first.resources and "\nkajo_compose:" in first.asm
    assert first.resources["kajo_compose"]["VGPRs"] > 0
