"""What the compiler made of kajo_render_exact_simple (kajo_amd/csrc/kernel_exact_simple.cpp), checked without a GPU as
tests/test_kernel_resources_cpu.py checks kajo_render_exact, whose budgets it must keep: it is the kernel the benchmarked frame runs. It
exists to carry FEWER instructions than that kernel -- the loops for general sphere records and scaled planes are not compiled in -- so
the instruction budget is the point: measured 1959 static vector instructions against kajo_render_exact's 2278."""
import os
import re
import subprocess

import devicecode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
KERNEL = "kajo_render_exact_simple"
VALU_BUDGET = 2000


def _compile():
    b = devicecode.build("kernel_exact_simple.cpp")
    return b.resources, b.asm


def test_the_unit_holds_one_kernel_within_the_exact_kernels_budgets():
    res, asm = _compile()
    assert sorted(res) == [KERNEL], sorted(res)
    r = res[KERNEL]
    assert r["Occupancy"] == 5 and r["VGPRs"] <= 96 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["SGPRs Spill"] <= 10, r
    body = devicecode.body(asm, KERNEL)
    assert not re.search(r"\n\s+flat_(load|store|atomic)", body)
    assert "v_div_scale_f32" not in body and "v_div_fmas_f32" not in body and "v_div_fixup_f32" in body
    n = len(re.findall(r"\n\s+v_\w+", body))
    assert n <= VALU_BUDGET, "%d VALU instructions, budget %d" % (n, VALU_BUDGET)
    assert n >= 0.85 * VALU_BUDGET, "%d VALU instructions -- far below the budget %d: lower it to keep the guard tight" % (n, VALU_BUDGET)


def test_the_makefile_compiles_it_with_the_exact_units_flags():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all"], capture_output=True, text=True, check=True).stdout
    strip = lambda l, src, obj: [w for w in l.split() if w not in ("-x", "hip") and not w.endswith(src) and not w.endswith(obj)]
    exact = next(l for l in plan.splitlines() if l.startswith("hipcc") and l.rstrip().split()[-3].endswith("kernel_exact.hip"))
    simple = next(l for l in plan.splitlines() if l.startswith("hipcc") and "kernel_exact_simple.cpp" in l and " -c " in l)
    assert strip(exact, "kernel_exact.hip", "kernel_exact.o") == strip(simple, "kernel_exact_simple.cpp", "kernel_exact_simple.o")
    assert "-ffp-contract=off" in simple.split()
