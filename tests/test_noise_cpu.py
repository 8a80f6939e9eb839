"""The noise estimate (include/kajo_hip.h "The noise estimate", kajo_amd/csrc/noise.hip) without a GPU: the structs, constants and entry
points as the header declares them, in the product and the tools' twin; every refusal that comes before a handle or a device is looked
for; the pure host half, kajo_hip_noise_evaluate, against a numpy quantile of hand-made histograms; what the compiler made of the two
kernels (nothing spilled, no scratch, no FLAT access, 16-byte loads, the moments summed without a fused multiply-add); that the
device code of every kernel from before is what it was, function by function, against digests recorded from the parent commit; that the
kernels live in a translation unit of their own, which no other unit includes; the driver's refusals; and the DEFINITION against the
CPU oracle: over K seeds the variance the estimate predicts for the mean must be the variance the means show."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import devicecode
from kajo_amd import capi
from kajo_amd.renderer import noise_evaluate
from oraclelib import OracleLib, available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
ENTRY_POINTS = ("kajo_hip_default_noise_params", "kajo_hip_noise_evaluate", "kajo_hip_noise", "kajo_hip_read_noise_moments")
KERNELS = ("kajo_noise_update", "kajo_noise_map")
BINS, WORDS, BASE = 514, 516, (127 - 16) << 4
F32, F64 = np.float32, np.float64


def _header():
    return open(os.path.join(ROOT, "include", "kajo_hip.h")).read()


def test_header_structs_constants_binding_and_libraries_agree():
    header = _header()
    sizes = {"KajoNoiseParams": 8, "KajoNoiseMoments": 32, "KajoNoiseResult": 48}
    for name, size in sizes.items():
        cls = getattr(capi, name)
        assert C.sizeof(cls) == size, name
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        names = [n for line in re.findall(r"^\s+\w+ ([\w, \[\]]+);", fields, re.M) for n in re.sub(r"\[\d+\]", "", line).split(", ")]
        assert names == [f for f, _ in cls._fields_], (name, names)
    assert capi.KajoNoiseResult.quantileValue.offset == 32 and capi.KajoNoiseMoments.n.offset == 16
    assert re.search(r"#define KAJO_FLAG_NOISE 16384u", header) and capi.KAJO_FLAG_NOISE == 16384
    assert re.search(r"#define KAJO_NOISE_BATCH_PASSES 4\b", header) and capi.KAJO_NOISE_BATCH_PASSES == 4
    assert re.search(r"#define KAJO_NOISE_HIST_WORDS 516\b", header) and capi.KAJO_NOISE_HIST_WORDS == WORDS == capi.KAJO_METER_BINS + 2
    assert re.search(r"#define KAJO_GROUP_PASSES 4\b", open(os.path.join(CSRC, "render_args.h")).read())
    # the next free bit: no other flag has it
    flags = {k: v for k, v in vars(capi).items() if k.startswith("KAJO_FLAG_") and v}
    assert [k for k, v in flags.items() if v & 16384] == ["KAJO_FLAG_NOISE"]
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    # the product always; the tools' twin where it is built, as the other stages' tests have it
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        if lib != capi.LIB_PATH and not os.path.exists(lib):
            continue
        nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in ENTRY_POINTS + ("kajo_noise_update_launch", "kajo_noise_map_launch"):
            assert re.search(r"\bT %s\b" % name, nm), (lib, name)


def test_default_params_are_the_documented_ones():
    L = capi.lib()
    p = capi.KajoNoiseParams(7.0, 0.1)
    L.kajo_hip_default_noise_params(C.byref(p))
    assert F32(p.floor) == F32(1e-2) and F32(p.quantile) == F32(0.95)
    L.kajo_hip_default_noise_params(None)  # accepted
    for text in ("(default 1e-2)", "(default 0.95)"):
        assert text in _header(), text


def _noise(L, params, handle=None):
    r = capi.KajoNoiseResult()
    rc = L.kajo_hip_noise(handle, None if params is None else C.byref(params), None, None, None, None, None, C.byref(r))
    return rc, L.kajo_hip_last_error().decode()


@pytest.mark.parametrize("floor,quantile,word", [
    (0.0, 0.95, "floor"), (-1e-2, 0.95, "floor"), (float("inf"), 0.95, "floor"), (float("nan"), 0.95, "floor"),
    (1e-2, 0.0, "quantile"), (1e-2, -0.5, "quantile"), (1e-2, 1.0001, "quantile"), (1e-2, float("nan"), "quantile"), (1e-2, float("inf"), "quantile"),
])
def test_bad_parameters_are_refused_before_a_handle_or_a_device_is_looked_for(floor, quantile, word):
    L = capi.lib()
    rc, msg = _noise(L, capi.KajoNoiseParams(floor, quantile))
    assert rc == capi.KAJO_E_INVALID and word in msg and "noise" in msg, (rc, msg)
    if word == "quantile":
        value = C.c_float(5.0)
        rc = L.kajo_hip_noise_evaluate(np.zeros(WORDS, np.uint32).ctypes.data_as(C.c_void_p), quantile, C.byref(value))
        assert rc == capi.KAJO_E_INVALID and "quantile" in L.kajo_hip_last_error().decode() and value.value == 5.0


def test_null_arguments_and_good_parameters_reach_the_handle_check():
    L = capi.lib()
    assert _noise(L, None) == (capi.KAJO_E_INVALID, "null noise parameters")
    for p in (capi.KajoNoiseParams(1e-2, 0.95), capi.KajoNoiseParams(1e-30, 1.0), capi.KajoNoiseParams(1e30, 2.0 ** -24)):
        assert _noise(L, p) == (capi.KAJO_E_INVALID, "null handle")
    assert L.kajo_hip_read_noise_moments(None, None) == capi.KAJO_E_INVALID
    value = C.c_float()
    hist = np.zeros(WORDS, np.uint32)
    assert L.kajo_hip_noise_evaluate(None, 0.5, C.byref(value)) == capi.KAJO_E_INVALID
    assert L.kajo_hip_noise_evaluate(hist.ctypes.data_as(C.c_void_p), 0.5, None) == capi.KAJO_E_INVALID
    with pytest.raises(ValueError):
        noise_evaluate(np.zeros(BINS, np.uint32))


def edge(b):
    """lower edge of bin b = 1..513: the float with the bits (b - 1 + base) << 19"""
    return np.array([(b - 1 + BASE) << 19], np.uint32).view(F32)[0]


def centre(b):
    if b == 0:
        return F32(2.0 ** -17)
    return edge(513) if b >= 513 else F32((F64(edge(b)) + F64(edge(b + 1))) / F64(2))


def bin_of(rel32):
    k = (np.asarray(rel32, F32).view(np.uint32) & 0x7fffffff) >> 19
    return np.where(k < BASE, 0, np.minimum(k.astype(np.int64) - BASE + 1, BINS - 1))


def quantile_of_pixels(rel32, q):
    """numpy's own quantile of the known pixels' relative errors -- the r-th smallest, r = ceil(q n) -- as the centre of its bin"""
    known = np.sort(rel32[rel32 >= 0])
    if not known.size:
        return F32(-1)
    r = min(known.size, max(1, int(np.ceil(F64(F32(q)) * known.size))))
    assert known[r - 1] == np.quantile(known, F64(F32(q)), method="inverted_cdf")
    return centre(int(bin_of(known[r - 1])))


def hist_of(rel32, bad=0):
    h = np.zeros(WORDS, np.uint32)
    h[:BINS] = np.bincount(bin_of(rel32[rel32 >= 0]), minlength=BINS)
    h[BINS] = (rel32 < 0).sum()
    h[BINS + 1] = bad
    return h


def test_evaluate_hand_made_histograms_against_numpy():
    assert noise_evaluate(np.zeros(WORDS, np.uint32), 0.95) == -1.0  # empty
    unknown = hist_of(np.full(100, -1, F32), bad=7)  # all unknown: the two counters behind the bins are not pixels with a value
    assert unknown[BINS] == 100 and noise_evaluate(unknown, 0.5) == -1.0
    one = hist_of(np.full(12, 0.03, F32))  # one bin
    for q in (2.0 ** -24, 0.5, 1.0):
        assert noise_evaluate(one, q) == centre(int(bin_of(F32(0.03)))) == quantile_of_pixels(np.full(12, 0.03, F32), q)
    zero = hist_of(np.zeros(5, F32))  # converged to the bit: bin 0 counts among the known, unlike the meter's black
    assert zero[0] == 5 and noise_evaluate(zero, 0.95) == F32(2.0 ** -17)
    assert noise_evaluate(hist_of(np.array([np.inf, 1e9], F32)), 1.0) == F32(65536.0)  # bin 513
    # ties at a bin edge: the edge itself belongs to the upper bin, the float below it to the lower one
    e = edge(200)
    below = np.nextafter(e, F32(0))
    rel = np.array([below] * 10 + [e] * 10, F32)
    h = hist_of(rel)
    assert h[199] == 10 and h[200] == 10
    for q in (0.5, float(F32(0.5) + F32(2.0 ** -24)), 0.05, 0.55, 1.0):
        assert noise_evaluate(h, q) == quantile_of_pixels(rel, q), q
    assert noise_evaluate(h, 0.5) == centre(199) and noise_evaluate(h, 0.55) == centre(200)
    # unknown pixels beside known ones do not move the quantile
    h2 = h.copy()
    h2[BINS], h2[BINS + 1] = 1000, 3
    assert noise_evaluate(h2, 0.5) == noise_evaluate(h, 0.5)
    rng = np.random.default_rng(516)
    for _ in range(100):
        rel = (10.0 ** rng.uniform(-7, 1, int(rng.integers(1, 400)))).astype(F32)
        rel[rng.random(rel.size) < 0.2] = -1
        q = float(F32(rng.uniform(1e-6, 1.0)))
        assert noise_evaluate(hist_of(rel), q) == quantile_of_pixels(rel, q)
    # the owners' histograms add word by word
    a, b = rel[: rel.size // 2], rel[rel.size // 2:]
    assert np.array_equal(hist_of(a) + hist_of(b), hist_of(rel))
    assert noise_evaluate(np.full(WORDS, 0xffffffff, np.uint32), 0.5) == centre(256)  # sums beyond 32 bits


def _compile():
    b = devicecode.build("noise.hip")
    assert "-ffp-contract=off" in b.cmd and "--offload-arch=gfx950" in b.cmd
    return b.resources, b.asm


def test_noise_kernels_spill_nothing_and_use_no_scratch_or_flat_access():
    res, asm = _compile()
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k in KERNELS:
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["Occupancy"] == 8, (k, r)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        loads = re.findall(r"\n\s+(global_load_\w+)", body)
        stores = re.findall(r"\n\s+(global_store_\w+)", body)
        atomics = set(re.findall(r"\n\s+(\w*atomic\w*)", body))
        if k == "kajo_noise_update":
            # a slot: T (its three colour words, or the float4), the baseline and the record's two halves in, the record and T out; no
            # atomics, no LDS, no cross-lane operation; s2 takes one multiply and one add
            assert r["LDS Size"] == 0 and not atomics, (r, atomics)
            assert sorted(loads) in (["global_load_dwordx3"] + ["global_load_dwordx4"] * 3, ["global_load_dwordx4"] * 4), loads
            assert stores == ["global_store_dwordx4"] * 3, stores
            assert not re.search(r"\n\s+(ds_|v_readlane|v_readfirstlane|v_permlane|v_mov_b32_dpp|s_barrier)\w*", body), k
            assert "v_mul_f64" in body and "v_add_f64" in body and not re.search(r"\n\s+v_fma\w*_f64", body), k
        else:
            # the record's two halves in; four planes out, a word per lane; the workgroup's 516 counters in LDS, flushed with integer adds
            assert r["LDS Size"] == WORDS * 4, r
            assert loads == ["global_load_dwordx4"] * 2 and stores == ["global_store_dword"] * 4, (loads, stores)
            assert atomics == {"global_atomic_add"} and "ds_add_u32" in body and "ds_add_rtn" not in body, atomics


def test_the_device_code_of_every_kernel_from_before_is_unchanged_function_by_function():
    """tests/golden/kernel_digests_before_noise.json: a SHA-256 per function of every device unit, recorded from the commit in front of the
    noise estimate (tools/kernel_digests.py: the Makefile's own commands, -S --cuda-device-only; a function is its label to its .Lfunc_end,
    comments dropped). The working tree, compiled the same way, must give the same functions with the same digests in the same units, and
    one unit more, noise, with the two kernels and nothing else. A shared header (render_args.h, device_scene.h), a flag of the Makefile or
    a source that moved a kernel shows here, whatever its text looks like."""
    devicecode.need_tools()
    tool = devicecode.digest_tool()
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_digests_before_noise.json")))
    before = recorded["units"]
    assert sorted(before) == sorted(["kernel_fast", "kernel_exact", "kernel_strict", "aux_kernels", "denoise", "glare", "despeckle", "meter", "local",
                                     "lens", "view", "matte", "grade"])
    assert sum(len(f) for f in before.values()) > 100 and all(re.fullmatch(r"[0-9a-f]{64}", d) for f in before.values() for d in f.values())
    now = devicecode.digests_now()
    assert sorted(now) == sorted(list(before) + ["noise"]), sorted(now)
    assert sorted(now.pop("noise")) == sorted(KERNELS)
    where = "(recorded with %s; this is %s)" % (recorded["compiler"], tool.compiler())
    for unit in before:
        assert sorted(now[unit]) == sorted(before[unit]), (unit, sorted(set(now[unit]) ^ set(before[unit])), where)
        moved = [f for f in before[unit] if now[unit][f] != before[unit][f]]
        assert not moved, (unit, moved, where)
    # the comparison can fail: another register in one instruction is another digest, a comment or a renumbered local label is not
    text = "\t.type\tk,@function\nk:\n; %bb.0:\n\tv_add_f32 v0, v1, v2 ; note\n.LBB7_1:\n\ts_cbranch_scc1 .LBB7_1\n\ts_endpgm\n.Lfunc_end7:\n"
    same = text.replace("LBB7", "LBB9").replace("; note", "").replace("; %bb.0:\n", "")
    assert tool.functions(text) == tool.functions(same) == {"k": "k:\nv_add_f32 v0, v1, v2\n.LBB_1:\ns_cbranch_scc1 .LBB_1\ns_endpgm"}
    assert tool.functions(text.replace("v1, v2", "v1, v3")) != tool.functions(text)


def test_the_kernels_live_in_a_unit_of_their_own_which_every_numerics_build_links():
    """No render, AOV or display source names them, and no other unit's compile line names the new one (that their device code is what it was is
    the test above)."""
    # (launch_plan.h: host arithmetic which no device source includes -- asserted below; kajo_hip_create's validation, which it holds, names
    # the flag in the refusal of the adaptive flag without it, as capi.cpp did while the validation was there)
    host_only = {"launch_plan.h": ("handle.h",), "handle.h": ("capi.cpp", "present.cpp")}
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".h", ".cpp")):
            text = open(os.path.join(CSRC, name)).read()
            for header, users in host_only.items():
                assert ('#include "%s"' % header in text) == (name in users), (name, header)
        if name.endswith((".hip", ".h")) and name != "noise.hip":
            text = open(os.path.join(CSRC, name)).read()
            assert not re.search(r'#include\s+"noise\.hip"', text) and "kajo_noise" not in text, name
            assert "KAJO_FLAG_NOISE" not in text or name == "launch_plan.h", name
    text = open(os.path.join(CSRC, "noise.hip")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["render_args.h"]
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("noise.o" in l and "meter.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "/noise.hip" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0], compiles
    # every other device unit is compiled by the command it had: none names the new one
    for l in plan.splitlines():
        if l.startswith("hipcc") and " -c " in l and "/noise.hip" not in l:
            assert not re.search(r"\bnoise\b", l), l


# ---- the definition against the oracle -----------------------------------------------------------------------------------------------
# spheres_a169 at 32 x 24, S = 4, 64 passes = 16 batches, K seeds. Per seed the estimate gives every pixel a mean m and a predicted
# variance of that mean, se^2; over the seeds the means have a variance of their own.
#   R = (sum over pixels of the mean over seeds of se^2) / (sum over pixels of the variance over seeds of m)
# is 1 for a right estimate; a missing / n, / 16 or n - 1 -> n moves it by 16x, 16x and 1.07x (the last is inside the band: the band is
# for the definition's structure). K: the denominator is a sample variance of K means, relative error about sqrt(2 / (K - 1)) a pixel,
# and the sum is led by the few pixels that see the light through the glass; measured with the oracle K = 16: 1.120, 32: 1.127, 64:
# 1.070, 128: 1.017. K = 64 keeps the oracle's own R inside [0.8, 1.25] with room, in 3 s.
K_SEEDS = 64


def oracle_moments(handle, W, H, S, batches, seed):
    acc = np.zeros((H, W, 4), F32)
    base = np.zeros_like(acc)
    n, s1, s2 = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for b in range(batches):
        handle.render(W, H, S=S, passes=4, seed=seed, first_pass=4 * b + 1, accum=acc)
        D = acc - base
        y = F32(0.2126) * D[..., 0] + F32(0.7152) * D[..., 1] + F32(0.0722) * D[..., 2]
        ok = np.isfinite(y)
        d = np.where(ok, y.astype(F64), 0.0)
        n, s1, s2 = n + ok, s1 + d, s2 + d * d
        base = acc.copy()
    return n, s1, s2


@pytest.mark.skipif(not available("oracle"), reason="oracle not built")
def test_the_predicted_variance_is_the_variance_of_the_means_over_seeds(scenes):
    handle = OracleLib("oracle").create(scenes["spheres_a169"], 1)
    W, H = 32, 24
    ms, se2 = [], []
    for k in range(K_SEEDS):
        n, s1, s2 = oracle_moments(handle, W, H, 4, 16, 236367 + 1000 * k)
        assert (n == 16).all()
        ms.append(s1 / (4 * n))
        v = np.maximum(s2 - s1 * s1 / n, 0.0) / (n - 1)
        se2.append(v / n / 16)
    R = np.mean(se2, 0).sum() / np.var(ms, 0, ddof=1).sum()
    print("R = %.4f over %d seeds" % (R, K_SEEDS))
    assert 0.8 <= R <= 1.25, R  # (the oracle's own: K is large enough)
    assert 0.5 <= R <= 2.0, R   # the condition on the definition
    # the evaluation's own restatement gives the same se: sqrt(v / n) / 4
    assert np.allclose(np.sqrt(se2[-1]), np.sqrt(v / n) / 4, rtol=1e-14)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--until-noise", "-0.1"], "--until-noise must be a finite number >= 0"),
    (["--until-noise", "nan"], "--until-noise must be a finite number >= 0"),
    (["--until-noise", "low"], "--until-noise must be a finite number >= 0"),
    (["--until-noise", "0.05", "--noise-quantile", "0"], "--noise-quantile must be a quantile in (0, 1]"),
    (["--until-noise", "0.05", "--noise-quantile", "1.5"], "--noise-quantile must be a quantile in (0, 1]"),
    (["--noise-map", "n.pfm", "--noise-floor", "0"], "--noise-floor must be a finite number > 0"),
    (["--until-noise", "0.05", "--noise-floor", "inf"], "--noise-floor must be a finite number > 0"),
    (["--until-noise", "0.05", "--max-passes", "0"], "--max-passes must be a whole number >= 1"),
    (["--until-noise", "0.05", "--max-passes", "6.5"], "--max-passes must be a whole number >= 1"),
    (["--noise-map", "n.pfm", "--max-passes", "64"], "--max-passes must be a whole number >= 1, with --until-noise"),
    (["--max-passes", "64"], "give them with one of the two"),
    (["--noise-quantile", "0.9"], "give them with one of the two"),
    (["--until-noise", "0.05", "--three-arg"], "the noise options need the backend's options"),
])
def test_driver_refuses_bad_noise_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_noise_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--until-noise E", "--noise-quantile Q", "--noise-floor F", "--max-passes N", "--noise-map FILE", "noise_stopped_at_pass"):
        assert opt in text, opt
