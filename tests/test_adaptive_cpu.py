"""Adaptive sampling (include/kajo_hip.h "Adaptive sampling", kajo_amd/csrc/adapt_kernels.cpp, adapt_math.h) without a GPU: the flag, the
structs and the entry points as the header declares them; every refusal that comes before a device or a handle is looked for; the rule,
kajo_hip_adapt_evaluate, against a float64 numpy restatement; the filter of the launch order, kajo_hip_adapt_order, against a Python
model, and under AddressSanitizer + UBSan in a program of its own (tools/adapt_san.cpp); the Makefile's plan, what the compiler made of
the three kernels, and that the device code of every kernel from before is what it was, against digests recorded from the parent commit."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import devicecode
from kajo_amd import capi
from kajo_amd.renderer import NOISE_MOMENTS, AdaptParams, adapt_evaluate, adapt_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
ENTRY_POINTS = ("kajo_hip_default_adapt_params", "kajo_hip_set_adaptive", "kajo_hip_adapt_state", "kajo_hip_adapt_passes",
                "kajo_hip_adapt_evaluate", "kajo_hip_adapt_order")
KERNELS = ("kajo_adapt_step", "kajo_adapt_select", "kajo_adapt_passes")
F32, F64 = np.float32, np.float64


def _header():
    return open(os.path.join(ROOT, "include", "kajo_hip.h")).read()


def test_flag_structs_binding_and_libraries_agree():
    header = _header()
    for name, size in {"KajoAdaptParams": 32, "KajoAdaptState": 48}.items():
        cls = getattr(capi, name)
        assert C.sizeof(cls) == size, name
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        names = [n for line in re.findall(r"^\s+\w+ ([\w, \[\]]+);", fields, re.M) for n in re.sub(r"\[\d+\]", "", line).split(", ")]
        assert names == [f for f, _ in cls._fields_], (name, names)
        assert "} %s; " % name in header and "/* %d bytes */" % size in header
    assert re.search(r"#define KAJO_FLAG_ADAPTIVE 32768u", header) and capi.KAJO_FLAG_ADAPTIVE == 32768
    flags = {k: v for k, v in vars(capi).items() if k.startswith("KAJO_FLAG_") and v}
    assert [k for k, v in flags.items() if v & 32768] == ["KAJO_FLAG_ADAPTIVE"]
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values())
    assert "Adaptive sampling" in header and header.index("The noise estimate (KAJO_FLAG_NOISE)") < header.index("Adaptive sampling (KAJO_FLAG_ADAPTIVE")
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        if lib != capi.LIB_PATH and not os.path.exists(lib):
            continue
        nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in ENTRY_POINTS + tuple(k + "_launch" for k in KERNELS):
            assert re.search(r"\bT %s\b" % name, nm), (lib, name)


def test_default_params_are_the_documented_ones():
    L = capi.lib()
    p = capi.KajoAdaptParams(7.0, 7.0, 7, 7, 7, (7, 7, 7))
    L.kajo_hip_default_adapt_params(C.byref(p))
    assert (p.target, F32(p.floor), p.minPasses, p.checkEvery, p.allowance, list(p.reserved)) == (0.0, F32(1e-2), 16, 4, 0, [0, 0, 0])
    L.kajo_hip_default_adapt_params(None)  # accepted
    for text in ("(default 1e-2)", "(default 16)", "(default 4)", "(default 0)"):
        assert text in _header(), text


def test_the_flag_alone_is_refused_at_create_before_a_device_is_looked_for(scenes):
    L = capi.lib()
    pod = scenes["spheres_a1"].pod()
    for extra in (0, capi.KAJO_FLAG_EXACT, capi.KAJO_FLAG_AOV):
        p = capi.KajoParams()
        L.kajo_hip_default_params(C.byref(p))
        p.flags = capi.KAJO_FLAG_ADAPTIVE | extra
        h = C.c_void_p()
        assert L.kajo_hip_create(C.byref(pod), 16, 16, C.byref(p), C.byref(h)) == capi.KAJO_E_INVALID
        assert "adaptive flag" in L.kajo_hip_last_error().decode() and not h.value


def _good():
    p = capi.KajoAdaptParams()
    capi.lib().kajo_hip_default_adapt_params(C.byref(p))
    p.target = 0.05
    return p


@pytest.mark.parametrize("field,value,word", [
    ("target", 0.0, "target"), ("target", -1.0, "target"), ("target", float("nan"), "target"),
    ("floor", 0.0, "floor"), ("floor", float("inf"), "floor"), ("floor", float("nan"), "floor"),
    ("minPasses", -1, "minPasses"), ("checkEvery", 0, "checkEvery"), ("checkEvery", 65537, "checkEvery"),
    ("allowance", -1, "allowance"), ("allowance", 64, "allowance"),
])
def test_bad_parameters_are_refused_before_the_handle_is_looked_at(field, value, word):
    L = capi.lib()
    p = _good()
    setattr(p, field, value)
    assert L.kajo_hip_set_adaptive(None, C.byref(p)) == capi.KAJO_E_INVALID
    msg = L.kajo_hip_last_error().decode()
    assert word in msg and "adaptive" in msg, msg
    rec = np.zeros(1, NOISE_MOMENTS)
    assert L.kajo_hip_adapt_evaluate(rec.ctypes.data_as(C.c_void_p), 1, C.byref(p), None, None) == capi.KAJO_E_INVALID


def test_null_arguments_and_good_parameters_reach_the_handle_check():
    L = capi.lib()
    assert L.kajo_hip_set_adaptive(None, None) == capi.KAJO_E_INVALID and L.kajo_hip_last_error() == b"null adaptive parameters"
    p = _good()
    p.reserved[1] = 1
    assert L.kajo_hip_set_adaptive(None, C.byref(p)) == capi.KAJO_E_INVALID and b"reserved" in L.kajo_hip_last_error()
    for p in (_good(), capi.KajoAdaptParams(1e30, 1e-30, 0, 1, 63), capi.KajoAdaptParams(float("inf"), 1.0, 2 ** 31 - 1, 65536, 0)):
        assert L.kajo_hip_set_adaptive(None, C.byref(p)) == capi.KAJO_E_INVALID and L.kajo_hip_last_error() == b"null handle"
    state = capi.KajoAdaptState()
    assert L.kajo_hip_adapt_state(None, C.byref(state)) == capi.KAJO_E_INVALID
    assert L.kajo_hip_adapt_passes(None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_adapt_evaluate(None, 1, C.byref(_good()), None, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_adapt_evaluate(None, 0, C.byref(_good()), None, None) == capi.KAJO_OK
    one = np.zeros(1, np.uint32)
    assert L.kajo_hip_adapt_order(None, 1, None, 1, 0, None, 0) == capi.KAJO_E_INVALID
    assert L.kajo_hip_adapt_order(None, 1, one.ctypes.data_as(C.c_void_p), 5, 0, None, 0) == capi.KAJO_E_INVALID
    bad = np.array([1], np.uint32)
    assert L.kajo_hip_adapt_order(bad.ctypes.data_as(C.c_void_p), 1, one.ctypes.data_as(C.c_void_p), 1, 0, None, 0) == capi.KAJO_E_INVALID
    assert L.kajo_hip_adapt_order(None, 1, one.ctypes.data_as(C.c_void_p), 2, 1, None, 0) == 2  # the number of words
    assert L.kajo_hip_adapt_order(None, 1, one.ctypes.data_as(C.c_void_p), 2, 1, one.ctypes.data_as(C.c_void_p), 1) == capi.KAJO_E_INVALID


# ---- the rule ------------------------------------------------------------------------------------------------------------------------

def numpy_loud(rec, target, floor):
    """include/kajo_hip.h: rel in float64 with this floor, rounded to float32; loud = n < 2 or rel > target; bad is ignored"""
    n = rec["n"].astype(F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = rec["s1"] / (4.0 * n)
        v = np.maximum(rec["s2"] - rec["s1"] * rec["s1"] / n, 0.0) / (n - 1.0)
        rel = ((np.sqrt(v / n) / 4.0) / (np.maximum(m, 0.0) + F64(F32(floor)))).astype(F32)
    return (rec["n"] < 2) | (rel > F32(target)), rel


def test_the_rule_is_the_numpy_restatement():
    rng = np.random.default_rng(32768)
    N = 20000
    rec = np.zeros(N, NOISE_MOMENTS)
    n = rng.integers(0, 40, N)
    n[:300] = np.repeat([0, 1, 2], 100)
    mean = 10.0 ** rng.uniform(-4, 1, N) * rng.choice([1, 1, 1, -1], N)
    spread = 10.0 ** rng.uniform(-4, 0, N)
    for i in range(N):
        y = (mean[i] * (1 + spread[i] * rng.standard_normal(n[i]))).astype(F32).astype(F64)
        rec["n"][i], rec["s1"][i], rec["s2"][i] = n[i], y.sum(), (y * y).sum()
    # equal batches: s2 - s1^2 / n rounds to either side of zero
    k = slice(300, 600)
    c = rng.integers(2, 40, 300)
    y = (10.0 ** rng.uniform(-3, 1, 300)).astype(F32).astype(F64)
    rec["n"][k], rec["s1"][k], rec["s2"][k] = c, c * y, np.nextafter(c * y * y, 0)
    assert ((rec["s2"][k] - rec["s1"][k] ** 2 / c) < 0).any()
    rec["n"][600:700], rec["s1"][600:700], rec["s2"][600:700] = 8, 0.0, 0.0  # black
    rec["bad"][::7] = 3  # ignored
    for target, floor in ((0.05, 1e-2), (0.5, 1e-2), (1e-3, 1.0), (1e-30, 1e-2), (1e30, 1e-2)):
        want, _ = numpy_loud(rec, target, floor)
        got = adapt_evaluate(rec, dict(target=target, floor=floor))
        assert np.array_equal(got, want), (target, floor, np.flatnonzero(got != want)[:5])
        total = C.c_int64()
        p = AdaptParams(target, floor).pod()
        assert capi.lib().kajo_hip_adapt_evaluate(rec.ctypes.data_as(C.c_void_p), N, C.byref(p), None, C.byref(total)) == 0
        assert total.value == want.sum()
    want, rel = numpy_loud(rec, 0.05, 1e-2)
    assert want[:200].all() and not want[600:700].any() and 0.05 < want[700:].mean() < 0.95  # (the draws hold both kinds)
    # rel == target exactly is not loud; the float above it is quiet too, the float below makes the pixel loud
    i = int(np.flatnonzero((rec["n"] >= 2) & (rel > 0) & np.isfinite(rel))[0])
    one = rec[i:i + 1]
    assert not adapt_evaluate(one, dict(target=float(rel[i])))[0]
    assert not adapt_evaluate(one, dict(target=float(np.nextafter(rel[i], F32(np.inf)))))[0]
    assert adapt_evaluate(one, dict(target=float(np.nextafter(rel[i], F32(0)))))[0]
    bad = one.copy()
    bad["bad"] = 1000
    assert not adapt_evaluate(bad, dict(target=float(rel[i])))[0]


# ---- the order -----------------------------------------------------------------------------------------------------------------------

def model_order(order, state, w, split):
    out = []
    for u in (range(len(state)) if order is None else order):
        if state[u] == 0:
            out += [u * w + k for k in range(w)] if split else [u]
    return np.array(out, np.uint32)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_the_order_filter_is_the_python_model(w, split):
    rng = np.random.default_rng(w * 2 + split)
    for n in (1, 2, 9, 160):
        cost = rng.integers(0, 30, n)
        by_cost = np.argsort(-cost, kind="stable").astype(np.uint32)
        for state in (np.zeros(n, np.uint32), np.ones(n, np.uint32), (np.arange(n) & 1).astype(np.uint32), (1 - (np.arange(n) & 1)).astype(np.uint32),
                      np.where(rng.random(n) < 0.5, 7, 0).astype(np.uint32)):
            for order in (None, by_cost):
                got = adapt_order(order, state, w, split)
                assert np.array_equal(got, model_order(order, state, w, split)), (n, w, split, state[:8])
                assert got.size == (state == 0).sum() * (w if split else 1)


def test_the_filter_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "adapt_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tools", "adapt_san.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert ": ok" in p.stdout


# ---- the slot-to-pixel arithmetic is the tile map's inverse, at every tile shape -------------------------------------------------------

SLOT_SOURCE = r"""
// adaptSlotPixel (adapt_math.h) beside kajoTileSlot (render_args.h) as host code: for every case (W H tileW tileH owners) on the command
// line, as 32-bit words on stdout: the slots per owner; (owner, slot) of every pixel, row-major, by kajoTileSlot; then for every owner and
// every slot of its buffer (answer, px, py) by adaptSlotPixel. Map and geometry are the ones kajo_hip_create fills: launch_plan.h
// kajoFramePlan's, owner by owner.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "launch_plan.h"

int main(int argc, char** argv)
{
    for (int a = 1; a + 4 < argc; a += 5) {
        KajoParams p{};
        p.tileW = atoi(argv[a + 2]);
        p.tileH = atoi(argv[a + 3]);
        p.tileCount = atoi(argv[a + 4]);
        const int W = atoi(argv[a]), H = atoi(argv[a + 1]);
        const TileMap m = kajoFramePlan(W, H, p, KajoLdsPlan(), Numerics::Fast).map;
        std::vector<int32_t> out;
        out.push_back(m.slotsPerOwner);
        for (int y = 0; y < m.H; y++)
            for (int x = 0; x < m.W; x++) {
                int owner;
                uint32_t slot;
                kajoTileSlot(m, x, y, &owner, &slot);
                out.push_back(owner);
                out.push_back((int32_t)slot);
            }
        for (int o = 0; o < m.tileCount; o++) {
            p.tileIndex = o;
            const AdaptGeom g = kajoFramePlan(W, H, p, KajoLdsPlan(), Numerics::Fast).adaptGeom;
            for (uint32_t s = 0; s < (uint32_t)m.slotsPerOwner; s++) {
                int px = -1, py = -1;
                out.push_back(kajo::adaptSlotPixel(g, s, &px, &py) ? 1 : 0);
                out.push_back(px);
                out.push_back(py);
            }
        }
        if (fwrite(out.data(), sizeof(int32_t), out.size(), stdout) != out.size())
            return 1;
    }
    return 0;
}
"""
SLOT_FRAMES = [(100, 75), (41, 23), (9, 200)]


def _slot_cases():
    from test_hip_tile_shapes import DEFAULT, TILES
    assert DEFAULT == (64, 16) and DEFAULT not in TILES
    return [(tile, frame, owners) for tile in TILES + [DEFAULT] for frame in SLOT_FRAMES for owners in (1, 3)]


@pytest.fixture(scope="module")
def host_slot_pixels(tmp_path_factory):
    """case -> (slots per owner, kajoTileSlot's (H, W, 2), adaptSlotPixel's (owners, slots, 3)): the stand-alone program, one run"""
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("adaptslot")
    src, exe = str(d / "adapt_slots.cpp"), str(d / "adapt_slots")
    with open(src, "w") as f:
        f.write(SLOT_SOURCE)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = _slot_cases()
    args = [str(v) for (tw, th), (w, h), owners in cases for v in (w, h, tw, th, owners)]
    p = subprocess.run([exe, *args], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    words = np.frombuffer(p.stdout, np.int32)
    out, at = {}, 0
    for case in cases:
        _, (w, h), owners = case
        slots = int(words[at])
        forward = words[at + 1:at + 1 + 2 * w * h].reshape(h, w, 2)
        at += 1 + 2 * w * h
        out[case] = (slots, forward, words[at:at + 3 * owners * slots].reshape(owners, slots, 3))
        at += 3 * owners * slots
    assert at == words.size
    return out


def test_the_slot_to_pixel_arithmetic_is_the_exact_inverse_of_the_tile_map_at_every_tile_shape(host_slot_pixels):
    """kajo::adaptSlotPixel against kajoTileSlot, both compiled as host code from the headers the kernels are compiled from: every tile
    shape of tests/test_hip_tile_shapes.py and the default one, one owner and three, three ragged frames. Every pixel of the image goes
    to a slot that comes back as that pixel; every other slot of every owner's buffer -- a ragged tile's outside part, a padding tile
    beyond nTilesOwned -- is answered with false."""
    from kajo_amd.tiles import TileLayout
    cases = _slot_cases()
    assert len(cases) == 7 * 3 * 2
    for case in cases:
        tile, (W, H), owners = case
        slots, forward, back = host_slot_pixels[case]
        lay = TileLayout(W, H, owners, tile)
        assert slots == lay.slots_per_owner, case
        owner, slot = forward[..., 0], forward[..., 1]
        assert ((owner >= 0) & (owner < owners) & (slot >= 0) & (slot < slots)).all(), case
        ys, xs = np.mgrid[0:H, 0:W]
        # every in-image pixel round-trips
        there = back[owner, slot]
        wrong = (there[..., 0] != 1) | (there[..., 1] != xs) | (there[..., 2] != ys)
        assert not wrong.any(), (case, np.argwhere(wrong)[:4], there[wrong][:4])
        # ... and no other slot is answered with true: outside the image, or beyond the owner's tiles
        used = np.zeros((owners, slots), bool)
        used[owner, slot] = True
        assert used.sum() == W * H, case  # (the map takes no slot twice)
        assert np.array_equal(back[..., 0] == 1, used), (case, np.argwhere((back[..., 0] == 1) != used)[:4])
        assert (~used).any() or (W % tile[0] == 0 and H % tile[1] == 0), case
    # the cases hold a padding tile (three owners, a tile count that is no multiple of three) and an owner without a tile
    assert any(TileLayout(W, H, o, t).n_tiles % o for t, (W, H), o in cases if o == 3)
    assert any(TileLayout(W, H, o, t).n_tiles < o for t, (W, H), o in cases)


# ---- the build -----------------------------------------------------------------------------------------------------------------------

def test_the_new_unit_is_in_both_link_lines_and_there_is_no_third_library():
    devicecode.need_tools()
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("adapt_kernels.o" in l and "noise.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "/adapt_kernels.cpp" in l]
    assert len(compiles) == 1, compiles
    cmd = compiles[0].split()
    assert "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd and cmd[cmd.index("-x") + 1] == "hip"
    # the rule's header names nothing of the estimate's unit, and the estimate's unit is untouched by it
    text = open(os.path.join(CSRC, "adapt_math.h")).read()
    assert "render_args.h" not in text and "#include \"noise" not in text
    assert re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, "adapt_kernels.cpp")).read()) == ["adapt_math.h", "render_args.h"]


def test_adaptive_kernels_spill_nothing_and_use_no_scratch_or_flat_access():
    b = devicecode.build("adapt_kernels.cpp")
    res, text = b.resources, b.asm
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k in KERNELS:
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["Occupancy"] == 8, (k, r)
        body = devicecode.body(text, k, end=".Lfunc_end")
        assert not re.search(r"\n\s+flat_\w+", body) and not re.search(r"\n\s+scratch_\w+", body), k
        stores = re.findall(r"\n\s+(global_store_\w+)", body)
        loads = re.findall(r"\n\s+(global_load_\w+)", body)
        atomics = re.findall(r"\n\s+(\w*atomic\w*)", body)
        assert not atomics, (k, atomics)
        if k == "kajo_adapt_step":
            # streams: the state word, then 16 bytes at a time (T's three colour words may come as one 12-byte load); no LDS, no cross-lane
            assert r["LDS Size"] == 0 and set(stores) == {"global_store_dwordx4"} and len(stores) == 4, stores
            # (a retired slot's record is read for n alone: the compiler narrows that half's load to the 8 bytes used)
            assert set(loads) <= {"global_load_dword", "global_load_dwordx2", "global_load_dwordx3", "global_load_dwordx4"}, loads
            assert loads.count("global_load_dword") == 1 and loads.count("global_load_dwordx4") + loads.count("global_load_dwordx3") >= 5, loads
            assert not re.search(r"\n\s+(ds_|v_readlane|v_permlane|v_mov_b32_dpp|s_barrier)\w*", body), k
            assert "v_mul_f64" in body and "v_add_f64" in body
        elif k == "kajo_adapt_select":
            # the record's two halves in, a ballot's population count, the waves' answers through LDS, one plain store of the state word
            # (of the record's second half only n is used: that load is narrowed to its 8 bytes)
            assert r["LDS Size"] == 16 and sorted(loads) == ["global_load_dwordx2", "global_load_dwordx4"] and stores == ["global_store_dword"], (r, loads, stores)
            assert re.search(r"\n\s+s_bcnt1_i32_b64", body) and "s_barrier" in body and re.search(r"\n\s+ds_(write|store)_b32", body)


def test_the_device_code_of_every_kernel_from_before_is_unchanged_function_by_function():
    """tests/golden/kernel_digests_before_adaptive.json: tools/kernel_digests.py over the parent commit -- all fourteen device units, the
    noise estimate's among them. The working tree must give the same functions with the same digests: adaptive sampling moved no kernel.
    (Its own unit is HIP source in a .cpp file, which the tool, made for the .hip units, does not list.)"""
    devicecode.need_tools()
    tool = devicecode.digest_tool()
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_digests_before_adaptive.json")))
    before = recorded["units"]
    assert sorted(before) == sorted(["kernel_fast", "kernel_exact", "kernel_strict", "aux_kernels", "denoise", "glare", "despeckle", "meter", "local",
                                     "lens", "view", "matte", "grade", "noise"])
    assert sorted(before["noise"]) == ["kajo_noise_map", "kajo_noise_update"] and sum(len(f) for f in before.values()) > 100
    now = devicecode.digests_now()
    where = "(recorded with %s; this is %s)" % (recorded["compiler"], tool.compiler())
    assert sorted(now) == sorted(before), (sorted(now), where)
    for unit in before:
        assert sorted(now[unit]) == sorted(before[unit]), (unit, sorted(set(now[unit]) ^ set(before[unit])), where)
        moved = [f for f in before[unit] if now[unit][f] != before[unit][f]]
        assert not moved, (unit, moved, where)


# ---- does it do its job: the scheme emulated over the CPU oracle's per-batch frames ----------------------------------------------------
# spheres_a169 at 32 x 24, S = 4, 64 passes = 16 batches, as tests/test_noise_cpu.py renders them; pixel blocks of 8 x 8 are the units
# (12 of them), decisions at passes 16, 32, 48 and 64, allowance 0, floor 1e-2. A retired block keeps its mean at retirement. Against an
# oracle render of 8192 passes (another seed): the RMSE of the adaptive frame, and of a uniform render of the same seed with the same
# number of camera paths rounded down to whole passes; pooled over K seeds (root of the summed squares), because one seed's RMSE at four
# samples a pass is led by a handful of fireflies and swings by a factor of three.
# Measured with the oracle, target 0.55, four disjoint groups of 16 seeds: pooled ratio adaptive / uniform 1.399 (this test's seeds),
# 1.580, 1.371, 1.535 -- a spread of 0.21 --; blocks retired by pass 64: 33 %, 34 %, 31 %, 36 % on average; camera paths saved 15 %, 15 %,
# 15 %, 17 %. That is: at this size the scheme is WORSE than the uniform render of equal paths, by about 1.4 to 1.6 in RMSE. A block
# that looks quiet after 16 to 48 passes of four samples has not yet met its fireflies, and the frozen mean misses them (the bias DESIGN.md 6o
# names). The bound below is the measured ratio plus a quarter, as the spread asks; the test cannot pass with nothing or everything retired.
QUALITY_TARGET, QUALITY_SEEDS, QUALITY_RATIO = 0.55, 16, 1.399


def _emulate(handle, W, H, seed, target, floor=1e-2):
    acc, base = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    rec = np.zeros((H, W), NOISE_MOMENTS)
    retired, frozen, mean = np.zeros((H, W), np.int64), np.zeros((H, W, 3)), None
    for b in range(16):
        handle.render(W, H, S=4, passes=4, seed=seed, first_pass=4 * b + 1, accum=acc)
        D = acc - base
        y = F32(0.2126) * D[..., 0] + F32(0.7152) * D[..., 1] + F32(0.0722) * D[..., 2]
        ok = np.isfinite(y) & (retired == 0)
        d = np.where(ok, y.astype(F64), 0.0)
        rec["n"] += ok
        rec["s1"] += d
        rec["s2"] += d * d
        base = acc.copy()
        P = 4 * (b + 1)
        mean = acc[..., :3].astype(F64) / P
        if P % 16 == 0:
            loud, _ = numpy_loud(rec, target, floor)
            for by in range(H // 8):
                for bx in range(W // 8):
                    at = (slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
                    if (retired[at] == 0).all() and not loud[at].any():
                        retired[at] = P
                        frozen[at] = mean[at]
    return np.where((retired > 0)[..., None], frozen, mean), np.where(retired > 0, retired, 64)


def test_the_scheme_against_a_uniform_render_of_equal_camera_paths(scenes):
    from oraclelib import OracleLib, available
    if not available("oracle"):
        pytest.skip("oracle not built")
    handle = OracleLib("oracle").create(scenes["spheres_a169"], 1)
    W, H = 32, 24
    truth = handle.render(W, H, S=4, passes=8192, seed=99991)[..., :3].astype(F64) / 8192

    def squared_error(frame):
        d = frame - truth
        return np.mean(d[np.isfinite(d).all(-1)] ** 2)

    adaptive = uniform = 0.0
    shares, saved = [], []
    for k in range(QUALITY_SEEDS):
        seed = 236367 + 1000 * k
        frame, passes = _emulate(handle, W, H, seed, QUALITY_TARGET)
        U = int(passes.sum() // (W * H))
        same_paths = handle.render(W, H, S=4, passes=U, seed=seed)[..., :3].astype(F64) / U
        adaptive += squared_error(frame)
        uniform += squared_error(same_paths)
        shares.append(float((passes < 64).mean()))
        saved.append(1.0 - passes.sum() / (64.0 * W * H))
    ratio = float(np.sqrt(adaptive / uniform))
    print("blocks retired by pass 64: %.3f on average (%.2f .. %.2f); camera paths saved %.3f; RMSE adaptive %.4f, uniform at equal paths %.4f, "
          "ratio %.3f" % (np.mean(shares), min(shares), max(shares), np.mean(saved), np.sqrt(adaptive / QUALITY_SEEDS),
                          np.sqrt(uniform / QUALITY_SEEDS), ratio))
    # the condition on the input: neither nothing nor everything retires
    assert 0.25 <= np.mean(shares) <= 0.75, np.mean(shares)
    assert ratio <= QUALITY_RATIO + 0.25, ratio
