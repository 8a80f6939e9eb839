"""Depth of field (include/kajo_hip.h kajo_hip_lens*, kajo_amd/csrc/lens.hip) without a GPU: the struct, the constant and the entry points
as the header declares them, in the product and the tools' twin; the documented defaults; every refusal that comes before a device is
looked at, and their order across the stages (despeckle, lens, glare, local, meter, tone, denoise, handle); the Makefile's plan; the
driver's refusals and help; the kernels' budgets from the compiler's remarks; and properties of the numpy restatement the GPU tests hold
the kernels to (tests/lens_replay.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import devicecode
from kajo_amd import capi
from lens_replay import aov_from_depth, restate
from local_replay import synthetic_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
ENTRY_POINTS = ("kajo_hip_default_lens_params", "kajo_hip_lens", "kajo_hip_lens_coc", "kajo_hip_lens_depth_at", "kajo_hip_present_lens_argb8")
F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")


def _params(cls, default, **kw):
    p = cls()
    getattr(capi.lib(), default)(C.byref(p))
    for k, v in kw.items():
        if k.startswith("reserved") and k != "reserved":
            p.reserved[int(k[len("reserved"):])] = v
        else:
            setattr(p, k, v)
    return p


def _lens(**kw):
    return _params(capi.KajoLensParams, "kajo_hip_default_lens_params", **kw)


def _despeckle(**kw):
    return _params(capi.KajoDespeckleParams, "kajo_hip_default_despeckle_params", **kw)


def _glare(**kw):
    return _params(capi.KajoGlareParams, "kajo_hip_default_glare_params", **kw)


def _local(**kw):
    return _params(capi.KajoLocalParams, "kajo_hip_default_local_params", **kw)


def _meter(**kw):
    return _params(capi.KajoMeterParams, "kajo_hip_default_meter_params", **kw)


def _tone(**kw):
    return _params(capi.KajoToneParams, "kajo_hip_default_tone_params", **kw)


def _denoise(**kw):
    return _params(capi.KajoDenoiseParams, "kajo_hip_default_denoise_params", **kw)


def _ref(p):
    return None if p is None else C.byref(p)


def _error():
    return (capi.lib().kajo_hip_last_error() or b"").decode()


def test_header_struct_constant_binding_and_libraries_agree():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    assert C.sizeof(capi.KajoLensParams) == 32
    fields = re.search(r"typedef struct KajoLensParams \{(.*?)\} KajoLensParams;", header, re.S).group(1)
    names = re.findall(r"^\s+\w+ (\w+)(?:\[\d+\])?;", fields, re.M)
    assert names == [f for f, _ in capi.KajoLensParams._fields_] == ["aperture", "focusDistance", "maxRadius", "flags", "reserved"]
    assert re.search(r"#define KAJO_LENS_MAX_RADIUS 16\b", header) and capi.KAJO_LENS_MAX_RADIUS == 16
    assert "image-space approximation" in header.lower()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    for lib in (capi.LIB_PATH, os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")):
        L = C.CDLL(lib)
        for name in ENTRY_POINTS:
            assert hasattr(L, name), (lib, name)
    version = capi.lib().kajo_hip_version()
    assert b"gfx950" in version and b"lens" in version.split(b";")[-1]


def test_defaults():
    p = capi.KajoLensParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    capi.lib().kajo_hip_default_lens_params(C.byref(p))
    assert F32(p.aperture) == F32(0.01) and p.focusDistance == 10.0 and p.maxRadius == 16 and p.flags == 0
    assert list(p.reserved) == [0.0] * 4
    capi.lib().kajo_hip_default_lens_params(None)  # NULL is accepted


BAD_FIELDS = [
    (dict(aperture=-0.01), "lens aperture must be finite and in [0, 1]"),
    (dict(aperture=1.0001), "lens aperture must be finite and in [0, 1]"),
    (dict(aperture=NAN), "lens aperture must be finite and in [0, 1]"),
    (dict(aperture=INF), "lens aperture must be finite and in [0, 1]"),
    (dict(focusDistance=0.0), "lens focus distance must be finite and positive"),
    (dict(focusDistance=-1.0), "lens focus distance must be finite and positive"),
    (dict(focusDistance=NAN), "lens focus distance must be finite and positive"),
    (dict(focusDistance=INF), "lens focus distance must be finite and positive"),
    (dict(maxRadius=0), "lens max radius must be in [1, 16]"),
    (dict(maxRadius=-3), "lens max radius must be in [1, 16]"),
    (dict(maxRadius=17), "lens max radius must be in [1, 16]"),
    (dict(flags=1), "unknown lens flag"),
    (dict(flags=0x80000000), "unknown lens flag"),
    (dict(reserved0=1.0), "lens reserved fields must be 0"),
    (dict(reserved3=NAN), "lens reserved fields must be 0"),
]


def _calls(lens, despeckle=None, denoise=None, glare=None, local=None, meter=None, tone=None):
    """the entry points that take the stage's parameters, with a NULL handle: -> [(name, rc, message)]"""
    L = capi.lib()
    tone = tone if tone is not None else _tone()
    out = []
    rc = L.kajo_hip_lens(None, _ref(despeckle), _ref(denoise), _ref(lens), None)
    out.append(("lens", rc, _error()))
    rc = L.kajo_hip_lens_coc(None, _ref(lens), None, None)
    out.append(("coc", rc, _error()))
    rc = L.kajo_hip_present_lens_argb8(None, _ref(despeckle), _ref(denoise), _ref(lens), _ref(glare), _ref(local), _ref(meter), C.byref(tone),
                                       None, None)
    out.append(("present", rc, _error()))
    return out


@pytest.mark.parametrize("fields,message", BAD_FIELDS, ids=["%s" % sorted(f.items()) for f, _ in BAD_FIELDS])
def test_every_refusal_comes_before_the_handle(fields, message):
    for name, rc, text in _calls(_lens(**fields)):
        assert rc == capi.KAJO_E_INVALID and text == message, (name, rc, text)


def test_the_edges_of_the_ranges_are_accepted_and_a_null_struct_is_not():
    for fields in (dict(aperture=0.0), dict(aperture=1.0), dict(focusDistance=1e-6), dict(focusDistance=1e30), dict(maxRadius=1),
                   dict(maxRadius=16)):
        for name, rc, text in _calls(_lens(**fields)):
            assert rc == capi.KAJO_E_INVALID and text == "null handle", (fields, name, text)
    L = capi.lib()
    assert L.kajo_hip_lens(None, None, None, None, None) == capi.KAJO_E_INVALID and _error() == "null lens parameters"
    assert L.kajo_hip_lens_coc(None, None, None, None) == capi.KAJO_E_INVALID and _error() == "null lens parameters"
    z = C.c_float()
    assert L.kajo_hip_lens_depth_at(None, 0, 0, C.byref(z)) == capi.KAJO_E_INVALID and _error() == "null argument"
    # lens == NULL in the chain entry is kajo_hip_present_local_argb8: its refusals, not this stage's
    assert L.kajo_hip_present_lens_argb8(None, None, None, None, None, None, None, C.byref(_tone()), None, None) == capi.KAJO_E_INVALID
    assert _error() == "null handle"
    assert L.kajo_hip_present_lens_argb8(None, None, None, None, None, C.byref(_local(detail=9.0)), None, C.byref(_tone()), None,
                                         None) == capi.KAJO_E_INVALID
    assert _error() == "local detail must be finite and in [0, 4]"


def test_the_order_of_refusals_across_the_stages():
    """despeckle, lens, glare, local, meter, tone, denoise, handle: each stage's bad parameters are reported while everything after it is
    bad too."""
    bad = dict(despeckle=_despeckle(rank=9), lens=_lens(maxRadius=99), glare=_glare(levels=99), local=_local(detail=9.0),
               meter=_meter(key=-1.0), tone=_tone(exposure=99.0), denoise=_denoise(iterations=99))
    good = dict(despeckle=_despeckle(), lens=_lens(), glare=_glare(), local=_local(), meter=_meter(), tone=_tone(), denoise=_denoise())
    messages = dict(despeckle="despeckle rank must be in [1, 4]", lens="lens max radius must be in [1, 16]",
                    glare="glare levels must be in [0, 12]", local="local detail must be finite and in [0, 4]",
                    meter="meter key must be finite and positive", tone="tone exposure must be finite and in [-32, 32]",
                    denoise="denoise iterations must be in [0, 8]")
    order = ["despeckle", "lens", "glare", "local", "meter", "tone", "denoise"]
    takes = dict(lens=("despeckle", "lens", "denoise"), coc=("lens",), present=order)
    for i, first in enumerate(order):
        args = {k: (good[k] if order.index(k) < i else bad[k]) for k in order}
        for name, rc, text in _calls(**args):
            assert rc == capi.KAJO_E_INVALID, (first, name)
            want = next((messages[k] for k in order[i:] if k in takes[name]), None)
            assert text == (want or "null handle"), (first, name, text)
    for name, rc, text in _calls(**good):
        assert rc == capi.KAJO_E_INVALID and text == "null handle", (name, text)
    # the metered exposure and the tone parameters' automatic exposure: refused with the tone parameters, before the denoiser's
    name, rc, text = _calls(lens=_lens(), meter=_meter(), tone=_tone(flags=capi.KAJO_TONE_AUTO_EXPOSURE), denoise=bad["denoise"])[2]
    assert rc == capi.KAJO_E_INVALID and "two automatic exposures" in text, (name, text)


def test_makefile_compiles_the_stage_once_and_links_it_twice():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("lens.o" in l for l in links), links
    compiles = [l for l in plan.splitlines() if l.startswith("hipcc") and "lens.hip" in l]
    assert len(compiles) == 1 and "-ffp-contract=off" in compiles[0] and "gfx950" in compiles[0], compiles
    assert "lens.hip" in open(os.path.join(CSRC, "Makefile")).read().split("HIPCC")[0]  # the header comment


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
@pytest.mark.parametrize("args,message", [
    (["--lens-aperture", "-0.1"], "lens aperture must be finite and in [0, 1]"),
    (["--lens-aperture", "1.5"], "lens aperture must be finite and in [0, 1]"),
    (["--lens-aperture", "nan"], "lens aperture must be finite and in [0, 1]"),
    (["--lens-aperture", "wide"], "lens aperture must be finite and in [0, 1]"),
    (["--lens-aperture", "0.02", "--lens-focus", "0"], "lens focus distance must be finite and positive"),
    (["--lens-aperture", "0.02", "--lens-focus", "inf"], "lens focus distance must be finite and positive"),
    (["--lens-aperture", "0.02", "--lens-focus", "near"], "lens focus distance must be finite and positive"),
    (["--lens-aperture", "0.02", "--lens-max-radius", "0"], "lens max radius must be in [1, 16]"),
    (["--lens-aperture", "0.02", "--lens-max-radius", "17"], "lens max radius must be in [1, 16]"),
    (["--lens-aperture", "0.02", "--lens-max-radius", "4x"], "lens max radius must be in [1, 16]"),
    (["--lens-aperture", "0.02", "--lens-focus-at", "5"], "--lens-focus-at X,Y must be a pixel of the frame"),
    (["--lens-aperture", "0.02", "--lens-focus-at", "-1,3"], "--lens-focus-at X,Y must be a pixel of the frame"),
    (["--lens-aperture", "0.02", "-w", "64", "-h", "32", "--lens-focus-at", "64,3"], "--lens-focus-at X,Y must be a pixel of the frame"),
    (["--lens-aperture", "0.02", "--lens-focus-at", "3,4,5"], "--lens-focus-at X,Y must be a pixel of the frame"),
    (["--lens-aperture", "0.02", "--lens-focus", "3", "--lens-focus-at", "3,4"], "two ways to focus"),
    (["--lens-focus", "3"], "shape the stage that --lens-aperture turns on"),
    (["--lens-focus-at", "3,4"], "shape the stage that --lens-aperture turns on"),
    (["--lens-max-radius", "8"], "shape the stage that --lens-aperture turns on"),
    (["--lens-aperture", "0.02", "--gpus", "3"], "--lens-aperture needs the whole frame on one GPU (--gpus 1, without --three-arg)"),
    (["--lens-aperture", "0.02", "--three-arg"], "--lens-aperture needs the whole frame on one GPU (--gpus 1, without --three-arg)"),
])
def test_driver_refuses_bad_lens_options_before_opening_a_device(tmp_path, args, message):
    out = tmp_path / "o.png"
    p = subprocess.run([BIN, *args, "-o", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_help_lists_the_lens_options():
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--lens-aperture A", "--lens-focus D", "--lens-focus-at X,Y", "--lens-max-radius R", "lens_focus", "lens_max_radius_px"):
        assert opt in text, opt
    assert text.index("--lens-aperture A") > text.index("--local-pivot STOPS|metered[:Q]") > text.index("    -v  ")  # appended


# -- the kernels' budgets --------------------------------------------------------------------------------------------------------------

# kernel -> (VGPRs at most, waves per SIMD, LDS bytes per workgroup): what the build produces. The gather is held to 4 waves per SIMD by
# its LDS -- two workgroups of eight waves on a CU's 160 KiB -- not by its registers
KERNELS = {"kajo_lens_prepare": (21, 8, 0), "kajo_lens_gather": (29, 4, 62640)}


def test_lens_kernels_keep_their_budgets():
    b = devicecode.build("lens.hip")
    assert "-ffp-contract=off" in b.cmd and "--offload-arch=gfx950" in b.cmd
    res = b.resources
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k, (vgprs, waves, lds) in KERNELS.items():
        r = res[k]
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["AGPRs"] == 0, (k, r)
        assert r["VGPRs"] <= vgprs and r["Occupancy"] == waves and r["LDS Size"] == lds, (k, r)
    assert 2 * KERNELS["kajo_lens_gather"][2] <= 160 * 1024  # two workgroups fit a CU


# -- the restatement itself ---------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _flat(W, H, depth):
    return aov_from_depth(np.full((H, W), depth, F32))


def test_restatement_copy_cases():
    P = 3
    for name, F in synthetic_frames(41, 23, P).items():
        A, B = _flat(41, 23, 25.0)
        r = restate(F, A, B, P, aperture=0.0)
        assert np.array_equal(_bits(r["out"]), _bits(F)), name


def test_restatement_all_in_focus_is_the_mean_times_the_passes():
    P = 3
    for name, F in synthetic_frames(41, 23, P).items():
        A, B = _flat(41, 23, 10.0)
        r = restate(F, A, B, P, aperture=0.5, focus_distance=10.0)
        assert not r["r"].any()
        c = r["counts"]
        with np.errstate(all="ignore"):
            want = (F[..., :3] / F32(P)).astype(F32).astype(F64) * P
        assert np.array_equal(r["out64"][c], want[c]), name
        assert np.array_equal(_bits(r["out"][~c]), _bits(F[~c])) and np.array_equal(_bits(r["out"][..., 3]), _bits(F[..., 3])), name


def test_restatement_constant_frame_stays_constant_under_any_depth():
    P = 4
    W, H = 41, 23
    F = synthetic_frames(W, H, P)["constant"]
    xs = np.arange(W, dtype=F32)[None, :].repeat(H, 0)
    step = np.where(xs < W // 2, 10.0, 40.0).astype(F32)
    ramp = (2.5 + 30.0 * xs / (W - 1)).astype(F32)
    m = (F[..., :3] / F32(P)).astype(F32).astype(F64) * P
    for depth in (step, ramp):
        for R in (5, 16):
            A, B = aov_from_depth(depth)
            r = restate(F, A, B, P, aperture=0.3, focus_distance=10.0, max_radius=R)
            assert r["r"].max() > 1
            rel = np.abs(r["out64"] - m) / m
            assert rel.max() <= 1100 * 2.0 ** -53, rel.max()


@pytest.mark.parametrize("radius", [1.0, 2.0, 4.7, 8.0, 16.0])
def test_restatement_keeps_the_energy_of_a_bright_pixel(radius):
    """a single bright pixel on a plane of constant circle of confusion r: the divisor 1 + pi r (r + 1) approximates the lattice sum of
    the disc, so the energy spread over the neighbours sums to the pixel's within 3 %"""
    P = 2
    N = 69  # (every window that holds the pixel lies inside the image: its normalisation is the whole lattice sum)
    F = np.zeros((N, N, 4), F32)
    F[N // 2, N // 2, :3] = F32([900.0, 450.0, 120.0]) * P
    # u = |1 - f / z| = 1/2 at z = 2 f: r = aperture H / 2
    A, B = _flat(N, N, 20.0)
    r = restate(F, A, B, P, aperture=2.0 * radius / N, focus_distance=10.0, max_radius=16)
    assert np.allclose(r["r"], radius, rtol=1e-6)
    ratio = r["out64"].sum((0, 1)) / F[..., :3].astype(F64).sum((0, 1))
    assert (ratio >= 0.97).all() and (ratio <= 1.03).all(), ratio


def test_restatement_sharp_foreground_takes_nothing_from_a_defocused_background():
    """left half in focus and dark, right half far, bright and blurred: on the foreground side re = min(r_q, r_p) = 0 for every tap behind
    it, so no background energy crosses the edge, and the foreground comes out as (F / P) P."""
    P = 2
    W, H = 48, 20
    F = np.full((H, W, 4), 0.01, F32) * P
    F[:, W // 2:, :3] = F32(500.0) * P
    depth = np.full((H, W), 10.0, F32)
    depth[:, W // 2:] = 80.0
    A, B = aov_from_depth(depth)
    r = restate(F, A, B, P, aperture=0.9, focus_distance=10.0, max_radius=16)
    assert (r["r"][:, :W // 2] == 0).all() and (r["r"][:, W // 2:] > 10).all()
    want = (F[..., :3] / F32(P)).astype(F32).astype(F64) * P
    assert np.array_equal(r["out64"][:, :W // 2], want[:, :W // 2])
    # the other way round the blurred foreground does lie over the sharp background
    depth = np.full((H, W), 10.0, F32)
    depth[:, W // 2:] = 1.25
    A, B = aov_from_depth(depth)
    r = restate(F, A, B, P, aperture=0.1, focus_distance=10.0, max_radius=16)
    assert (r["r"][:, :W // 2] == 0).all() and (r["r"][:, W // 2:] > 10).all()
    assert (r["out64"][:, W // 2 - 4:W // 2, 0] > 10 * want[0, 0, 0]).all()


def test_restatement_never_spreads_a_poisoned_pixel():
    P = 3
    for W, H in ((7, 5), (41, 23)):
        F = synthetic_frames(W, H, P)["poisoned"]
        A, B = _flat(W, H, 20.0)
        for R in (1, 16):
            r = restate(F, A, B, P, aperture=1.0, focus_distance=10.0, max_radius=R)
            c = r["counts"]
            assert 4 <= (~c).sum() <= 6 and c.sum() >= 29
            assert np.array_equal(_bits(r["out"][~c]), _bits(F[~c])), R
            assert np.isfinite(r["out"][c][:, :3]).all(), R
            assert np.array_equal(_bits(r["out"][..., 3]), _bits(F[..., 3]))
            assert (r["sumW"][c] > 0).all()
