"""The refusals kajo_hip_create issues before it looks for a device (kajo_amd/csrc/launch_plan.h kajoCheckCreate), without a GPU: one row
per sentence of its validation, rows that trip two at once (the order), and the rows it accepts -- default tiles (0 -> 64x16), tileCount
0 -> 1, a frame of 1 x 2^31-1 whose padded tiles exceed 2^28 pixel blocks -- which a machine without a GPU answers with KAJO_E_NO_DEVICE:
the later refusals (LDS limit, 2^28 blocks, adaptive unit size) come after the device lookup. The (return code, kajo_hip_last_error text)
of every row is compared with tests/golden/create_refusals.json. The table was recorded on a machine without a GPU from the library as it
stood before create's validation moved out of capi.cpp into kajoCheckCreate: `table()` below over that commit's libkajo_hip.so, written
as {"rows": [[name, code, text], ...]}; its libkajo_hip_tune.so gave the same table. The product and the tools' twin answer alike. Where a
GPU is present the rows that expect KAJO_E_NO_DEVICE are skipped: there the call would go on to build a handle."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from kajo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "create_refusals.json")
LIBS = {"product": os.path.join(ROOT, "kajo_amd", "libkajo_hip.so"), "tune": os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")}

F = capi
AOV = F.KAJO_FLAG_AOV
# (name, scene variant, W, H, KajoParams fields over kajo_hip_default_params'): in the order of create's checks
ROWS = [
    ("null-scene", "null", 64, 64, {}),
    ("null-params", "good", 64, 64, None),
    ("null-out", "good", 64, 64, "no-out"),
    ("width-0", "good", 0, 64, {}),
    ("height-negative", "good", 64, -1, {}),
    ("frame-of-2^31-pixels", "good", 65536, 32768, {}),
    ("negative-plane-count", "neg-planes", 64, 64, {}),
    ("spheres-without-an-array", "no-sphere-array", 64, 64, {}),
    ("S-0", "good", 64, 64, dict(samplesPerPass=0)),
    ("S-65536", "good", 64, 64, dict(samplesPerPass=65536)),
    ("strict-and-exact", "good", 64, 64, dict(flags=F.KAJO_FLAG_STRICT | F.KAJO_FLAG_EXACT)),
    ("coop", "good", 64, 64, dict(flags=F.KAJO_FLAG_COOP)),
    ("deferred", "good", 64, 64, dict(flags=F.KAJO_FLAG_DEFERRED)),
    ("depth-negative", "good", 64, 64, dict(depthLimit=-1)),
    ("depth-1001", "good", 64, 64, dict(depthLimit=1001)),
    ("tile-4x64", "good", 64, 64, dict(tileW=4, tileH=64)),
    ("tile-12x64", "good", 64, 64, dict(tileW=12, tileH=64)),
    ("tile-8x8", "good", 64, 64, dict(tileW=8, tileH=8)),
    ("tile-negative", "good", 64, 64, dict(tileW=-64)),
    ("tile-count-negative", "good", 64, 64, dict(tileCount=-1)),
    ("tile-index-negative", "good", 64, 64, dict(tileIndex=-1)),
    ("tile-index-beyond", "good", 64, 64, dict(tileIndex=2, tileCount=2)),
    ("tile-index-1-of-default-count", "good", 64, 64, dict(tileIndex=1, tileCount=0)),
    ("aov-on-part-of-the-frame", "good", 64, 64, dict(flags=AOV, tileCount=2)),
    ("specular-without-aov", "good", 64, 64, dict(flags=F.KAJO_FLAG_AOV_SPECULAR)),
    ("matte-without-aov", "good", 64, 64, dict(flags=F.KAJO_FLAG_AOV_MATTE)),
    ("tiled-without-aov", "good", 64, 64, dict(flags=F.KAJO_FLAG_AOV_TILED)),
    ("adaptive-without-noise", "good", 64, 64, dict(flags=F.KAJO_FLAG_ADAPTIVE)),
    ("tiled-frame-too-wide", "good", 524289, 8, dict(flags=AOV | F.KAJO_FLAG_AOV_TILED)),
    ("tiled-frame-too-tall", "good", 8, 262145, dict(flags=AOV | F.KAJO_FLAG_AOV_TILED)),
    ("tiled-tile-too-wide", "good", 64, 64, dict(flags=AOV | F.KAJO_FLAG_AOV_TILED, tileW=524288, tileH=8)),
    ("tiled-tile-too-tall", "good", 64, 64, dict(flags=AOV | F.KAJO_FLAG_AOV_TILED, tileW=8, tileH=524288)),
    ("exact-far-coordinate", "far", 64, 64, {}),
    ("strict-tiny-coordinate", "tiny", 64, 64, dict(flags=F.KAJO_FLAG_STRICT)),
    ("exact-nan-coordinate", "nan", 64, 64, {}),
    # two at once: the earlier check answers
    ("size-before-scene-arrays", "neg-planes", 0, 64, {}),
    ("scene-arrays-before-S", "no-sphere-array", 64, 64, dict(samplesPerPass=0)),
    ("S-before-strict-and-exact", "good", 64, 64, dict(samplesPerPass=0, flags=F.KAJO_FLAG_STRICT | F.KAJO_FLAG_EXACT)),
    ("strict-and-exact-before-coop", "good", 64, 64, dict(flags=F.KAJO_FLAG_STRICT | F.KAJO_FLAG_EXACT | F.KAJO_FLAG_COOP)),
    ("coop-before-deferred", "good", 64, 64, dict(flags=F.KAJO_FLAG_COOP | F.KAJO_FLAG_DEFERRED)),
    ("deferred-before-depth", "good", 64, 64, dict(flags=F.KAJO_FLAG_DEFERRED, depthLimit=-1)),
    ("depth-before-tile", "good", 64, 64, dict(depthLimit=-1, tileW=4)),
    ("tile-before-tile-index", "good", 64, 64, dict(tileW=4, tileIndex=-1)),
    ("tile-index-before-aov-part", "good", 64, 64, dict(flags=AOV, tileIndex=2, tileCount=2)),
    ("aov-part-before-specular", "good", 64, 64, dict(flags=AOV | F.KAJO_FLAG_AOV_SPECULAR, tileCount=2)),
    ("specular-before-matte", "good", 64, 64, dict(flags=F.KAJO_FLAG_AOV_SPECULAR | F.KAJO_FLAG_AOV_MATTE)),
    ("matte-before-tiled", "good", 64, 64, dict(flags=F.KAJO_FLAG_AOV_MATTE | F.KAJO_FLAG_AOV_TILED)),
    ("tiled-before-adaptive", "good", 64, 64, dict(flags=F.KAJO_FLAG_AOV_TILED | F.KAJO_FLAG_ADAPTIVE)),
    ("adaptive-before-tiled-range", "good", 524289, 8, dict(flags=AOV | F.KAJO_FLAG_AOV_TILED | F.KAJO_FLAG_ADAPTIVE)),
    ("tiled-range-before-coordinates", "far", 524289, 8, dict(flags=F.KAJO_FLAG_EXACT | AOV | F.KAJO_FLAG_AOV_TILED)),
    # accepted: the device lookup answers on a machine without a GPU
    ("accepted-defaults", "good", 64, 64, {}),
    ("accepted-default-tiles", "good", 64, 64, dict(tileW=0, tileH=0)),
    ("accepted-default-tile-count", "good", 64, 64, dict(tileCount=0)),
    ("accepted-1-x-2^31-1", "good", 1, 2 ** 31 - 1, {}),
    ("accepted-fast-far-coordinate", "far", 64, 64, dict(flags=0)),
    ("accepted-every-flag", "good", 64, 64, dict(flags=F.KAJO_FLAG_EXACT | F.KAJO_FLAG_COUNTERS | AOV | F.KAJO_FLAG_AOV_SPECULAR | F.KAJO_FLAG_AOV_MATTE |
                                                 F.KAJO_FLAG_AOV_TILED | F.KAJO_FLAG_NOISE | F.KAJO_FLAG_ADAPTIVE, tileIndex=1, tileCount=3)),
    ("accepted-device-ordinal-99", "good", 64, 64, dict(device=99)),  # (the ordinal is looked at behind the device count)
]


def scene_pod(base, variant):
    """-> (KajoScene or None, what keeps its arrays alive)"""
    if variant == "null":
        return None, None
    sc = base
    if variant in ("far", "tiny", "nan"):
        spheres = base.spheres.copy()
        spheres[0, 12] = {"far": np.float32(2.0 ** 41), "tiny": np.float32(2.0 ** -41), "nan": np.float32("nan")}[variant]
        sc = type(base)(base.background, base.view, base.proj, spheres, base.planes, variant)
    pod = sc.pod()
    if variant == "neg-planes":
        pod.nPlanes = -1
    if variant == "no-sphere-array":
        pod.spheres = None
    return pod, sc


def table(path, base, names=None):
    """[name, return code, error text] of every row (of `names`), from the library at `path`"""
    L = C.CDLL(path)
    L.kajo_hip_last_error.restype = C.c_char_p
    L.kajo_hip_create.argtypes = [C.POINTER(capi.KajoScene), C.c_int, C.c_int, C.POINTER(capi.KajoParams), C.POINTER(C.c_void_p)]
    rows = []
    for name, variant, W, H, fields in ROWS:
        if names is not None and name not in names:
            continue
        pod, keep = scene_pod(base, variant)
        p = capi.KajoParams()
        L.kajo_hip_default_params(C.byref(p))
        for k, v in (fields.items() if isinstance(fields, dict) else ()):
            setattr(p, k, v)
        h = C.c_void_p()
        rc = L.kajo_hip_create(C.byref(pod) if pod is not None else None, W, H, None if fields is None else C.byref(p),
                               None if fields == "no-out" else C.byref(h))
        assert rc != 0 and not h.value, (name, rc)  # (no device here: nothing is ever built)
        rows.append([name, rc, (L.kajo_hip_last_error() or b"").decode()])
        del keep
    return rows


def gpu_present():
    try:
        n = C.c_int(0)
        return C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


@pytest.fixture(scope="module")
def golden_rows():
    with open(GOLDEN) as f:
        return json.load(f)["rows"]


def test_the_table_has_a_row_per_sentence_and_the_accepted_rows(golden_rows):
    assert [r[0] for r in golden_rows] == [r[0] for r in ROWS]
    refused = [r for r in golden_rows if r[1] == capi.KAJO_E_INVALID]
    accepted = [r for r in golden_rows if r[1] == capi.KAJO_E_NO_DEVICE]
    assert len(refused) + len(accepted) == len(golden_rows) and all(r[0].startswith("accepted-") for r in accepted)
    assert {r[0] for r in golden_rows if r[0].startswith("accepted-")} == {r[0] for r in accepted} and len(accepted) >= 5
    assert len({r[2] for r in accepted}) == 1
    # every sentence of create's validation: 16 fixed ones and the coordinate range's, which names what it found
    sentences = {r[2] for r in refused}
    assert len({s.split("(found")[0] for s in sentences}) == 17, sorted(sentences)
    assert sum("(found" in s for s in sentences) == 3


@pytest.mark.parametrize("which", sorted(LIBS))
def test_refusals_in_front_of_the_device_lookup_are_the_recorded_ones(which, golden_rows, scenes):
    assert os.path.exists(LIBS[which]), LIBS[which]
    want = [r for r in golden_rows if r[1] != capi.KAJO_E_NO_DEVICE]
    got = table(LIBS[which], scenes["spheres_a169"], {r[0] for r in want})
    assert len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong[:10]


@pytest.mark.parametrize("which", sorted(LIBS))
def test_what_create_accepts_meets_the_device_lookup(which, golden_rows, scenes):
    if gpu_present():
        pytest.skip("a GPU is present: these rows would build a handle")
    want = [r for r in golden_rows if r[1] == capi.KAJO_E_NO_DEVICE]
    got = table(LIBS[which], scenes["spheres_a169"], {r[0] for r in want})
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]
