"""The refusals of the display chain (include/kajo_hip.h: despeckle -> denoise -> grade -> lens -> glare -> local -> meter -> tone ->
view) without a GPU: every chain entry point called with a null handle, so that nothing reaches a device, over a matrix of its stages --
each one absent, all good, each one bad together with every stage checked after it, no tone parameters, no destination -- and the
(return code, kajo_hip_last_error text) of every row compared with tests/golden/chain_refusals.json. The table was recorded from the
library as it stood before the chain entries became wrappers of one check and one run (kajo_amd/csrc/present.cpp checkChain / runChain);
the product and the tools' twin answer alike."""
import ctypes as C
import json
import os

import pytest

from kajo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_refusals.json")
LIBS = {"product": os.path.join(ROOT, "kajo_amd", "libkajo_hip.so"), "tune": os.path.join(ROOT, "kajo_amd", "libkajo_hip_tune.so")}

# the order the refusals are issued in: the stages' parameters, the view's, then the denoiser's (which looks at the handle)
CHECK_ORDER = ("despeckle", "grade", "lens", "glare", "local", "meter", "tone", "view", "denoise")

# every chain entry point and its arguments in the header's order; `dst` is what the call fills (image, radiance or histogram)
ENTRIES = {
    "kajo_hip_tonemap_argb8": "h tone denoise dst scale",
    "kajo_hip_tonemap_gathered_argb8_device": "h gathered tone dst",
    "kajo_hip_glare": "h glare denoise dst",
    "kajo_hip_display_argb8": "h denoise glare tone dst scale",
    "kajo_hip_display_gathered_argb8_device": "h gathered glare tone dst",
    "kajo_hip_present_argb8": "h despeckle denoise glare tone dst scale",
    "kajo_hip_present_gathered_argb8_device": "h gathered despeckle glare tone dst",
    "kajo_hip_meter": "h despeckle denoise glare meter dst result",
    "kajo_hip_present_metered_argb8": "h despeckle denoise glare meter tone dst result",
    "kajo_hip_present_metered_gathered_argb8_device": "h gathered despeckle glare meter tone dst result",
    "kajo_hip_local": "h despeckle denoise glare local dst",
    "kajo_hip_present_local_argb8": "h despeckle denoise glare local meter tone dst result",
    "kajo_hip_present_local_gathered_argb8_device": "h gathered despeckle glare local meter tone dst result",
    "kajo_hip_lens": "h despeckle denoise lens dst",
    "kajo_hip_present_lens_argb8": "h despeckle denoise lens glare local meter tone dst result",
    "kajo_hip_present_view_argb8": "h despeckle denoise lens glare local meter tone view dst result",
    "kajo_hip_present_view_gathered_argb8_device": "h gathered despeckle glare local meter tone view dst result",
    "kajo_hip_grade": "h despeckle denoise grade dst",
    "kajo_hip_present_grade_argb8": "h despeckle denoise grade lens glare local meter tone view dst result",
    "kajo_hip_present_grade_gathered_argb8_device": "h gathered despeckle grade glare local meter tone view dst result",
}

STRUCTS = {"despeckle": capi.KajoDespeckleParams, "grade": capi.KajoGradeParams, "lens": capi.KajoLensParams, "glare": capi.KajoGlareParams,
           "local": capi.KajoLocalParams, "meter": capi.KajoMeterParams, "tone": capi.KajoToneParams, "view": capi.KajoViewParams,
           "denoise": capi.KajoDenoiseParams}


def spoil(stage, p):
    """one field of a stage's parameters out of range"""
    if stage == "despeckle":
        p.rank = 0
    elif stage == "grade":
        p.nRegions = 9
    elif stage == "lens":
        p.maxRadius = 0
    elif stage == "glare":
        p.levels = -1
    elif stage == "local":
        p.iterations = -1
    elif stage == "meter":
        p.key = -1.0
    elif stage == "tone":
        p.curve = 99
    elif stage == "view":
        p.outW = 0
    elif stage == "denoise":
        p.iterations = -1


def good(L, stage):
    p = STRUCTS[stage]()
    getattr(L, "kajo_hip_default_%s_params" % stage)(C.byref(p))
    if stage == "view":
        p.outW = p.outH = 8
    return p


def cases(slots):
    """(case name, {stage: 'good' | 'bad' | 'auto' | 'regions' | None}, dst given) of one entry point"""
    stages = [s for s in CHECK_ORDER if s in slots]
    allGood = {s: "good" for s in stages}
    out = [("good", allGood, True), ("null-dst", allGood, False)]
    for i, s in enumerate(stages):
        out.append(("no-" + s, dict(allGood, **{s: None}), True))
        out.append(("bad-from-" + s, dict(allGood, **{t: "bad" for t in stages[i:]}), True))
    if "meter" in stages and "tone" in stages:
        out.append(("two-automatic-exposures", dict(allGood, tone="auto"), True))
    if "grade" in stages:
        out.append(("grade-regions", dict(allGood, grade="regions"), True))
    return out


def table(path):
    """[entry, case, return code, error text] of every row, from the library at `path`"""
    L = C.CDLL(path)
    L.kajo_hip_last_error.restype = C.c_char_p
    rows = []
    for entry, spec in ENTRIES.items():
        slots = spec.split()
        for name, plan, withDst in cases(slots):
            keep, args = [], []
            for slot in slots:
                if slot in ("h", "gathered"):
                    args.append(None)
                elif slot in STRUCTS:
                    if plan[slot] is None:
                        args.append(None)
                        continue
                    p = good(L, slot)
                    if plan[slot] == "bad":
                        spoil(slot, p)
                    elif plan[slot] == "auto":
                        p.flags = 1  # KAJO_TONE_AUTO_EXPOSURE
                    elif plan[slot] == "regions":
                        p.nRegions = 1
                        p.regions[0].n = 1
                        p.regions[0].objects[0] = 1
                    keep.append(p)
                    args.append(C.byref(p))
                else:  # dst, scale, result: room for whatever a call could write with no frame at hand
                    buf = (C.c_uint32 * 1024)()
                    keep.append(buf)
                    args.append(buf if (slot != "dst" or withDst) else None)
            rc = getattr(L, entry)(*args)
            rows.append([entry, name, rc, (L.kajo_hip_last_error() or b"").decode() if rc else ""])
    return rows


@pytest.fixture(scope="module")
def golden_rows():
    with open(GOLDEN) as f:
        return json.load(f)["rows"]


def test_the_table_covers_every_chain_entry_point(golden_rows):
    assert {r[0] for r in golden_rows} == set(ENTRIES)
    assert set(ENTRIES) <= set(capi.EXPORTS)
    chain = {n for n in capi.EXPORTS if n.startswith(("kajo_hip_present_", "kajo_hip_display_", "kajo_hip_tonemap_"))}
    assert chain <= set(ENTRIES), chain - set(ENTRIES)
    assert 200 <= len(golden_rows) <= 600
    assert all(r[2] != 0 for r in golden_rows)  # a null handle: every row is a refusal


@pytest.mark.parametrize("which", sorted(LIBS))
def test_refusals_are_the_recorded_ones(which, golden_rows):
    assert os.path.exists(LIBS[which]), LIBS[which]
    got = table(LIBS[which])
    assert len(got) == len(golden_rows)
    wrong = [(g, w) for g, w in zip(got, golden_rows) if g != w]
    assert not wrong, wrong[:10]
