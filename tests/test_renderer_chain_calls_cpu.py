"""The Python binding of the display chain (kajo_amd/capi.py STAGES / CHAIN_ENTRIES, kajo_amd/renderer.py HipRenderer) without a GPU.

a. A HipRenderer made without a device, its library replaced by a stand-in that records every chain call, is driven through present()
   over every subset of its optional stages, with and without an encode, and through the eight narrower methods: the entry called, the
   bytes of every parameter block handed over, the arrays returned and the second return value equal
   tests/golden/renderer_chain_calls.json row by row.
b. The argtypes / restype of every export equal the rendering kept in the same golden.
c. Every row of CHAIN_ENTRIES is its entry's prototype in include/kajo_hip.h.

The golden was recorded by record() from the binding as it stood before the entry points became a table: `python
tests/test_renderer_chain_calls_cpu.py [out.json]` with that kajo_amd first on the path (KAJO_HIP_LIB = a built library) writes it. It is
never written from the code under test."""
import ctypes as C
import itertools
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "renderer_chain_calls.json")
W, H = 70, 37

SCALE, TONE_SCALE = 1.5, 2.5  # what the stand-in writes through a `scale` pointer, and answers kajo_hip_tone_scale with
RESULT = dict(pixels=2590, nonfinite=1, under=2, over=3, metered=2584, anchorL=0.25, whiteL=4.0, exposure=-0.5, minBin=17, maxBin=400)

# every keyword of every builder, none at its default
FRONT = dict(
    despeckle=dict(factor=8.0, rank=2, floor=0.5),
    denoise=dict(iterations=3, sigma_luminance=2.5, sigma_normal=0.25, sigma_depth=0.75, demodulate=False, noise_guided=True),
    grade=dict(slope=[1.1, 0.9, 1.2], offset=0.05, power=[0.8, 1.0, 1.25], saturation=1.5, white_balance=[1.25, 1.0, 0.75],
               regions=[dict(objects=[3, 5], amount=0.5, slope=0.7, offset=[0.1, 0.0, -0.1], power=1.5, saturation=0.25)]),
    lens=dict(aperture=0.05, focus_distance=4.0, max_radius=9),
    glare=dict(levels=4, strength=0.25, threshold=1.5),
    local=dict(compression=0.4, detail=1.5, sigma_range=1.25, iterations=3, pivot=-1.5, metered=True, pivot_percentile=0.25),
    meter=dict(percentile=0.4, key=0.25, white_percentile=0.9, auto_white=True),
    view=dict(out_w=35, out_h=18, rect=(3.5, 2.0, 60.25, 30.5), filter="lanczos3"),
)
TONE = dict(curve="reinhard", exposure=0.75, white=3.0, auto_exposure=True, key=0.3)
ENCODES = (dict(format="rgba16f", transfer="srgb", scene=True, peak_nits=400.0, dither_seed=7),
           dict(format="rgb10a2", transfer="pq", dither=True, peak_nits=600.0, dither_seed=12345))


class Recorder:
    """Stands where HipRenderer keeps libkajo_hip.so: the host-only defaults go to the real library, every other call is written down
    and answered with success."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.startswith("kajo_hip_default_"):
            return getattr(self.real, name)
        if name == "kajo_hip_destroy":
            return lambda h: 0
        if name.startswith("kajo_"):
            return lambda *args: self.call(name, args)
        raise AttributeError(name)

    def call(self, name, args):
        seen = []
        for a in args:
            obj = getattr(a, "_obj", None)  # what byref() points at
            if a is None:
                seen.append(None)
            elif obj is None:  # a handle or a buffer: only that it is there
                seen.append("buffer" if (a.value if isinstance(a, C.c_void_p) else a) else None)
            elif isinstance(obj, C.c_float):
                obj.value = TONE_SCALE if name == "kajo_hip_tone_scale" else SCALE
                seen.append("float*")
            elif type(obj).__name__ == "KajoMeterResult":
                for k, v in RESULT.items():
                    setattr(obj, k, v)
                seen.append("KajoMeterResult*")
            else:
                seen.append("%s:%s" % (type(obj).__name__, bytes(obj).hex()))
        self.calls.append([name] + seen)
        return 0


def _plain(x):
    """a return value as JSON keeps it"""
    if isinstance(x, np.ndarray):
        return {"shape": list(x.shape), "dtype": str(x.dtype)}
    if isinstance(x, (tuple, list)):
        return [_plain(v) for v in x]
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    return x if x is None or isinstance(x, (str, bool)) else (int(x) if isinstance(x, (int, np.integer)) else float(x))


def _type_name(t):
    return None if t is None else t.__name__


def record():
    """{"calls": [[label, the library calls made, the value returned or the exception raised], ...], "argtypes": {export: [argtypes,
    restype]}} of the kajo_amd that is importable"""
    from kajo_amd import capi, renderer

    r = renderer.HipRenderer.__new__(renderer.HipRenderer)
    r.width, r.height, r._h = W, H, C.c_void_p(1)
    r._L = rec = Recorder(capi.lib())
    rows = []

    def run(label, fn, *args, **kw):
        rec.calls = []
        try:
            got = _plain(fn(*args, **kw))
        except Exception as e:  # (the refusals the binding itself makes)
            got = "%s: %s" % (type(e).__name__, e)
        rows.append([label, rec.calls, got])

    names = sorted(FRONT)
    for n in range(len(names) + 1):
        for subset in itertools.combinations(names, n):
            stages = {s: FRONT[s] for s in subset}
            run("present " + " ".join(subset), r.present, **stages, **TONE)
            for e in ENCODES:
                run("present %s encode=%s" % (" ".join(subset), e["format"]), r.present, encode=e, **stages, **TONE)
    front = lambda *stages: {s: FRONT[s] for s in stages}
    for label, kw in (("defaults", {}), ("tone only", TONE)):
        run("present " + label, r.present, **kw)
    run("tonemap", r.tonemap)
    run("tonemap all", r.tonemap, **TONE, **front("denoise"))
    run("glare", r.glare)
    run("glare all", r.glare, **FRONT["glare"], **front("denoise"))
    run("display", r.display)
    run("display all", r.display, **front("denoise", "glare"), **TONE)
    run("meter", r.meter)
    run("meter all", r.meter, **front("despeckle", "denoise", "glare"), **FRONT["meter"])
    run("local", r.local)
    run("local all", r.local, **front("despeckle", "denoise", "glare"), **FRONT["local"])
    run("lens", r.lens)
    run("lens all", r.lens, **front("despeckle", "denoise"), **FRONT["lens"])
    run("grade", r.grade)
    run("grade all", r.grade, **front("despeckle", "denoise"), **FRONT["grade"])
    run("encode", r.encode)
    run("encode view", r.encode, view=dict(out_w=20))
    for e in ENCODES:
        run("encode all %s" % e["format"], r.encode, encode=e, **TONE)
        run("encode all %s view" % e["format"], r.encode, encode=e, view=FRONT["view"], **TONE)
    # the refusals that never reach the library
    run("tonemap unknown curve", r.tonemap, curve="filmic")
    run("present unknown curve", r.present, curve="filmic", **front("glare"))
    run("encode unknown curve", r.encode, curve="filmic")
    run("view wrong shape", r.view, np.zeros((H, W + 1), np.uint32))
    run("encode_pixels unknown curve", renderer.encode_pixels, np.zeros((4, 3), np.float32), curve="filmic")
    run("encode_view_pixels unknown curve", renderer.encode_view_pixels, np.zeros((4, 4, 3), np.float32), curve="filmic")
    r._h = None

    L = capi.lib()
    argtypes = {}
    for name in capi.EXPORTS:
        f = getattr(L, name)
        argtypes[name] = [None if f.argtypes is None else [_type_name(t) for t in f.argtypes], _type_name(f.restype)]
    return {"calls": rows, "argtypes": argtypes}


def _packed(table):
    """the parameter blocks repeat from row to row: the file keeps each once, the calls name them by index"""
    blocks, index = [], {}
    for _, calls, _ in table["calls"]:
        for call in calls:
            for i, a in enumerate(call):
                if isinstance(a, str) and ":" in a:
                    if a not in index:
                        index[a] = len(blocks)
                        blocks.append(a)
                    call[i] = "@%d" % index[a]
    return dict(table, blocks=blocks)


def _unpacked(table):
    blocks = table["blocks"]
    for _, calls, _ in table["calls"]:
        for call in calls:
            call[:] = [blocks[int(a[1:])] if isinstance(a, str) and a.startswith("@") else a for a in call]
    return table


def _golden():
    with open(GOLDEN) as f:
        return _unpacked(json.load(f))


def test_the_binding_makes_the_recorded_calls():
    from kajo_amd import capi

    want = _golden()["calls"]
    got = json.loads(json.dumps(record()["calls"]))  # (tuples become lists, as in the file)
    assert len(want) >= 520
    called = {call[0] for _, calls, _ in got for call in calls}
    assert called <= set(capi.CHAIN_ENTRIES) | {"kajo_hip_tone_scale"}, called - set(capi.CHAIN_ENTRIES)
    assert not {"kajo_hip_display_argb8", "kajo_hip_tonemap_argb8"} & {call[0] for label, calls, _ in got if label.startswith("present")
                                                                          for call in calls}
    assert [row[0] for row in got] == [row[0] for row in want]
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "%d rows differ; the first (got, recorded): %r" % (len(wrong), wrong[:3])


def test_argtypes_are_the_recorded_ones():
    from kajo_amd import capi

    want = _golden()["argtypes"]
    got = json.loads(json.dumps(record()["argtypes"]))
    for name in list(capi.CHAIN_ENTRIES) + ["kajo_hip_default_%s_params" % s for s in capi.STAGES]:
        assert got[name][0] is not None, name
        assert got[name] == want[name], (name, got[name], want[name])
    wrong = {n: (got.get(n), want[n]) for n in want if got.get(n) != want[n]}  # and nothing else moved either
    assert not wrong and set(got) == set(want), wrong


def _prototype(header, name):
    """the parameters of an entry point as include/kajo_hip.h declares it"""
    m = re.search(r"^int %s\((.*?)\);" % re.escape(name), header, re.M | re.S)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _prototype_slots(header, name):
    """the same in the table's notation"""
    slots = []
    for param in _prototype(header, name):
        stage = re.fullmatch(r"const Kajo(\w+)Params\* \w+", param)
        if param == "kajo_hip_t h":
            slots.append("h")
        elif param == "const void* gathered":
            slots.append("gathered")
        elif stage:
            slots.append(stage.group(1).lower())
        elif param == "float* scale":
            slots.append("scale")
        elif param == "KajoMeterResult* result":
            slots.append("result")
        else:
            assert re.fullmatch(r"(uint32_t|float|void)\* \w+", param), (name, param)
            slots.append("dst")
    return slots


def test_the_table_is_the_headers():
    from kajo_amd import capi
    from test_chain_refusals_cpu import ENTRIES

    with open(os.path.join(ROOT, "include", "kajo_hip.h")) as f:
        header = f.read()
    assert list(capi.STAGES) == "despeckle denoise grade lens glare local meter tone view encode".split()
    assert len(capi.CHAIN_ENTRIES) == 26
    where = []
    for name, row in capi.CHAIN_ENTRIES.items():
        slots, proto = row.split(), _prototype_slots(header, name)
        assert [s for s in proto if s in capi.STAGES] == [s for s in slots if s in capi.STAGES], name
        assert ("gathered" in slots) == (proto[1] == "gathered"), name
        tail = lambda s: [x for x in s if x in ("dst", "scale", "result")]
        assert tail(proto) == tail(slots) == slots[-len(tail(slots)):], name
        assert slots == proto, name
        assert getattr(capi.lib(), name).argtypes is not None, name
        where.append(header.index("\nint %s(" % name))
    assert where == sorted(where)  # the header's order
    assert {n: capi.CHAIN_ENTRIES[n] for n in ENTRIES} == ENTRIES
    assert set(capi.CHAIN_ENTRIES) <= set(capi.EXPORTS)
    chain = {n for n in capi.EXPORTS if n.startswith(("kajo_hip_present_", "kajo_hip_display_", "kajo_hip_tonemap_"))}
    chain |= {n for n in capi.EXPORTS if n.startswith("kajo_hip_encode") and _prototype(header, n)[0] == "kajo_hip_t h"}
    assert chain <= set(capi.CHAIN_ENTRIES), chain - set(capi.CHAIN_ENTRIES)
    assert set(capi.CHAIN_ENTRIES) - set(ENTRIES) == {n for n in chain if n.startswith("kajo_hip_encode")}


if __name__ == "__main__":
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as out:
        json.dump(_packed(record()), out, separators=(",", ":"))
        out.write("\n")
