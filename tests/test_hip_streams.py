"""The caller's-stream contract of include/kajo_hip.h on the GPU: every entry point the header calls asynchronous runs on the stream
kajo_hip_set_stream gave the handle and is ordered by it alone; every entry point that waits, waits for that stream. bench.py and
hip::Scheduler put render, gather, compose / resolve and the display chain on one stream of their own and rely on exactly this.

A launch, memset or copy that slipped onto the null stream or a stale stream still gives the right image while the device is idle,
which in every other module it is. Here a device-side spin (torch.cuda._sleep, as tests/test_hip_view.py) stands on the caller's
stream S in front of the calls, so that such a slip reads the PREVIOUS frame -- the poison: the same owners' tile buffers after another
pass count, which is also what every scratch buffer of the handle holds when a case starts -- and gives other words. Every case first
shows that the poison's image differs from the true one, and carries a guard: an event recorded behind the spin must still be
incomplete at the moment named in the case ("spin ended early" otherwise: a failure, not a skip). Compares are exact on words and
result bytes; the expected values are computed once per numerics build on the handles' own streams, waited, device idle.

  A  late input     spin; G.copy_(true) over the poison; the call; out.clone() -- all on S, then S.synchronize() only. The three-owner
                    root with a gathered tensor, and one owner with gathered = NULL whose own tile buffers are G.
  B  late render    spin; render() without wait(); then one waiting reader, or one asynchronous twin with gathered = NULL
  C  switching      set_stream orders the old stream; the null stream and back; close() leaves the caller's stream alone; two calls
                    with different view / grade parameters back to back reuse the pinned staging block
  D  no host wait   the guard of A and B is taken when the call RETURNS wherever the header says "asynchronous ... no host
                    synchronisation": the resolve, tonemap, display, present, metered (meter NULL) and local (no metered pivot) twins,
                    the view and grade twins once their scratch stands, kajo_hip_resolve_argb8_device, kajo_hip_compose_aov and
                    kajo_hip_render. Where the header says the call waits once (a meter, KAJO_LOCAL_PIVOT_METERED) it is taken before.

The frame is 70 x 37 (ragged against the 64 x 16 tile on both axes), spheres_a169, 4 samples per pass; the stage parameters are
tests/test_hip_chain.py's, none of them the identity; EXACT (the default build and the benchmark's) and STRICT."""
import ctypes as C

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, view_weights
from test_hip_chain import GATHERED, H, OUT_H, OUT_W, STAGES, W, call_host, call_meter, ref, stage_params, words_of

pytestmark = pytest.mark.gpu

BUILDS = {"exact": dict(exact=True), "strict": dict(strict=True)}
SPIN_CYCLES = 20_000_000  # tests/test_hip_view.py's: device time hundreds of times what enqueueing a chain takes; not a tolerance
RESOLVE = "kajo_hip_resolve_gathered_argb8_device"
METERED = "kajo_hip_present_metered_gathered_argb8_device"
LOCAL = "kajo_hip_present_local_gathered_argb8_device"
VIEW = "kajo_hip_present_view_gathered_argb8_device"
GRADE = "kajo_hip_present_grade_gathered_argb8_device"
# name -> (entry point, the stages given, the parameter set, the header says it waits once)
TWINS = {
    "resolve": (RESOLVE, (), "chain", False),
    "tonemap": ("kajo_hip_tonemap_gathered_argb8_device", ("tone",), "chain", False),
    "display": ("kajo_hip_display_gathered_argb8_device", ("glare", "tone"), "chain", False),
    "present": ("kajo_hip_present_gathered_argb8_device", ("despeckle", "glare", "tone"), "chain", False),
    "metered-null": (METERED, ("despeckle", "glare", "tone"), "chain", False),
    "metered": (METERED, ("despeckle", "glare", "meter", "tone"), "chain", True),
    "local": (LOCAL, ("despeckle", "glare", "local", "tone"), "chain", False),
    "local-pivot": (LOCAL, ("despeckle", "glare", "local", "tone"), "pivot", True),
    "view": (VIEW, ("despeckle", "glare", "local", "tone", "view"), "chain", False),
    "grade": (GRADE, ("despeckle", "grade", "glare", "local", "tone", "view"), "chain", False),
}
# Two views and two grades for the staging blocks (C 4). The views differ in filter and rectangle but share their layout -- the output
# size, the longest row of either axis -- and the second one's source rows lie inside the first one's: rows of one read through the
# other's geometry name pixels inside the image, so a slip here is a wrong image and never a wild read (test_the_two_views_share_a_layout)
VIEW_A = dict(out_w=20, out_h=10, rect=(0.25, 0.25, 60.25, 30.25), filter="triangle")
VIEW_B = dict(out_w=20, out_h=10, rect=(5.25, 3.25, 25.25, 13.25), filter="lanczos3")
SLOPE_A, SLOPE_B = (1.25, 1.0, 0.75), (0.5, 1.5, 1.0)
OUT_WORDS = (W * H, OUT_W * OUT_H, VIEW_A["out_w"] * VIEW_A["out_h"])  # the sizes of the images the twins write


def torch_():
    import torch
    return torch


def tensor_of(ptr, nbytes):
    from bench import DevicePtr
    return torch_().as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda")


def words(t):
    return t.cpu().numpy().view(np.uint32)


def same(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


class Spin:
    """A spinning kernel on `stream` and an event directly behind it"""

    def __init__(self, stream):
        torch = torch_()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(SPIN_CYCLES)
        self.event = torch.cuda.Event()
        self.event.record(stream)

    def running(self):
        return not self.event.query()


class Config:
    """A root handle and the buffers its calls read: G = (accumulation, AOV, matte) tile buffers as the calls are handed them; `frames`
    = their true and poison contents; src = the pointers passed (None: the handle's own buffers, which G then is)"""

    def __init__(self, root, G=None, frames=None, src=(None, None, None)):
        torch = torch_()
        self.root, self.G, self.frames, self.src = root, G, frames, src
        self.outs = {n: torch.zeros(n, dtype=torch.int32, device="cuda") for n in OUT_WORDS}
        self.want, self.poison = {}, {}

    def load(self, which, stream=None):
        """G <- the true or the poison buffers, on `stream` (None: now, waited)"""
        torch = torch_()
        if stream is None:
            for g, f in zip(self.G, self.frames[which]):
                g.copy_(f)
            torch.cuda.synchronize()
        else:
            with torch.cuda.stream(stream):
                for g, f in zip(self.G, self.frames[which]):
                    g.copy_(f)


# ---- the cases of A: enqueue() makes the asynchronous call(s), finish() reads every copy of the result ------------------------------

class Twin:
    def __init__(self, name):
        self.entry, self.stages, self.params, self.waits = TWINS[name]

    def enqueue(self, world, cfg, p=None):
        p = p or world.params[self.params]
        n = p["view"].outW * p["view"].outH if "view" in self.stages else W * H
        out, res = cfg.outs[n], capi.KajoMeterResult()
        src = None if cfg.src[0] is None else C.c_void_p(cfg.src[0])
        args = [cfg.root._h, src]
        if self.entry != RESOLVE:
            args += [ref(p, self.stages, s) for s in GATHERED[self.entry]]
        args.append(C.c_void_p(out.data_ptr()))
        if self.entry != RESOLVE and "meter" in GATHERED[self.entry]:
            args.append(C.byref(res))
        capi.check(getattr(capi.lib(), self.entry)(*args))
        return out, res

    def finish(self, world, cfg, state, stream):
        """the results to compare: idle (stream None) the output; else the output and a copy torch made behind the call on `stream`,
        after that stream alone was waited for"""
        torch = torch_()
        out, res = state
        if stream is None:
            cfg.root.wait()
            torch.cuda.synchronize()
            return [(words(out), bytes(res))]
        with torch.cuda.stream(stream):
            copy = out.clone()
        stream.synchronize()
        return [(words(out), bytes(res)), (words(copy), bytes(res))]


class Compose:
    """kajo_hip_compose, then kajo_hip_read_radiance, which waits"""
    waits = False

    def enqueue(self, world, cfg, p=None):
        cfg.root.compose(cfg.G[0].data_ptr())

    def finish(self, world, cfg, state, stream):
        return [cfg.root.radiance()]


class ComposeAov:
    """kajo_hip_compose_aov, then kajo_hip_read_aov and kajo_hip_read_matte, which wait"""
    waits = False

    def enqueue(self, world, cfg, p=None):
        cfg.root.compose_aov(cfg.src[1], cfg.src[2])

    def finish(self, world, cfg, state, stream):
        a, m = cfg.root.aov(), cfg.root.matte()
        return [(a["raw"][0], a["raw"][1], a["samples"], m["ids"], m["counts"], m["samples"])]


CASES = dict({name: Twin(name) for name in TWINS}, compose=Compose(), compose_aov=ComposeAov())


def idle(world, cfg, case, p=None):
    return case.finish(world, cfg, case.enqueue(world, cfg, p), None)[0]


# ---- the readers of B: each waits by itself ------------------------------------------------------------------------------------------

def _noise(r):
    n = r.noise()
    return tuple(n[k] for k in ("mean", "stderr", "relative", "batches", "hist", "pixels", "known", "unknown", "bad", "quantile_value"))


def _counters(r):
    c = r.counters()
    return tuple(c[k] for k in ("passes", "paths", "launches", "traversals", "vertices"))  # (kernelMs is a time)


def _despeckle(r):
    d = r.despeckle()
    return d["radiance"], d["clamped"], d["repaired"]


def _matte(r):
    m = r.matte()
    return m["ids"], m["counts"], m["samples"]


def _aov(r):
    a = r.aov()
    return a["raw"][0], a["raw"][1], a["samples"]


def _meter(world, r):
    rc, hist, res = call_meter(r._h, world.params["chain"])
    return rc, hist, bytes(res)


def _pinned(world, r, what):
    """kajo_hip_read_radiance / kajo_hip_resolve_argb8 into page-locked host memory, where the copy itself does not hold the host up:
    the words are there when the call returns only if the call waited for the handle's stream"""
    t = world.pinned[what]
    fn = capi.lib().kajo_hip_read_radiance if what == "radiance" else capi.lib().kajo_hip_resolve_argb8
    capi.check(fn(r._h, C.c_void_p(t.data_ptr())))
    return t.numpy().copy()


READERS = {
    "read_radiance": lambda world, r: r.radiance(),
    "read_radiance-pinned": lambda world, r: _pinned(world, r, "radiance"),
    "resolve_argb8-pinned": lambda world, r: _pinned(world, r, "argb8"),
    "resolve_argb8": lambda world, r: r.argb8(),
    "read_aov": lambda world, r: _aov(r),
    "read_matte": lambda world, r: _matte(r),
    "present_grade_argb8": lambda world, r: call_host(r._h, "kajo_hip_present_grade_argb8", STAGES, world.params["chain"]),
    "despeckle": lambda world, r: _despeckle(r),
    "meter": _meter,
    "counters": lambda world, r: _counters(r),
}
NOISE_READERS = {"read_noise_moments": lambda world, r: r.noise_moments(), "noise": lambda world, r: _noise(r)}


class World:
    pass


def _snapshot(handles):
    """the handles' (accumulation, AOV, matte) tile buffers side by side, as a gather leaves them"""
    torch = torch_()
    parts = ([], [], [])
    for o in handles:
        o.wait()
        ptr, nbytes = o.tile_buffer()
        aov, aov_bytes, matte, matte_bytes = o.aov_tile_buffers()
        for k, (p, n) in enumerate(((ptr, nbytes), (aov, aov_bytes), (matte, matte_bytes))):
            parts[k].append(tensor_of(p, n).clone())
    torch.cuda.synchronize()  # (the handles run on streams of their own)
    frames = tuple(torch.cat(p) for p in parts)
    torch.cuda.synchronize()
    return frames


def _late_schedule(r, first, second):
    """the frame of B and C: `first` passes, waited -- the previous frame --, then `second` more"""
    r.reset()
    r.render(first).wait()
    r.render(second).wait()


def _view_pair(root):
    return root._view_params(**VIEW_A), root._view_params(**VIEW_B)


def _staging_params(world, root, which):
    """the parameter sets of C 4: the chain's, with the two views or the two global ops"""
    out = []
    for k in range(2):
        p = stage_params()
        if which == "view":
            p["view"] = _view_pair(root)[k]
        else:
            p["grade"].global_.slope[:] = (SLOPE_A, SLOPE_B)[k]
        out.append(p)
    return out


def _build_world(scenes, build):
    torch = torch_()
    sc, kw = scenes["spheres_a169"], BUILDS[build]
    world = World()
    world.handles = []

    def make(**more):
        r = HipRenderer(sc, W, H, spp=4, **more, **kw)
        world.handles.append(r)
        return r

    world.params = dict(chain=stage_params(), pivot=stage_params())
    world.params["pivot"]["local"].flags = capi.KAJO_LOCAL_PIVOT_METERED
    tiled = dict(aov=True, matte=True, aov_tiled=True)
    owners = [make(tile_index=k, tile_count=3, **tiled) for k in range(3)]
    one = make(**tiled)
    world.plain = make(aov=True, matte=True, counters=True)
    world.noisy = make(noise=True)
    # A: the poison is the frame of one pass, the true frame that of two; every root has rendered two
    world.configs = {}
    for name, handles in (("owners3", owners), ("owner1", [one])):
        for o in handles:
            o.render(1)
        poison = _snapshot(handles)
        for o in handles:
            o.render(1)
        true = _snapshot(handles)
        if len(handles) > 1:
            G = tuple(torch.empty_like(t) for t in true)
            src = tuple(g.data_ptr() for g in G)
        else:
            aov, aov_bytes, matte, matte_bytes = one.aov_tile_buffers()
            G = (tensor_of(*one.tile_buffer()), tensor_of(aov, aov_bytes), tensor_of(matte, matte_bytes))
            src = (None, None, None)
        world.configs[name] = cfg = Config(handles[0], G, dict(true=true, poison=poison), src)
        for which, into in (("true", cfg.want), ("poison", cfg.poison)):  # (the poison last: it stands in every scratch buffer)
            cfg.load(which)
            for case in CASES:
                into[case] = idle(world, cfg, CASES[case])
            if name == "owners3":
                for kind in ("view", "grade"):
                    into["staging-" + kind] = [idle(world, cfg, CASES[kind], p) for p in _staging_params(world, cfg.root, kind)]
    # B, C: two passes behind one (the noise estimate: two batches of four behind one)
    world.late = Config(world.plain)
    world.pinned = dict(radiance=torch.empty(W * H * 4, dtype=torch.float32, pin_memory=True),
                        argb8=torch.empty(W * H, dtype=torch.int32, pin_memory=True))
    _late_schedule(world.plain, 1, 1)
    for name in READERS:
        world.late.want[name] = READERS[name](world, world.plain)
    for name in TWINS:
        world.late.want[name] = idle(world, world.late, CASES[name])
    out = world.late.outs[W * H]
    capi.check(capi.lib().kajo_hip_resolve_argb8_device(world.plain._h, C.c_void_p(out.data_ptr())))
    world.plain.wait()
    torch.cuda.synchronize()
    world.late.want["resolve_argb8_device"] = words(out)
    _late_schedule(world.noisy, 4, 4)
    for name in NOISE_READERS:
        world.late.want[name] = NOISE_READERS[name](world, world.noisy)
    world.ramp = torch.arange(1000, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # from here on every handle is on the caller's stream
    world.S, world.S2 = torch.cuda.Stream(), torch.cuda.Stream()
    for r in world.handles:
        r.set_stream(world.S.cuda_stream)
    return world


@pytest.fixture(scope="module", params=sorted(BUILDS))
def world(request, scenes):
    w = _build_world(scenes, request.param)
    yield w
    torch_().cuda.synchronize()
    for r in w.handles:
        r.close()


def _settle(world):
    torch_().cuda.synchronize()


# ---- A and D -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("config", ["owners3", "owner1"])
def test_late_input_is_waited_for_on_the_caller_s_stream(world, config, case):
    cfg, c, S = world.configs[config], CASES[case], world.S
    assert not same(cfg.poison[case], cfg.want[case]), "the poison gives the true frame's output: the case would show nothing"
    try:
        # the previous frame, through the same call on S: it stands in G, in the output and in every scratch buffer of the chain, and the
        # view's and the grade's scratch stands for these parameters
        cfg.load("poison", S)
        before = c.finish(world, cfg, c.enqueue(world, cfg), S)
        spin = Spin(S)
        cfg.load("true", S)
        early = spin.running()
        state = c.enqueue(world, cfg)
        returned = spin.running()
        got = c.finish(world, cfg, state, S)
    finally:
        _settle(world)
    assert all(same(b, cfg.poison[case]) for b in before), "the previous frame on the caller's stream"
    assert early, "spin ended early: it was over before the call was made"
    if not c.waits:
        assert returned, "spin ended early, or the call waited for the stream: it was over when the call returned"
    for g in got:
        assert same(g, cfg.want[case]), (config, case)


# ---- B and D -------------------------------------------------------------------------------------------------------------------------

def _late_render(world, r, first, second, read):
    """read() of the previous frame, waited; then read() directly behind a spin and an un-waited render of `second` more passes"""
    try:
        r.reset()
        r.render(first).wait()
        stale = read()
        spin = Spin(world.S)
        r.render(second)
        rendered = spin.running()
        got = read()
    finally:
        _settle(world)
    return stale, rendered, got


@pytest.mark.parametrize("reader", sorted(READERS) + sorted(NOISE_READERS))
def test_readers_wait_for_a_late_render(world, reader):
    noisy = reader in NOISE_READERS
    r, passes = (world.noisy, 4) if noisy else (world.plain, 1)
    read = (NOISE_READERS if noisy else READERS)[reader]
    want = world.late.want[reader]
    stale, rendered, got = _late_render(world, r, passes, passes, lambda: read(world, r))
    assert not same(stale, want), "the previous frame reads as the true one: the case would show nothing"
    assert rendered, "spin ended early, or kajo_hip_render waited for the stream: it was over when render() returned"
    assert same(got, want), reader


def _resolve_device(world, r, out):
    capi.check(capi.lib().kajo_hip_resolve_argb8_device(r._h, C.c_void_p(out.data_ptr())))


@pytest.mark.parametrize("twin", sorted(TWINS) + ["resolve_argb8_device"])
def test_one_owner_twins_run_behind_a_late_render(world, twin):
    cfg, S, r = world.late, world.S, world.late.root
    want = cfg.want[twin]

    def run(spin):
        """the twin on S -> (every copy of its result, the spin was still running when the call returned)"""
        if twin == "resolve_argb8_device":
            out = cfg.outs[W * H]
            _resolve_device(world, r, out)
            returned = spin is not None and spin.running()
            S.synchronize()
            return [words(out)], returned
        state = CASES[twin].enqueue(world, cfg)
        returned = spin is not None and spin.running()
        return CASES[twin].finish(world, cfg, state, S), returned

    try:
        r.reset()
        r.render(1).wait()
        stale, _ = run(None)
        spin = Spin(S)
        r.render(1)
        rendered = spin.running()
        got, returned = run(spin)
    finally:
        _settle(world)
    assert not same(stale[0], want), "the previous frame reads as the true one: the case would show nothing"
    assert rendered, "spin ended early, or kajo_hip_render waited for the stream: it was over when render() returned"
    if twin == "resolve_argb8_device" or not CASES[twin].waits:
        assert returned, "spin ended early, or the call waited for the stream: it was over when the call returned"
    for g in got:
        assert same(g, want), twin


# ---- C -------------------------------------------------------------------------------------------------------------------------------

def test_set_stream_orders_the_old_stream(world):
    """C 1: a render behind a spin on S, then set_stream(S2) and a resolve on S2, and only S2 is waited for"""
    r, S, S2 = world.plain, world.S, world.S2
    out, want = world.late.outs[W * H], world.late.want["resolve_argb8_device"]
    try:
        r.reset()
        r.render(1).wait()
        _resolve_device(world, r, out)
        S.synchronize()
        stale = words(out)
        spin = Spin(S)
        r.render(1)
        rendered = spin.running()
        r.set_stream(S2.cuda_stream)
        _resolve_device(world, r, out)
        S2.synchronize()
        got = words(out)
    finally:
        _settle(world)
        r.set_stream(S.cuda_stream)
    assert not same(stale, want), "the previous frame reads as the true one: the case would show nothing"
    assert rendered, "spin ended early: it was over when render() returned"
    assert same(got, want)


def test_the_null_stream_and_back(world):
    """C 2: set_stream(NULL) behind work on S, calls on the null stream, S again"""
    r, S = world.plain, world.S
    out, want = world.late.outs[W * H], world.late.want["resolve_argb8_device"]
    try:
        r.reset()
        r.render(1).wait()
        spin = Spin(S)
        r.render(1)
        rendered = spin.running()
        r.set_stream(None)
        on_null = r.argb8().reshape(-1)
        radiance = r.radiance()
        r.set_stream(S.cuda_stream)
        spin = Spin(S)
        _resolve_device(world, r, out)
        returned = spin.running()
        S.synchronize()
        back = words(out)
        again = r.radiance()
    finally:
        _settle(world)
        r.set_stream(S.cuda_stream)
    assert rendered and returned, "spin ended early"
    assert same(on_null, want) and same(back, want)
    assert same(radiance, world.late.want["read_radiance"]) and same(again, radiance)


def test_close_leaves_the_caller_s_stream_alone(world, scenes):
    """C 3: a handle closed behind late work on the stream it was given; the stream still runs the caller's work"""
    torch = torch_()
    S = world.S
    try:
        r = HipRenderer(scenes["spheres_a169"], W, H, spp=4, **BUILDS["exact"])
        r.set_stream(S.cuda_stream)
        spin = Spin(S)
        r.render(1)
        rendered = spin.running()
        r.close()
        with torch.cuda.stream(S):
            tripled = world.ramp * 3
        S.synchronize()
        done = S.query()
    finally:
        _settle(world)
    assert rendered, "spin ended early: it was over when render() returned"
    assert done and np.array_equal(tripled.cpu().numpy(), np.arange(1000, dtype=np.int32) * 3)


def test_the_two_views_share_a_layout():
    """(host only) what VIEW_A and VIEW_B are chosen for: the same output size and longest rows, B's source rows inside A's"""
    axes = []
    for v in (VIEW_A, VIEW_B):
        x0, y0, x1, y1 = v["rect"]
        axes.append((view_weights(W, x0, x1, v["out_w"], v["filter"]), view_weights(H, y0, y1, v["out_h"], v["filter"])))
    (ax, ay), (bx, by) = axes
    assert ax[2].shape == bx[2].shape and ay[2].shape == by[2].shape
    assert ay[0].min() <= by[0].min() and (by[0] + by[1]).max() <= (ay[0] + ay[1]).max()
    assert not np.array_equal(ax[2], bx[2]) and not np.array_equal(ay[2], by[2])


@pytest.mark.parametrize("kind", ["view", "grade"])
def test_two_parameter_sets_back_to_back_through_the_staging_block(world, kind):
    """C 4: behind one spin, two view (or grade) twin calls with different parameters. The second may wait for the first one's upload to
    leave the pinned staging block (include/kajo_hip.h); both images are those of their own parameters"""
    torch = torch_()
    cfg, c, S = world.configs["owners3"], CASES[kind], world.S
    want = cfg.want["staging-" + kind]
    assert not same(want[0], want[1]), "the two parameter sets give one image: the case would show nothing"
    params = _staging_params(world, cfg.root, kind)
    n = words_of(c.stages) if kind == "grade" else VIEW_A["out_w"] * VIEW_A["out_h"]
    first = torch.zeros(n, dtype=torch.int32, device="cuda")
    try:
        cfg.load("true", S)
        S.synchronize()
        torch.cuda.synchronize()
        spin = Spin(S)
        out, res = c.enqueue(world, cfg, params[0])
        pending = spin.running()
        with torch.cuda.stream(S):
            first.copy_(out)  # (both calls write cfg.outs[n])
        out, res = c.enqueue(world, cfg, params[1])
        S.synchronize()
        got = [(words(first), bytes(res)), (words(out), bytes(res))]
    finally:
        _settle(world)
    assert pending, "spin ended early: it was over when the first call returned"
    assert same(got[0], want[0]) and same(got[1], want[1])
