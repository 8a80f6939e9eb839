"""Tiled AOVs (KAJO_FLAG_AOV_TILED, include/kajo_hip.h kajo_hip_compose_aov) on the GPU: owners that keep the AOV sums and coverage tables of
their own tiles, gathered side by side and composed on owner 0, give the words of the one-owner handle without the flag -- the AOVs, the
mattes, the denoised frame and the display chain -- for 1, 2, 3 and 8 owners, tiles cut by the frame's edges, an owner without a tile;
the state rules of the readers; and the driver's --aov-tiled. Every comparison is on the bits (uint32 views)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import bits
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import stress_scene
from kajo_amd.tiles import TileLayout

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
SEED = 0o715517
SPP = 4  # n = 2
OWNERS = (1, 2, 3, 8)
# (W, H, tile): the frame's edges cut tiles; 130x70 in 64x16 tiles is 15 tiles, so that with 8 owners one owner has a single tile
FRAMES = [(130, 70, (64, 16)), (130, 70, (32, 8)), (72, 130, (8, 32))]
FLAGS = [dict(), dict(aov_specular=True), dict(matte=True), dict(matte=True, aov_specular=True)]
BUILDS = {"strict": dict(strict=True), "exact": dict(exact=True), "fast": dict()}
OBJECTS = [3, 4, 7]


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _cat(buffers):
    """Device buffers (ptr, bytes) side by side on the device, as a gather leaves them (torch tensor)."""
    import torch
    from bench import DevicePtr
    parts = [torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").clone() for ptr, nbytes in buffers]
    torch.cuda.synchronize()  # (the handles run on streams of their own)
    g = torch.cat(parts)
    torch.cuda.synchronize()
    return g


def _compose(owners, matte=True):
    """Gather the owners' tile buffers and compose the frame and the AOVs on owner 0. Returns the gathered tensors (kept alive by the caller
    until the reads are done)."""
    for o in owners:
        o.wait()
    root = owners[0]
    frame = _cat([o.tile_buffer() for o in owners])
    bufs = [o.aov_tile_buffers() for o in owners]
    aov = _cat([(b[0], b[1]) for b in bufs])
    tables = _cat([(b[2], b[3]) for b in bufs]) if (matte and bufs[0][2]) else None
    root.compose(frame.data_ptr())
    root.compose_aov(aov.data_ptr(), None if tables is None else tables.data_ptr())
    return frame, aov, tables


def _render(owners):
    for o in owners:
        o.render(1)
    for o in owners:
        o.render(1)


def _results(r, matte):
    """Everything the AOV readers give on a handle, as a dict of arrays."""
    a = r.aov()
    out = {"A": a["raw"][0], "B": a["raw"][1], "samples": np.array([a["samples"]], np.int64)}
    if matte:
        m = r.matte()
        mask, dominant = r.matte_mask(OBJECTS)
        out.update(ids=m["ids"], counts=m["counts"], matte_samples=np.array([m["samples"]], np.int64), mask=mask, dominant=dominant)
    d = r.denoise()
    out.update(denoised=d["radiance"], denoised_argb8=d["argb8"])
    return out


def _tiled(sc, W, H, tile, n, build, **flags):
    return [HipRenderer(sc, W, H, spp=SPP, seed=SEED, tile=tile, aov=True, aov_tiled=True, tile_index=i, tile_count=n, **build, **flags)
            for i in range(n)]


def _close(owners):
    for o in owners:
        o.close()


def _untiled(sc, W, H, tile, build, **flags):
    with HipRenderer(sc, W, H, spp=SPP, seed=SEED, tile=tile, aov=True, **build, **flags) as r:
        _render([r])
        return _results(r, flags.get("matte", False)), r.aov_kernel()


def _tiled_results(sc, W, H, tile, n, build, **flags):
    owners = _tiled(sc, W, H, tile, n, build, **flags)
    try:
        _render(owners)
        keep = _compose(owners)
        res = _results(owners[0], flags.get("matte", False))
        kernel = owners[0].aov_kernel()
        del keep
        return res, kernel
    finally:
        _close(owners)


def _assert_same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert same(got[k], want[k]), (what, k, int((bits(got[k]) != bits(want[k])).sum()))


@pytest.mark.parametrize("build", ["strict", "exact"])
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "+".join(sorted(f)) or "aov")
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d_tile%dx%d" % (f[0], f[1], f[2][0], f[2][1]))
def test_owners_do_not_matter(scenes, frame, flags, build):
    """STRICT and EXACT: the composed AOVs, mattes and denoised frame of 1, 2, 3 and 8 tiled owners are the untiled handle's, bit for bit."""
    W, H, tile = frame
    sc = scenes["spheres_a169"]  # (mirror wall and glass ball: the chain of aov_specular has work)
    want, kernel = _untiled(sc, W, H, tile, BUILDS[build], **flags)
    assert want["samples"][0] == 2 * SPP
    assert want["A"][..., 3].any() and np.isfinite(want["denoised"]).any()  # (the frame has hits: equal buffers are not empty ones)
    for n in OWNERS:
        got, k = _tiled_results(sc, W, H, tile, n, BUILDS[build], **flags)
        assert k == kernel  # (the same instance: the tiled shape is an argument of the launch)
        _assert_same(got, want, (n, build))


@pytest.mark.parametrize("build", ["strict", "exact"])
@pytest.mark.parametrize("which", ["biglist", "big"])
def test_owners_do_not_matter_in_the_large_scene_instances(scenes, which, build):
    """The _biglist and _big instances (the grid scenes of tests/test_hip_aov.py), with the chain and the tables, 3 owners."""
    W, H, tile = 130, 70, (64, 16)
    sc = stress_scene(scenes["spheres_a169"], 60, 4)
    extra = capi.KAJO_FLAG_NO_SHADOW_LISTS if which == "big" else 0
    flags = dict(matte=True, aov_specular=True, flags=extra)
    want, kernel = _untiled(sc, W, H, tile, BUILDS[build], **flags)
    assert ("_biglist" in kernel) == (which == "biglist") and "_big" in kernel
    got, k = _tiled_results(sc, W, H, tile, 3, BUILDS[build], **flags)
    assert k == kernel
    _assert_same(got, want, (which, build))


def test_fast_owners_agree(scenes):
    """FAST: tiled handles of 1, 2, 3 and 8 owners agree bit for bit; against the untiled FAST handle the differing words are printed (DESIGN.md
    section 6j records them: 0 in every buffer on the MI355X, the same kernel instance runs both shapes) and therefore asserted."""
    W, H, tile = 130, 70, (64, 16)
    sc = scenes["spheres_a169"]
    flags = dict(matte=True, aov_specular=True)
    first = None
    for n in OWNERS:
        got, _ = _tiled_results(sc, W, H, tile, n, BUILDS["fast"], **flags)
        if first is None:
            first = got
        else:
            _assert_same(got, first, n)
    want, _ = _untiled(sc, W, H, tile, BUILDS["fast"], **flags)
    differing = {k: int((bits(first[k]) != bits(want[k])).sum()) for k in want}
    print("FAST tiled against untiled, differing words:", differing)
    assert not any(differing.values()), differing


def test_an_owner_without_a_tile(scenes):
    """40x24 in 64x16 tiles is one tile per tile row, two in all: of three owners the last owns nothing (and so would the second of a
    40x16 frame, which is run too). It renders and reads its zeroed buffers without a launch; the result is the untiled handle's."""
    import torch
    from bench import DevicePtr
    tile = (64, 16)
    sc = scenes["spheres_a169"]
    for W, H in ((40, 24), (40, 16)):
        _no_tile_case(sc, W, H, tile, torch, DevicePtr)


def _no_tile_case(sc, W, H, tile, torch, DevicePtr):
    want, _ = _untiled(sc, W, H, tile, BUILDS["exact"], matte=True)
    owners = _tiled(sc, W, H, tile, 3, BUILDS["exact"], matte=True)
    n_tiles = TileLayout(W, H, 3, tile).n_tiles
    try:
        _render(owners)
        for o in owners[n_tiles:]:
            o.wait()
            a, ab, m, mb = o.aov_tile_buffers()
            assert ab == 2 * 64 * 16 * 16 and mb == 64 * 16 * 64
            assert not torch.as_tensor(DevicePtr(a, ab // 4), device="cuda").any().item()
            assert not torch.as_tensor(DevicePtr(m, mb // 4), device="cuda").any().item()
        keep = _compose(owners)
        _assert_same(_results(owners[0], True), want, "no tile")
        del keep
    finally:
        _close(owners)


def _state(call):
    with pytest.raises(capi.KajoError) as e:
        call()
    return e.value.code


def test_state_rules(scenes):
    sc = scenes["spheres_a169"]
    W, H = 130, 70
    with HipRenderer(sc, W, H, spp=SPP, seed=SEED, exact=True, aov=True, matte=True, aov_tiled=True) as r, \
            HipRenderer(sc, W, H, spp=SPP, seed=SEED, exact=True, aov=True, matte=True) as u:
        r.render(1)
        u.render(1)
        for call in (r.aov, r.denoise, r.matte, lambda: r.matte_mask(OBJECTS)):
            assert _state(call) == capi.KAJO_E_STATE  # before the first compose
        r.compose_aov()  # (one owner: its own buffers, one kernel)
        _assert_same(_results(r, True), _results(u, True), "one owner")
        r.render(1)
        u.render(1)
        for call in (r.aov, r.denoise, r.matte):
            assert _state(call) == capi.KAJO_E_STATE  # a render followed the compose
        r.compose_aov()
        _assert_same(_results(r, True), _results(u, True), "after the next compose")
        r.reset()
        assert _state(r.aov) == capi.KAJO_E_STATE
        r.compose_aov()
        a = r.aov()
        assert a["samples"] == 0 and not bits(a["raw"][0]).any() and not bits(a["raw"][1]).any()
        assert not r.matte()["counts"].any()
        # an untiled AOV handle has no tile buffers, and nothing to compose
        assert _state(u.aov_tile_buffers) == capi.KAJO_E_STATE
        assert _state(u.compose_aov) == capi.KAJO_E_STATE
    owners = _tiled(sc, W, H, (64, 16), 2, BUILDS["exact"], matte=True)
    try:
        _render(owners)
        assert _state(lambda: owners[0].compose_aov(None)) == capi.KAJO_E_INVALID
        # a matte handle composed without the matte buffers reads its AOVs and refuses the tables
        keep = _compose(owners, matte=False)
        assert owners[0].aov()["samples"] == 2 * SPP
        assert _state(owners[0].matte) == capi.KAJO_E_STATE and _state(lambda: owners[0].matte_mask(OBJECTS)) == capi.KAJO_E_STATE
        del keep
    finally:
        _close(owners)


def test_the_handle_stays_as_it_was(scenes):
    """radiance(), counters() (kernelMs included) and the passes rendered afterwards of an owner 0 that composed, read and denoised are
    those of a twin that never did."""
    sc = scenes["spheres_a169"]
    W, H = 130, 70
    kw = dict(spp=SPP, seed=SEED, exact=True, aov=True, matte=True, aov_tiled=True, counters=True)
    with HipRenderer(sc, W, H, **kw) as r, HipRenderer(sc, W, H, **kw) as twin:
        r.render(2)
        twin.render(2)
        r.wait()
        twin.wait()
        before = r.counters()
        r.compose_aov()
        _results(r, True)
        after = r.counters()
        assert after == before  # (kernelMs included: none of the new calls is timed)
        assert same(r.radiance(), twin.radiance())
        r.render(1)
        twin.render(1)
        assert same(r.radiance(), twin.radiance())
        ca, cb = r.counters(), twin.counters()
        assert {k: v for k, v in ca.items() if k != "kernelMs"} == {k: v for k, v in cb.items() if k != "kernelMs"}
        r.compose_aov()
        twin.compose_aov()
        _assert_same(_results(r, True), _results(twin, True), "afterwards")


def test_display_chain_on_the_root(scenes):
    """EXACT, 130x70, 3 owners, one NaN pixel on both sides: present() with every stage on the composed root gives the ARGB8, the scale bits
    and the meter result of the untiled handle's same call."""
    import torch
    from bench import DevicePtr
    sc = scenes["spheres_a169"]
    W, H, n = 130, 70, 3
    hole = (65, 17)
    chain = dict(despeckle=dict(), denoise=dict(iterations=3), glare=dict(strength=0.1), local=dict(compression=0.6), meter=dict(),
                 curve="reinhard")

    def poison(owners):
        layout = TileLayout(W, H, len(owners))
        for o in owners:
            o.wait()
        owner, slot = layout.owner_and_slot(np.array([hole[0]]), np.array([hole[1]]))
        ptr, nbytes = owners[int(owner[0])].tile_buffer()
        buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
        buf[int(slot[0]), 0] = float("nan")
        torch.cuda.synchronize()

    with HipRenderer(sc, W, H, spp=SPP, seed=SEED, exact=True, aov=True) as u:
        _render([u])
        poison([u])
        want_img, want_meter = u.present(**chain)
        want_scale = u.tone_scale()
        want_plain, want_plain_scale = u.present(despeckle=dict(), denoise=dict(iterations=3), glare=dict(strength=0.1))
    owners = _tiled(sc, W, H, (64, 16), n, BUILDS["exact"])
    try:
        _render(owners)
        poison(owners)
        keep = _compose(owners)
        img, meter = owners[0].present(**chain)
        assert np.array_equal(img, want_img)
        assert bits(np.float32(owners[0].tone_scale())) == bits(np.float32(want_scale))
        assert meter == want_meter
        plain, plain_scale = owners[0].present(despeckle=dict(), denoise=dict(iterations=3), glare=dict(strength=0.1))
        assert np.array_equal(plain, want_plain) and bits(np.float32(plain_scale)) == bits(np.float32(want_plain_scale))
        del keep
    finally:
        _close(owners)


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver(scenes, tmp_path):
    """kajo_render --aov-tiled on 1, 3 and 2 owners writes the files of the --gpus 1 run without the switch, byte for byte."""
    import torch
    sc = scenes["spheres_a169"]
    pod = str(tmp_path / "scene.pod")
    sc.write_pod(pod)

    def run(name, extra):
        d = tmp_path / name
        d.mkdir()
        cmd = [BIN, "-w", "160", "-h", "90", "--spp", "4", "--passes", "2", "--scene-pod", pod, "--json", "-o", str(d / "out.png"),
               "--aov", str(d / "aov"), "--aov-specular", "--matte-ids", str(d / "ids.pfm"), "--matte-mask", str(d / "mask.pfm"),
               "--matte-objects", "3,4", "--denoise", str(d / "denoised.png"), "--despeckle", "--glare", "0.1"] + extra
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
        assert p.returncode == 0, (name, p.stderr[-2000:])
        stats = json.loads(p.stdout.strip().splitlines()[-1])
        return {f.name: f.read_bytes() for f in sorted(d.iterdir())}, stats

    want, stats = run("plain", ["--gpus", "1"])
    assert "aov_tiled" not in stats and len(want) == 7
    two = ["--gpus", "2"] + (["--same-device"] if torch.cuda.device_count() < 2 else [])
    for name, extra in (("one", ["--gpus", "1"]), ("three", ["--gpus", "3", "--same-device"]), ("two", two)):
        got, stats = run(name, extra + ["--aov-tiled"])
        assert stats["aov_tiled"] is True
        assert sorted(got) == sorted(want)
        for f in want:
            assert got[f] == want[f], (name, f)
