"""Checkpoints (include/kajo_hip.h "Checkpoints"; kajo_amd/csrc/checkpoint.cpp, checkpoint_kernels.cpp) on the GPU: a session saved at P1 passes,
restored into a fresh twin handle and continued is the uninterrupted render bit for bit -- the accumulation in the tile buffer, the
radiance, the image, and with their flags the AOVs, the coverage tables, the noise moments and map, the counters and the adaptive state --
for every numerics build, at pass counts inside a group of four, from a section of the handle's own layout and from a merged whole-frame
section into other layouts. The section is a function of (scene, parameters, passes); the digests computed on the device are the numpy
restatement's (tests/checkpointlib.py) and add over owners; a refused restore leaves the handle as it was.

The tile buffers are compared at the slots of the image's pixels: include/kajo_hip.h leaves the other slots of a rendered buffer open
(a restore writes them as zero, which a test below holds)."""
import numpy as np
import pytest

import checkpointlib as ck
from kajo_amd import capi
from kajo_amd.renderer import HipRenderer, checkpoint_info, checkpoint_merge
from kajo_amd.tiles import TileLayout
from scenes_extra import dense_scene

pytestmark = pytest.mark.gpu

SEED = 0o715517
BUILDS = {"fast": {}, "exact": dict(exact=True), "strict": dict(strict=True)}
FRAMES = [(41, 23), (65, 9), (130, 40)]
TOTAL = 16
KW = dict(spp=4, depth_limit=8, seed=SEED)


@pytest.fixture(scope="module")
def the_scenes(scenes):
    return {"spheres": scenes["spheres_a169"], "grid60": dense_scene(scenes["spheres_a169"], 60, 3, seed=11),
            "other": scenes["spheres_a1"]}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_words(ptr, nbytes):
    import torch
    from bench import DevicePtr
    return torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda")


def raw_buffer(r):
    """the handle's whole tile buffer on the host, (slots, 4) uint32"""
    import torch
    r.wait()
    t = device_words(*r.tile_buffer()).clone()
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32).reshape(-1, 4)


def in_image(r):
    """the slots of the handle's buffer that hold a pixel of the image"""
    lay = TileLayout(r.width, r.height, r.params.tileCount, (r.params.tileW, r.params.tileH))
    ys, xs = np.mgrid[0:r.height, 0:r.width]
    owner, slot = lay.owner_and_slot(xs, ys)
    used = np.zeros(lay.slots_per_owner, bool)
    used[slot[owner == r.params.tileIndex]] = True
    return used


def outputs(r, **flags):
    """everything a reader of the handle can see, as arrays of bits"""
    out = {"tiles": raw_buffer(r)[in_image(r)]}
    if r.params.tileCount == 1:
        out["radiance"] = u32(r.radiance())
        out["argb8"] = r.argb8()
    if flags.get("aov") and not flags.get("aov_tiled"):
        a = r.aov()
        out.update({"aov_A": u32(a["raw"][0]), "aov_B": u32(a["raw"][1]), "aov_samples": a["samples"]})
    if flags.get("matte") and not flags.get("aov_tiled"):
        m = r.matte()
        out.update({"matte_" + k: np.asarray(v) for k, v in m.items()})
    if flags.get("noise"):
        rec = r.noise_moments()
        out.update({"moments_" + k: rec[k].view(np.uint64) for k in ("s1", "s2", "n", "bad")})
        n = r.noise()
        out.update({"noise_" + k: u32(n[k]) for k in ("mean", "stderr", "relative", "batches", "hist")})
    if flags.get("counters"):
        c = r.counters()
        # (laneSlots counts wave iterations: it follows the cut of the passes into launches on any handle, and is held below)
        out.update({"counter_" + k: c[k] for k in ("passes", "paths", "traversals", "vertices", "shadowQueries", "primitiveTests")})
    if flags.get("adaptive") is not None:
        out["adapt_state"] = r.adapt_state()
        out["adapt_passes"] = r.adapt_passes()
    return out


def same(a, b, why):
    assert sorted(a) == sorted(b), why
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], (why, k)


_STRAIGHT = {}


def straight(sc, key, W, H, passes=TOTAL, **flags):
    k = (key, W, H, passes, repr(sorted(flags.items())))
    if k not in _STRAIGHT:
        with HipRenderer(sc, W, H, **KW, **flags) as r:
            r.render(passes)
            _STRAIGHT[k] = outputs(r, **flags)
    return _STRAIGHT[k]


def resumed(sc, W, H, first, passes=TOTAL, **flags):
    """render `first` passes, save, restore into a fresh twin, render on to `passes`"""
    with HipRenderer(sc, W, H, **KW, **flags) as a:
        blob = a.render(first).checkpoint()
    with HipRenderer(sc, W, H, **KW, **flags) as b:
        b.restore(blob)
        assert b.passes == first
        b.render(passes - first)
        return outputs(b, **flags), blob


# ---- resume is the uninterrupted render -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [5, 6, 8])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("build", BUILDS)
def test_resume_is_the_uninterrupted_render(the_scenes, build, frame, first):
    sc, (W, H) = the_scenes["spheres"], frame
    got, blob = resumed(sc, W, H, first, **BUILDS[build])
    kinds = [p["name"] for p in checkpoint_info(blob)["planes"]]
    # 5 and 6 end inside a group of four: FAST and EXACT carry its summands, STRICT adds pass by pass
    assert kinds == (["SUM", "CARRY"] if build != "strict" and first % 4 else ["SUM"]), kinds
    same(got, straight(sc, "spheres", W, H, **BUILDS[build]), (build, frame, first))


FLAG_SETS = {"aov": dict(aov=True, aov_specular=True, matte=True), "noise": dict(noise=True), "counters": dict(counters=True)}


@pytest.mark.parametrize("first", [6, 8])
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_resume_with_each_flag_set(the_scenes, flags, first):
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    kw = dict(FLAG_SETS[flags], exact=True)
    got, blob = resumed(sc, W, H, first, **kw)
    names = [p["name"] for p in checkpoint_info(blob)["planes"]]
    assert {"aov": {"AOV", "MATTE"}, "noise": {"NOISE_BASE", "NOISE_MOMENTS"}, "counters": {"COUNTERS"}}[flags] <= set(names), names
    same(got, straight(sc, "spheres", W, H, **kw), (flags, first))


def test_lane_slots_follow_the_cut_of_the_passes_on_any_handle(the_scenes):
    """Why the comparisons with the straight run leave laneSlots out: KajoCounters.laneSlots is "64 * wave-iterations of the trace loop"
    (include/kajo_hip.h), and how many iterations the waves of a launch take depends on which passes the launch holds. One handle,
    no checkpoint: 6 + 10 passes against 16 trace the same paths in another number of iterations."""
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    with HipRenderer(sc, W, H, **KW, exact=True, counters=True) as a:
        one = a.render(16).counters()
    with HipRenderer(sc, W, H, **KW, exact=True, counters=True) as b:
        two = b.render(6).render(10).counters()
    assert all(one[k] == two[k] for k in ("passes", "paths", "traversals", "vertices", "shadowQueries"))
    assert one["laneSlots"] != two["laneSlots"], one


def test_a_restore_brings_every_counter_back(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    with HipRenderer(sc, W, H, **KW, exact=True, counters=True) as a:
        blob = a.render(6).checkpoint()
        want = a.counters()
    assert want["laneSlots"] > 0 and want["launches"] > 0
    with HipRenderer(sc, W, H, **KW, exact=True, counters=True) as b:
        b.render(3)
        got = b.restore(blob).counters()
    assert got == dict(want, tailGroups=0), (got, want)  # (kernelMs and launches travel in the trailer)


def test_resume_on_a_grid_class_scene(the_scenes):
    sc, (W, H) = the_scenes["grid60"], (65, 9)
    kw = dict(exact=True, aov=True, noise=True, counters=True)
    got, _ = resumed(sc, W, H, 6, **kw)
    same(got, straight(sc, "grid60", W, H, **kw), "grid60")


def _tiled_owners(sc, W, H, n, tile=(64, 16), **kw):
    return [HipRenderer(sc, W, H, **KW, tile=tile, tile_index=i, tile_count=n, **kw) for i in range(n)]


def _tiled_outputs(owners):
    import torch
    out = {}
    for i, r in enumerate(owners):
        r.wait()
        used = in_image(r)
        aov, aov_bytes, matte, matte_bytes = r.aov_tile_buffers()
        a = device_words(aov, aov_bytes).clone().cpu().numpy().view(np.uint32).reshape(2, -1, 4)
        m = device_words(matte, matte_bytes).clone().cpu().numpy().view(np.uint32).reshape(2, -1, 8)
        torch.cuda.synchronize()
        out.update({"tiles%d" % i: raw_buffer(r)[used], "aov%d" % i: a[:, used], "matte%d" % i: m[:, used]})
    return out


def test_resume_with_tiled_aovs_and_three_owners(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (130, 40)
    kw = dict(exact=True, aov=True, matte=True, aov_tiled=True)
    owners = _tiled_owners(sc, W, H, 3, **kw)
    try:
        for r in owners:
            r.render(TOTAL)
        want = _tiled_outputs(owners)
    finally:
        for r in owners:
            r.close()
    first = _tiled_owners(sc, W, H, 3, **kw)
    twins = _tiled_owners(sc, W, H, 3, **kw)
    try:
        for a, b in zip(first, twins):
            b.restore(a.render(6).checkpoint())
            b.render(TOTAL - 6)
        same(_tiled_outputs(twins), want, "tiled")
    finally:
        for r in first + twins:
            r.close()


# ---- adaptive ---------------------------------------------------------------------------------------------------------------------------

def test_resume_of_an_adaptive_session(the_scenes):
    sc, (W, H), P = the_scenes["spheres"], (41, 23), 32
    # a target some units meet at the first decision (pass 16) and others do not: the lower median of the units' worst relative error
    with HipRenderer(sc, W, H, **KW, exact=True, noise=True, adaptive=True) as t:
        rel = t.render(16).noise()["relative"]
        slots = t.adapt_state()["unitSlots"]
    ys, xs = np.mgrid[0:H, 0:W]
    _, slot = TileLayout(W, H, 1).owner_and_slot(xs, ys)
    worst = np.sort([rel[slot // slots == u].max() for u in np.unique(slot // slots)])
    target = float(worst[(len(worst) - 1) // 2])
    assert target > 0 and worst[-1] > target
    kw = dict(exact=True, noise=True, adaptive=dict(target=target))
    with HipRenderer(sc, W, H, **KW, **kw) as a:
        a.render(18)
        s = a.adapt_state()
        assert s["lastDecisionPass"] == 16 and 0 < s["activeUnits"] < s["units"], s  # one retired at least, one still active
        blob = a.checkpoint()
        assert "ADAPT" in [p["name"] for p in checkpoint_info(blob)["planes"]]
    with HipRenderer(sc, W, H, **KW, **kw) as b:
        b.restore(blob)
        assert b.adapt_state() == s
        got = outputs(b.render(P - 18), **kw)
    want = straight(sc, "spheres", W, H, passes=P, **kw)
    assert want["adapt_state"]["lastDecisionPass"] == 32
    same(got, want, "adaptive")
    # another layout: refused, and the handle is what it was
    with HipRenderer(sc, W, H, **KW, tile=(16, 16), **kw) as c:
        before = c.render(4).digest()
        with pytest.raises(capi.KajoError, match="ADAPT"):
            c.restore(blob)
        assert c.digest() == before and c.passes == 4


# ---- layout-free ------------------------------------------------------------------------------------------------------------------------

def _composed(owners, lay):
    gathered = np.zeros((lay.world, lay.slots_per_owner, 4), np.uint32)
    for i, r in enumerate(owners):
        gathered[i] = raw_buffer(r)
    return lay.compose(gathered)


def test_a_merged_section_restores_into_any_layout(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (130, 40)
    want = straight(sc, "spheres", W, H, exact=True)
    owners = _tiled_owners(sc, W, H, 3, exact=True)
    try:
        blobs = [r.render(6).checkpoint() for r in owners]
        digests = [r.digest()["SUM"] for r in owners]
    finally:
        for r in owners:
            r.close()
    merged = checkpoint_merge(blobs)
    info = checkpoint_info(merged)
    assert (info["tileCount"], info["pixels"], info["passesDone"]) == (1, W * H, 6)
    assert [p["name"] for p in info["planes"]] == ["SUM", "CARRY"]
    assert info["planes"][0]["digest"] == sum(digests) & ck.MASK
    # (a) one whole-frame handle
    with HipRenderer(sc, W, H, **KW, exact=True) as r:
        assert r.restore(merged).digest()["SUM"] == info["planes"][0]["digest"]
        same(outputs(r.render(TOTAL - 6)), want, "whole frame")
    # (b) two owners with 16x16 tiles, composed
    two = _tiled_owners(sc, W, H, 2, tile=(16, 16), exact=True)
    try:
        for r in two:
            r.restore(merged).render(TOTAL - 6)
        frame = _composed(two, TileLayout(W, H, 2, (16, 16)))
        assert np.array_equal(frame, want["radiance"])
    finally:
        for r in two:
            r.close()


# ---- the section is a function of (scene, parameters, passes) ---------------------------------------------------------------------------

@pytest.mark.parametrize("build", ["exact", "strict"])
def test_the_section_does_not_depend_on_the_cut_of_the_passes_or_on_slots_outside_the_image(the_scenes, build):
    import torch
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    kw = dict(BUILDS[build], noise=True, aov=True)
    bodies = []
    for cut in ((6,), (1, 2, 3), (4, 2), (6,)):
        with HipRenderer(sc, W, H, **KW, **kw) as r:
            for c in cut:
                r.render(c)
            if len(bodies) == 3:  # the twin: every slot that holds no pixel of the image poisoned before the save
                r.wait()
                buf = device_words(*r.tile_buffer()).view(-1, 4)
                buf[torch.from_numpy(~in_image(r)).cuda()] = float("nan")
                torch.cuda.synchronize()
            bodies.append(ck.body(r.checkpoint()))
    assert bodies[0] == bodies[1] == bodies[2] == bodies[3]
    # ... and a restore defines every slot: zero where there is no pixel
    with HipRenderer(sc, W, H, **KW, **kw) as r:
        r.restore(bodies[0] + bytes(16))
        buf = raw_buffer(r)
        assert not buf[~in_image(r)].any()
        ys, xs = np.mgrid[0:H, 0:W]
        _, slot = TileLayout(W, H, 1).owner_and_slot(xs, ys)
        assert np.array_equal(buf[slot.ravel()], ck.parse(bodies[0] + bytes(16))["planes"][ck.SUM]["words"])


# ---- the digest -------------------------------------------------------------------------------------------------------------------------

def test_the_digest_is_the_restatement_over_the_radiance_and_survives_a_restore(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (65, 9)
    with HipRenderer(sc, W, H, **KW, exact=True, aov=True) as r:
        d = r.render(6).digest()
        assert sorted(d) == ["AOV", "CARRY", "SUM"]
        assert d["SUM"] == ck.digest(np.arange(W * H), u32(r.radiance()).reshape(-1, 4))
        a = r.aov()
        assert d["AOV"] == ck.digest(np.arange(W * H), np.concatenate([u32(a["raw"][0]).reshape(-1, 4), u32(a["raw"][1]).reshape(-1, 4)], 1))
        blob = r.checkpoint()
    in_blob = {p["name"]: p["digest"] for p in checkpoint_info(blob)["planes"]}
    assert in_blob == d
    with HipRenderer(sc, W, H, **KW, exact=True, aov=True) as r:
        assert r.restore(blob).digest() == d
        r.render(1)
        assert r.digest()["SUM"] != d["SUM"]


def test_the_owners_digests_add_up_to_the_whole_frames(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (130, 40)
    with HipRenderer(sc, W, H, **KW, strict=True) as r:
        whole = r.render(5).digest()["SUM"]
    for tile in ((64, 16), (16, 16)):
        owners = _tiled_owners(sc, W, H, 3, tile=tile, strict=True)
        try:
            assert sum(o.render(5).digest()["SUM"] for o in owners) & ck.MASK == whole, tile
        finally:
            for o in owners:
                o.close()


# ---- refusals on a live handle ----------------------------------------------------------------------------------------------------------

def test_a_refused_restore_leaves_the_handle_as_it_was(the_scenes):
    sc, (W, H) = the_scenes["spheres"], (41, 23)
    with HipRenderer(sc, W, H, **KW, exact=True) as r:
        good = r.render(6).checkpoint()
    sections = {}
    with HipRenderer(the_scenes["other"], W, H, **KW, exact=True) as r:
        sections["another scene"] = (r.render(6).checkpoint(), "fingerprint")
    with HipRenderer(sc, W, H, **dict(KW, seed=SEED + 1), exact=True) as r:
        sections["another seed"] = (r.render(6).checkpoint(), "fingerprint")
    with HipRenderer(sc, W, H, **dict(KW, spp=9), exact=True) as r:
        sections["another S"] = (r.render(6).checkpoint(), "fingerprint")
    with HipRenderer(sc, W, H, **KW, strict=True) as r:
        sections["strict into exact"] = (r.render(6).checkpoint(), "fingerprint")
    with HipRenderer(sc, W, H, **KW, exact=True, noise=True) as r:
        sections["planes the handle does not keep"] = (r.render(6).checkpoint(), "planes")
    bad = bytearray(good)
    bad[ck.parse(good)["planes"][ck.CARRY]["offset"] + 5] ^= 0x40
    sections["a corrupted plane"] = (bytes(bad), "plane CARRY")
    sections["a truncated section"] = (good[:-40], "truncated")
    # a header of another frame size under the handle's own fingerprint word: held field by field, nothing is read past the plane
    sections["another frame size"] = (ck.section(W + 1, H, {ck.SUM: np.zeros(((W + 1) * H, 4), np.uint32)}, flags=capi.KAJO_FLAG_EXACT, seed=SEED,
                                                 fingerprint=ck.parse(good)["fingerprint"]), "fingerprint")
    with HipRenderer(sc, W, H, **KW, tile=(16, 16), tile_index=1, tile_count=2, exact=True) as r:
        sections["another owner's section"] = (r.render(6).checkpoint(), "layout")
    with HipRenderer(sc, W, H, **KW, exact=True) as r:
        r.render(3)
        before, frame = r.digest(), r.radiance().copy()
        for name, (blob, word) in sections.items():
            with pytest.raises(capi.KajoError, match=word) as e:
                r.restore(blob)
            assert e.value.code == capi.KAJO_E_INVALID, name
            assert r.digest() == before and r.passes == 3 and r.counters()["passes"] == 3, name
        assert np.array_equal(u32(r.render(1).radiance()), straight(sc, "spheres", W, H, passes=4, exact=True)["radiance"])
        assert not np.array_equal(frame, r.radiance())
    # the converse: a section without the planes the handle keeps
    with HipRenderer(sc, W, H, **KW, exact=True, noise=True, counters=True) as r:
        before = r.render(4).digest()
        with pytest.raises(capi.KajoError, match="planes"):
            r.restore(good)
        assert r.digest() == before


# ---- the driver -------------------------------------------------------------------------------------------------------------------------

import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
SCENE = os.path.join(ROOT, "kajo_amd", "data", "caustics.json")
DRIVER = [BIN, "-w", "65", "-h", "9", "-r", "hip", "--spp", "4", "--batch", "3", "--json", "--no-preview"]


def _drive(tmp_path, name, passes, extra, ok=True):
    out, raw = str(tmp_path / (name + ".png")), str(tmp_path / (name + ".raw"))
    p = subprocess.run(DRIVER + ["--passes", str(passes), "-o", out, "--raw", raw] + extra + [SCENE], capture_output=True, text=True, timeout=120)
    if not ok:
        assert p.returncode != 0, p.stdout
        return p.stderr
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1]), open(out, "rb").read(), open(raw, "rb").read()


def test_driver_stops_and_resumes_to_the_straight_run(tmp_path):
    """kajo_render at 65x9 with --batch 3: 6 passes with --checkpoint, then --resume to 16, against a straight 16-pass run: --raw and the
    PNG byte for byte, frame_digest equal; then the same file resumed by three owners (through the merge), and a periodic file."""
    assert os.path.exists(BIN), BIN
    file, other = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    want, png, raw = _drive(tmp_path, "straight", 16, ["--checkpoint", other])
    assert (want["checkpoint_file"], want["checkpoint_passes"], want["resumed_from_passes"]) == (other, 16, 0)
    first, _, _ = _drive(tmp_path, "first", 6, ["--checkpoint", file])
    assert first["checkpoint_passes"] == 6 and first["frame_digest"] != want["frame_digest"] and not os.path.exists(file + ".tmp")
    got, png2, raw2 = _drive(tmp_path, "resumed", 16, ["--resume", file])
    assert (got["resumed_from_passes"], got["checkpoint_passes"], got["frame_digest"]) == (6, 0, want["frame_digest"])
    assert png2 == png and raw2 == raw
    # the digest is the SUM plane's: --raw is that plane for one owner
    words = np.frombuffer(raw, np.uint32).reshape(-1, 4)
    assert int(want["frame_digest"], 16) == ck.digest(np.arange(65 * 9), words)
    # another number of owners: merged first
    three, png3, raw3 = _drive(tmp_path, "three", 16, ["--resume", file, "--gpus", "3", "--same-device", "--checkpoint", other, "--checkpoint-every", "4"])
    assert (three["resumed_from_passes"], three["checkpoint_passes"], three["frame_digest"]) == (6, 16, want["frame_digest"])
    assert png3 == png and raw3 == raw
    # ... and their file back into one
    back, png4, raw4 = _drive(tmp_path, "back", 16, ["--resume", other])
    assert back["resumed_from_passes"] == 16 and back["frame_digest"] == want["frame_digest"] and png4 == png and raw4 == raw


@pytest.mark.parametrize("rule", ["adaptive", "until-noise"])
def test_driver_resumes_a_stop_rule_session_to_the_straight_run(tmp_path, rule):
    """run()'s own bookkeeping across a resume: an --adaptive session (decisions every 8 passes from pass 8 on) and an --until-noise one,
    two owners on one device, stopped at 12 passes -- between two decisions; --batch 3 becomes refreshes of whole batches of four under a
    rule -- and resumed to 32: the frame, the statistics of the rule and the digest are the straight run's."""
    assert os.path.exists(BIN), BIN
    file = str(tmp_path / "rule.ckpt")
    opts = {"adaptive": ["--adaptive", "0.3", "--adaptive-min-passes", "8", "--adaptive-every", "2"],
            "until-noise": ["--until-noise", "1e-6"]}[rule] + ["--gpus", "2", "--same-device"]
    keys = {"adaptive": ("adaptive_active_units", "adaptive_units", "adaptive_paths", "adaptive_stopped_at_pass", "noise_quantile_value"),
            "until-noise": ("noise_quantile_value", "noise_known_px", "noise_bad_px", "noise_stopped_at_pass")}[rule]
    want, png, raw = _drive(tmp_path, "straight", 0, opts + ["--max-passes", "32", "--checkpoint", str(tmp_path / "end.ckpt")])
    assert want["passes"] == 32 and want["checkpoint_passes"] == 32
    if rule == "adaptive":
        assert 0 < want["adaptive_active_units"] < want["adaptive_units"], want  # (some retired, some still active: the rule did something)
    first, _, _ = _drive(tmp_path, "first", 0, opts + ["--max-passes", "12", "--checkpoint", file])
    assert first["passes"] == 12
    got, png2, raw2 = _drive(tmp_path, "resumed", 0, opts + ["--max-passes", "32", "--resume", file])
    assert (got["passes"], got["resumed_from_passes"], got["frame_digest"]) == (32, 12, want["frame_digest"])
    assert [got[k] for k in keys] == [want[k] for k in keys], (got, want)
    assert png2 == png and raw2 == raw


def test_driver_refuses_an_adaptive_file_at_another_gpu_count(tmp_path):
    file = str(tmp_path / "adaptive.ckpt")
    _drive(tmp_path, "a", 8, ["--adaptive", "0.5", "--max-passes", "8", "--checkpoint", file])
    err = _drive(tmp_path, "b", 16, ["--adaptive", "0.5", "--max-passes", "16", "--resume", file, "--gpus", "2", "--same-device"], ok=False)
    assert "adaptive" in err and "GPU" in err, err
    assert "--checkpoint" in _drive(tmp_path, "c", 4, ["--checkpoint-every", "2"], ok=False)
