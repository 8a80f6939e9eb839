"""Object-coverage mattes (KAJO_FLAG_AOV_MATTE; include/kajo_hip.h kajo_hip_read_matte, kajo_hip_matte_mask; the _matte instances of
kajo_amd/csrc/aov.inc.hip and kajo_amd/csrc/matte.hip) on the GPU.

The definition is restated in numpy (tests/matte_replay.py): the ids are the oracle's trace over the replayed camera rays -- for
KAJO_FLAG_AOV_SPECULAR the final hits of tests/aov_specular_replay.py's chain -- and the tables, the first-come rule, the rank order and
the mask are integer numpy. The counts are integers, so STRICT and EXACT handles must give the restatement word for word, and every
build must keep the invariants."""
import json
import os
import subprocess

import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import stress_scene
from oraclelib import available

from aov_specular_replay import material_tables, replay_specular, with_delta_balls, without_delta
from matte_replay import mask_of, restate
from framelib import read_pfm
from test_hip_aov import crowded_scene, open_floor
from test_matte_cpu import OVERFLOW

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not available("oracle"), reason="oracle not built")]
SEED = 0o715517
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
BUILDS = [dict(exact=True), dict(strict=True), dict()]
ORACLE_BUILDS = (dict(strict=True), dict(exact=True))  # STRICT's walk: the oracle's ids
FRAMES = [(1, 1), (7, 5), (41, 23), (65, 9)]
P = 3


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def tables_equal(got, want):
    return (bits_equal(got["ids"], want["ids"]) and bits_equal(got["counts"], want["counts"]) and
            np.array_equal(got["dropped"], want["dropped"]) and got["samples"] == want["samples"])


def render(sc, w, h, spp, passes=P, **kw):
    with HipRenderer(sc, w, h, spp=spp, seed=SEED, aov=True, matte=True, **kw) as r:
        r.render(passes)
        return r.matte(), r.aov_kernel()


def check_rank_order(m):
    """count descending, id ascending on ties, empties last as (-1, 0)"""
    ids, counts = m["ids"].astype(np.int64), m["counts"].astype(np.int64)
    assert (counts[..., :-1] >= counts[..., 1:]).all()
    tie = (counts[..., :-1] == counts[..., 1:]) & (counts[..., 1:] > 0)
    assert (ids[..., :-1][tie] < ids[..., 1:][tie]).all()
    assert ((counts == 0) == (ids == -1)).all() and (ids >= -1).all()


@pytest.mark.parametrize("spp", [4, 32])
@pytest.mark.parametrize("frame", FRAMES)
def test_tables_equal_the_restatement_strict_and_exact(scenes, frame, spp):
    sc = scenes["spheres_a169"]
    w, h = frame
    n2 = int(np.sqrt(float(spp))) ** 2
    for spec in (False, True):
        want = restate(sc, range(1, P + 1), w, h, spp, SEED, spec)
        assert want["samples"] == n2 * P
        for kw in ORACLE_BUILDS:
            got, kernel = render(sc, w, h, spp, aov_specular=spec, **kw)
            assert kernel == ("kajo_aov_strict_spec_matte" if spec else "kajo_aov_strict_matte"), kernel
            assert tables_equal(got, want), (frame, spp, spec, kw, np.argwhere((got["ids"] != want["ids"]) | (got["counts"] != want["counts"]))[:4])
            check_rank_order(got)


def test_rank_order_on_a_tie_the_restatement_shows(scenes):
    sc = scenes["spheres_a169"]
    w, h, spp = 41, 23, 4
    want = restate(sc, range(1, P + 1), w, h, spp, SEED)
    c = want["counts"].astype(np.int64)
    tie = ((c[..., :-1] == c[..., 1:]) & (c[..., 1:] > 0)).any(-1)
    assert tie.any()  # (measured: 14 pixels of this frame hold two ids seen equally often)
    got, _ = render(sc, w, h, spp, strict=True)
    y, x = np.argwhere(tie)[0]
    k = int(np.flatnonzero((c[y, x, :-1] == c[y, x, 1:]) & (c[y, x, 1:] > 0))[0])
    assert got["counts"][y, x, k] == got["counts"][y, x, k + 1] > 0 and got["ids"][y, x, k] < got["ids"][y, x, k + 1]
    assert bits_equal(got["ids"][tie], want["ids"][tie]) and bits_equal(got["counts"][tie], want["counts"][tie])


def test_with_the_chain_the_id_is_the_final_hit(scenes):
    """The mirror wall shows the objects it reflects; the restatement's chain is replay_specular's (same hit counts); without delta
    materials the flag changes no word."""
    sc = scenes["spheres_a169"]
    w, h, spp = 41, 23, 32
    lobe = material_tables(sc)[0]
    wall = int(np.flatnonzero(lobe[:sc.n_planes] == 2)[0]) + 1
    first = restate(sc, range(1, P + 1), w, h, spp, SEED, False)
    final = restate(sc, range(1, P + 1), w, h, spp, SEED, True)
    on_wall = (first["ids"][..., 0] == wall) & (first["counts"][..., 0] == first["samples"])
    assert on_wall.any() and (final["ids"][on_wall] != wall).any()
    A, _, stats = replay_specular(sc, range(1, P + 1), w, h, spp, SEED)
    assert stats["followed"] > 0
    hits = np.where(final["ids"] > 0, final["counts"], 0).sum(-1)
    assert np.array_equal(hits, A[..., 3].astype(np.int64))  # (nothing dropped on this frame: the tables hold every sample)
    got, _ = render(sc, w, h, spp, aov_specular=True, strict=True)
    assert tables_equal(got, final)
    assert (got["ids"][on_wall][:, 0] != wall).any()
    plain = without_delta(sc)
    for kw in BUILDS:
        a, ka = render(plain, w, h, spp, **kw)
        b, kb = render(plain, w, h, spp, aov_specular=True, **kw)
        assert "_spec" not in ka and "_spec_matte" in kb
        assert tables_equal(a, b), kw
    strict, _ = render(plain, w, h, spp, aov_specular=True, strict=True)
    assert tables_equal(strict, restate(plain, range(1, P + 1), w, h, spp, SEED, False))


def _big_scenes(scenes):
    base = scenes["spheres_a169"]
    return {
        "stress1000": (stress_scene(base, 1000, 16), 0, "biglist_lg"),
        "stress1000_nolists": (stress_scene(base, 1000, 16), capi.KAJO_FLAG_NO_SHADOW_LISTS, "big_lg"),
        "grid_global": (crowded_scene(base), 0, "biglist"),
        "grid_global_nolists": (crowded_scene(base), capi.KAJO_FLAG_NO_SHADOW_LISTS, "big"),
    }


@pytest.mark.parametrize("spec", [False, True])
@pytest.mark.parametrize("name", ["stress1000", "stress1000_nolists", "grid_global", "grid_global_nolists"])
def test_overflow_first_come_and_dropped_on_the_large_scene_instances(scenes, name, spec):
    sc, flags, cls = _big_scenes(scenes)[name]
    if spec:
        sc = with_delta_balls(sc)
    w, h, spp, passes = OVERFLOW["w"], OVERFLOW["h"], OVERFLOW["spp"], OVERFLOW["passes"]
    want = restate(sc, passes, w, h, spp, SEED, spec)
    over = want["distinct"] > 8
    print(name, spec, "pixels with more than 8 ids: %d, the most %d, samples dropped %d" % (over.sum(), want["distinct"].max(), want["dropped"].sum()))
    assert over.any() and (want["dropped"][over] > 0).all() and (want["dropped"][~over] == 0).all()  # (the oracle's side first)
    # the ids a full table holds are the first eight that came, whatever came more often later
    seq = want["sample_ids"]
    for y, x in np.argwhere(over):
        col = seq[:, y * w + x]
        _, first_at = np.unique(col, return_index=True)
        first_eight = col[np.sort(first_at)[:8]]
        assert sorted(want["ids"][y, x].tolist()) == sorted(first_eight.tolist())
    for kw in ORACLE_BUILDS:
        got, kernel = render(sc, w, h, spp, passes=len(passes), aov_specular=spec, flags=flags, **kw)
        assert kernel == "kajo_aov_strict_%s_%s" % ("spec_matte" if spec else "matte", cls), kernel
        assert tables_equal(got, want), (name, spec, kw)
        check_rank_order(got)
        assert (got["counts"][over] > 0).all()


@pytest.mark.parametrize("build", BUILDS)
def test_pass_cuts_reset_twin_and_second_read(scenes, build):
    w, h, spp = 41, 23, 32
    for sc, flags in ((scenes["spheres_a169"], 0), (stress_scene(scenes["spheres_a169"], 60, 4), 0)):
        got = []
        for ppl, cuts in ((0, (1, 2)), (0, (3,)), (1, (3,)), (0, (3,))):  # (the last: a twin of the second)
            with HipRenderer(sc, w, h, spp=spp, seed=SEED, aov=True, matte=True, passes_per_launch=ppl, flags=flags, **build) as r:
                for c in cuts:
                    r.render(c)
                m = r.matte()
                again = r.matte()
                assert tables_equal(m, again)
                masks = r.matte_mask([0, 3])
                got.append(m)
                if ppl == 1:
                    r.reset()
                    e = r.matte()
                    assert e["samples"] == 0 and (e["ids"] == -1).all() and (e["counts"] == 0).all() and (e["dropped"] == 0).all()
                    mask, dominant = r.matte_mask([0, 3])
                    assert (mask == 0).all() and (dominant == -1).all()
                    assert tables_equal(r.render(3).matte(), m)
                    after = r.matte_mask([0, 3])
                    assert bits_equal(after[0], masks[0]) and bits_equal(after[1], masks[1])
        for g in got[1:]:
            assert g["samples"] == 75 and tables_equal(g, got[0]), (sc.name, build)


def test_set_pass_count_leaves_the_tables_alone(scenes):
    sc = scenes["spheres_a169"]
    w, h, spp = 7, 5, 32
    with HipRenderer(sc, w, h, spp=spp, seed=SEED, strict=True, aov=True, matte=True) as r:
        before = r.render(1).matte()
        r.set_pass_count(5)
        assert tables_equal(r.matte(), before)
        got = r.render(1).matte()
    assert tables_equal(got, restate(sc, (1, 6), w, h, spp, SEED))


def test_no_pass_rendered_and_handles_without_the_flag(scenes):
    sc = scenes["spheres_a169"]
    with HipRenderer(sc, 7, 5, spp=4, seed=SEED, exact=True, aov=True, matte=True) as r:
        m = r.matte()
        assert m["samples"] == 0 and (m["ids"] == -1).all() and (m["counts"] == 0).all()
        mask, dominant = r.matte_mask([1, 2, 3])
        assert (mask == 0).all() and (dominant == -1).all()
        L = capi.lib()
        assert L.kajo_hip_read_matte(r._h, None, None, None) == 0 and L.kajo_hip_matte_mask(r._h, None, 0, None, None) == 0
    with HipRenderer(sc, 7, 5, spp=4, seed=SEED, exact=True, aov=True) as r:
        assert "matte" not in r.aov_kernel()
        r.render(1)
        for call in (r.matte, lambda: r.matte_mask([1])):
            with pytest.raises(capi.KajoError) as e:
                call()
            assert e.value.code == capi.KAJO_E_STATE


@pytest.mark.parametrize("build", BUILDS)
def test_invariants_in_every_build(scenes, build):
    """counts + dropped = samples; where nothing is dropped the hit count A.w of the same walk is the counts of the ids other than 0."""
    w, h, spp = 41, 23, 32
    base = scenes["spheres_a169"]
    for sc, spec in ((base, False), (base, True), (open_floor(base), False), (open_floor(base), True)):
        assert not restate(sc, range(1, P + 1), w, h, spp, SEED, spec)["dropped"].any()
        with HipRenderer(sc, w, h, spp=spp, seed=SEED, aov=True, matte=True, aov_specular=spec, **build) as r:
            r.render(P)
            m, A = r.matte(), r.aov()["raw"][0]
        counts = m["counts"].astype(np.int64)
        assert m["samples"] == 75 and (counts.sum(-1) + m["dropped"] == m["samples"]).all() and (m["dropped"] >= 0).all()
        hits = A[..., 3].astype(np.int64)
        assert np.array_equal(hits, A[..., 3])  # (whole numbers)
        assert np.array_equal(np.where(m["ids"] > 0, counts, 0).sum(-1), hits), (sc.name, spec, build)
        assert np.array_equal(np.where(m["ids"] == 0, counts, 0).sum(-1), m["samples"] - hits), (sc.name, spec, build)
        check_rank_order(m)
        if sc.name == "open_floor":
            assert (m["ids"] == 0).any() and (m["ids"] > 0).any()
    # ... and the first identity where samples are dropped (the large scene, the overflow frame)
    sc = stress_scene(base, 1000, 16)
    m, _ = render(sc, OVERFLOW["w"], OVERFLOW["h"], OVERFLOW["spp"], passes=2, **build)
    assert (m["counts"].sum(-1, dtype=np.int64) + m["dropped"] == 50).all() and (m["dropped"] > 0).any() and (m["dropped"] >= 0).all()
    check_rank_order(m)


def test_fast_equals_strict_away_from_silhouettes(scenes):
    """Where STRICT's table holds one id and its eight neighbours hold the same one, no ray of the pixel is near an edge FAST's rounding
    could move: FAST's table is the same."""
    sc = scenes["spheres_a169"]
    w, h, spp = 65, 41, 32
    s, _ = render(sc, w, h, spp, strict=True)
    f, _ = render(sc, w, h, spp)
    single = s["counts"][..., 0] == s["samples"]
    top = np.where(single, s["ids"][..., 0], -2)
    interior = np.zeros((h, w), bool)
    interior[1:-1, 1:-1] = single[1:-1, 1:-1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            interior[1:-1, 1:-1] &= top[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] == top[1:-1, 1:-1]
    seen = np.unique(top[interior])
    print("interior pixels: %d of %d, ids %s" % (interior.sum(), interior.size, seen.tolist()))
    assert seen.size >= 2
    assert bits_equal(f["ids"][interior], s["ids"][interior]) and bits_equal(f["counts"][interior], s["counts"][interior])


@pytest.mark.parametrize("name", ["spheres_a169", "stress1000"])
def test_matte_mask(scenes, name):
    if name == "stress1000":
        sc, (w, h, spp, passes) = stress_scene(scenes["spheres_a169"], 1000, 16), (OVERFLOW["w"], OVERFLOW["h"], OVERFLOW["spp"], 2)
    else:
        sc, (w, h, spp, passes) = scenes["spheres_a169"], (41, 23, 32, P)
    n_objects = sc.n_planes + sc.n_spheres
    with HipRenderer(sc, w, h, spp=spp, seed=SEED, exact=True, aov=True, matte=True) as r:
        r.render(passes)
        m = r.matte()
        samples = m["samples"]
        everything = list(range(n_objects + 1))
        held = np.unique(m["ids"][m["ids"] >= 0]).tolist()
        chosen = held[::2]
        rest = [i for i in everything if i not in chosen]
        for objects in (chosen, rest, everything, [0], held[:1], [n_objects]):
            mask, dominant = r.matte_mask(objects)
            assert bits_equal(mask, mask_of(m["ids"], m["counts"], samples, objects)), objects
            assert bits_equal(dominant, m["ids"][..., 0].astype(np.float32))
        # a set and its complement: m1 = fl(a / s), m2 = fl(b / s) with a + b = s - dropped, each within half an ulp of a number
        # below 1 (2^-25), so their exact sum is within 2^-24 -- one float32 rounding -- of 1 - dropped / s
        m1, m2 = r.matte_mask(chosen)[0].astype(np.float64), r.matte_mask(rest)[0].astype(np.float64)
        assert (m1 > 0).any() and (m2 > 0).any()
        assert (np.abs((m1 + m2) - (1.0 - m["dropped"] / samples)) <= 2.0 ** -24).all()
        assert (r.matte_mask(everything)[0] == ((samples - m["dropped"]).astype(np.float32) / np.float32(samples))).all()
        if name == "stress1000":
            assert (m["dropped"] > 0).any()
        zeros, _ = r.matte_mask([])
        assert (zeros == 0).all() and zeros.dtype == np.float32
        assert bits_equal(r.matte_mask(chosen + chosen[::-1] + chosen[:1])[0], r.matte_mask(chosen)[0])
        for bad in ([n_objects + 1], [-1], [1, 2, 1 << 30]):
            with pytest.raises(capi.KajoError) as e:
                r.matte_mask(bad)
            assert e.value.code == capi.KAJO_E_INVALID and "out of range" in str(e.value)
        assert tables_equal(r.matte(), m)


@pytest.mark.parametrize("build", BUILDS)
def test_a_matte_handle_leaves_everything_else_alone(scenes, build):
    w, h, spp = 41, 23, 32
    for sc in (scenes["spheres_a169"], stress_scene(scenes["spheres_a169"], 1000, 16)):
        out = []
        for matte in (False, True):
            with HipRenderer(sc, w, h, spp=spp, seed=SEED, aov=True, matte=matte, counters=True, **build) as r:
                r.render(1).render(2)
                if matte:
                    r.counters()
                    r.matte()
                    r.matte_mask([0, 1, 2])
                c = r.counters()
                got = dict(radiance=r.radiance(), A=r.aov()["raw"][0], B=r.aov()["raw"][1], argb8=r.argb8(), counters=c)
                if matte:  # the readers change nothing, the device time included
                    r.matte()
                    r.matte_mask([3])
                    assert r.counters() == c and bits_equal(r.radiance(), got["radiance"]) and bits_equal(r.aov()["raw"][0], got["A"])
                out.append(got)
        a, b = out
        for k in ("radiance", "A", "B", "argb8"):
            assert bits_equal(a[k], b[k]), (sc.name, build, k)
        # (kernelMs is a measured time: the one counter two runs of anything do not share)
        assert {k: v for k, v in a["counters"].items() if k != "kernelMs"} == {k: v for k, v in b["counters"].items() if k != "kernelMs"}
        assert a["counters"]["launches"] > 0 and a["counters"]["traversals"] > 0


JSON_KEYS = ["width", "height", "passes", "gpus", "paths", "traversals", "vertices", "wall_s", "kernel_ms", "msamples_per_s", "batch_ms",
             "batch_passes", "preview_updates", "preview_updates_on_owning_thread", "preview_event_calls"]


@pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")
def test_driver_writes_the_mask_and_the_ids(scenes, tmp_path):
    sc = scenes["spheres_a169"]
    w, h, spp = 41, 23, 32
    pod = str(tmp_path / "scene.pod")
    sc.write_pod(pod)
    common = [BIN, "-w", str(w), "-h", str(h), "--passes", "3", "--spp", str(spp), "--gpus", "1", "--scene-pod", pod, "--strict", "--json"]
    plain_png, matte_png = str(tmp_path / "plain.png"), str(tmp_path / "matte.png")
    mask_pfm, ids_pfm = str(tmp_path / "mask.pfm"), str(tmp_path / "ids.pfm")
    p = subprocess.run(common + ["-o", plain_png], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    assert list(json.loads(p.stdout.strip().splitlines()[-1])) == JSON_KEYS  # (what they were)
    p = subprocess.run(common + ["-o", matte_png, "--matte-mask", mask_pfm, "--matte-objects", "3,4,7", "--matte-ids", ids_pfm],
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    assert list(stats) == JSON_KEYS + ["matte_samples", "matte_dropped_pixels"]
    assert open(plain_png, "rb").read() == open(matte_png, "rb").read()
    with HipRenderer(sc, w, h, spp=spp, seed=SEED, strict=True, aov=True, matte=True) as r:
        r.render(3)
        mask, dominant = r.matte_mask([3, 4, 7])
        m = r.matte()
    assert (mask > 0).any()
    assert bits_equal(read_pfm(mask_pfm)[..., 0], mask) and bits_equal(read_pfm(ids_pfm)[..., 0], dominant)
    assert stats["matte_samples"] == m["samples"] == 75 and stats["matte_dropped_pixels"] == int((m["dropped"] > 0).sum())
    # --aov-specular is honoured, and alone with a matte option it is accepted
    p = subprocess.run(common + ["-o", "", "--matte-ids", ids_pfm, "--aov-specular"], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    with HipRenderer(sc, w, h, spp=spp, seed=SEED, strict=True, aov=True, matte=True, aov_specular=True) as r:
        final = r.render(3).matte_mask([])[1]
    assert not bits_equal(final, dominant) and bits_equal(read_pfm(ids_pfm)[..., 0], final)
    # an id the scene does not have is the library's refusal
    p = subprocess.run(common + ["-o", "", "--matte-mask", mask_pfm, "--matte-objects", "3,100000"], capture_output=True, text=True, timeout=180)
    assert p.returncode == 2 and "out of range" in p.stderr, (p.returncode, p.stderr)
