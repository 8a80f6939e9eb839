"""GPU test of the C++ host side (kajo_amd/host): hip::Scheduler behind Kajo's Scheduler interface,
driven by the headless kajo_render binary, must give exactly the frame the C ABI gives directly."""
import json
import os
import subprocess

import numpy as np
import pytest

from framelib import read_png
from kajo_amd.renderer import HipRenderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kajo_amd", "host", "kajo_render")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(BIN), reason="kajo_render not built")]


def run(tmp_path, *extra):
    out, raw = str(tmp_path / "o.png"), str(tmp_path / "o.raw")
    cmd = [BIN, "-w", "96", "-h", "54", "-r", "hip", "--passes", "2", "-o", out, "--raw", raw, "--json", *extra,
           os.path.join(ROOT, "kajo_amd", "data", "caustics.json")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    return np.fromfile(raw, np.float32).reshape(54, 96, 4), read_png(out), stats


def test_driver_matches_c_abi(tmp_path, scenes):
    acc, png, stats = run(tmp_path)
    assert stats["passes"] == 2 and stats["paths"] == 96 * 54 * 25 * 2
    sc = scenes["caustics_a169"]
    from kajo_amd.scene import Scene
    import numpy as _np
    z = _np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    strict_parse = Scene.from_npz(z, "caustics_a169/strict_")  # what the host loader produces, bit for bit
    with HipRenderer(strict_parse, 96, 54, exact=True) as r:  # hip::Options::numerics defaults to Exact (round 5)
        want = r.render(2).radiance()
        px = r.argb8()
    assert np.array_equal(acc.view(np.uint32), want.view(np.uint32))
    # PNG bytes are R, G, B, A of the ARGB8 pixels (renderer/Image.cpp:34-38)
    assert np.array_equal(png[..., 0], (px >> 16) & 255) and np.array_equal(png[..., 1], (px >> 8) & 255)
    assert np.array_equal(png[..., 2], px & 255) and (png[..., 3] == 255).all()


@pytest.mark.parametrize("extra", [("--gpus", "2", "--same-device"), ("--gpus", "3", "--same-device", "--batch", "2"), ("--batch", "2")])
def test_tile_owners_and_batching_do_not_change_the_frame(tmp_path, extra):
    base, _, _ = run(tmp_path)
    acc, _, _ = run(tmp_path, *extra)
    assert np.array_equal(acc.view(np.uint32), base.view(np.uint32))


def test_rccl_gather_call_sequence_on_one_gpu(tmp_path):
    # hip::Scheduler's RCCL path (ncclCommInitAll, grouped ncclSend / ncclRecv into the gather buffer, kajo_hip_compose)
    # run with ONE owner: rank 0 sends its tile buffer to itself. Exactly the N > 1 call sequence; the frame must be the
    # no-gather frame bit for bit. (The driver's 8-GPU run must not be this code's first execution.)
    base, png0, _ = run(tmp_path)
    acc, png1, stats = run(tmp_path, "--force-gather", "--gather", "rccl")
    assert stats["gpus"] == 1
    assert np.array_equal(acc.view(np.uint32), base.view(np.uint32))
    assert np.array_equal(png0, png1)
    acc, _, _ = run(tmp_path, "--force-gather", "--gather", "copy", "--batch", "1")
    assert np.array_equal(acc.view(np.uint32), base.view(np.uint32))


def test_three_argument_constructor_takes_the_whole_node(tmp_path, scenes):
    """The form a Kajo checkout constructs -- new hip::Scheduler(scene, image.get(), preview.get()), renderer/Main.cpp:135-142 as
    integration/apply_to_kajo.sh patches it -- has no options: it deals the frame to EVERY visible GPU (one here; KAJO_HIP_GPUS
    caps it), gathers with RCCL, and runs until the preview closes. Same frame as the C ABI gives directly; the scene travels
    as a flat image of scene::Scene (--scene-pod), so the JSON loader is not part of what is compared."""
    import torch
    sc = scenes["spheres_a169"]
    pod = str(tmp_path / "scene.pod")
    sc.write_pod(pod)
    out, raw = str(tmp_path / "o.png"), str(tmp_path / "o.raw")
    cmd = [BIN, "-w", "160", "-h", "90", "-r", "hip", "--passes", "3", "--three-arg", "-o", out, "--raw", raw, "--json", "--scene-pod", pod]
    env = {k: v for k, v in os.environ.items() if k != "KAJO_HIP_GPUS"}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=env)
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    # (the form has no pass budget: it refreshes until the "window" closes -- the headless preview does after 3 passes -- and a
    # refresh renders as many passes as fit a 30 Hz frame, so it may overshoot by part of a batch, as the reference's loop does)
    assert stats["gpus"] == torch.cuda.device_count() and 3 <= stats["passes"] <= 3 + 16
    acc = np.fromfile(raw, np.float32).reshape(90, 160, 4)
    # (rendered here launch by launch as the scheduler rendered it; since round 6 the cut no longer matters -- tests/test_hip_pass_cuts.py)
    with HipRenderer(sc, 160, 90, exact=True) as r:  # the form's numerics: EXACT (the reference's decisions on every path)
        for b in stats["batch_passes"]:
            r.render(b)
        want = r.radiance()
    assert sum(stats["batch_passes"]) == stats["passes"]
    assert np.array_equal(acc.view(np.uint32), want.view(np.uint32))
    # ... unless the environment names another build (the form has no options)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=dict(env, KAJO_HIP_NUMERICS="fast"))
    assert p.returncode == 0, p.stderr
    with HipRenderer(sc, 160, 90) as r:
        for b in json.loads(p.stdout.strip().splitlines()[-1])["batch_passes"]:
            r.render(b)
        want = r.radiance()
    assert np.array_equal(np.fromfile(raw, np.float32).reshape(90, 160, 4).view(np.uint32), want.view(np.uint32))
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=dict(env, KAJO_HIP_NUMERICS="double"))
    assert p.returncode == 2 and "KAJO_HIP_NUMERICS" in p.stderr
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=dict(env, KAJO_HIP_GPUS="1"))
    assert p.returncode == 0 and json.loads(p.stdout.strip().splitlines()[-1])["gpus"] == 1
    # The form's MULTI-GPU code -- ncclCommInitAll, grouped send / receive, the image resolved from the gathered tile buffers, host copy --
    # run here with one owner sending to itself (round-4 advisor finding: on a one-GPU box the default took the no-gather shortcut, so
    # the path a node runs had never executed through this constructor). Same frame, same image.
    out2, raw2 = str(tmp_path / "g.png"), str(tmp_path / "g.raw")
    cmd2 = [c if c not in (out, raw) else (out2 if c == out else raw2) for c in cmd]
    p = subprocess.run(cmd2, capture_output=True, text=True, timeout=180, env=dict(env, KAJO_HIP_FORCE_GATHER="1"))
    assert p.returncode == 0, p.stderr
    st2 = json.loads(p.stdout.strip().splitlines()[-1])
    with HipRenderer(sc, 160, 90, exact=True) as r:
        for b in st2["batch_passes"]:
            r.render(b)
        want2 = r.radiance()
        px2 = r.argb8()
    assert np.array_equal(np.fromfile(raw2, np.float32).reshape(90, 160, 4).view(np.uint32), want2.view(np.uint32))
    png = read_png(out2)
    assert np.array_equal(png[..., 0], (px2 >> 16) & 255) and np.array_equal(png[..., 1], (px2 >> 8) & 255) and np.array_equal(png[..., 2], px2 & 255)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=dict(env, KAJO_HIP_GPUS=str(torch.cuda.device_count() + 1)))
    assert p.returncode == 2 and "KAJO_HIP_GPUS" in p.stderr


def test_driver_numerics_flags(tmp_path):
    """kajo_render --fast / --exact (default) / --strict select the three numerics builds of include/kajo_hip.h."""
    from kajo_amd.scene import Scene
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")
    for flag, kw in (("--fast", {}), ("--exact", {"exact": True}), ("--strict", {"strict": True})):
        acc, _, _ = run(tmp_path, flag)
        with HipRenderer(sc, 96, 54, **kw) as r:
            want = r.render(2).radiance()
        assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)), flag


def test_driver_matches_oracle_strict(tmp_path):
    # the C++ host path end to end (loader -> hip::Scheduler -> C ABI -> STRICT kernels) against the CPU oracle itself
    from oraclelib import OracleLib, available
    if not available("oracle"):
        pytest.skip("oracle not built")
    from kajo_amd.scene import Scene
    acc, _, _ = run(tmp_path, "--strict")
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "caustics_a169/strict_")
    want = OracleLib("oracle").create(sc, 1).render(96, 54, S=32, passes=2)
    assert np.array_equal(acc[..., :3].view(np.uint32), want[..., :3].view(np.uint32))


def test_unknown_renderer_and_bad_scene(tmp_path):
    p = subprocess.run([BIN, "-r", "gl"], capture_output=True, text=True)
    assert p.returncode == 1 and "Unknown renderer" in p.stderr   # renderer/Main.cpp:139-142
    bad = tmp_path / "bad.json"
    bad.write_text("[]")
    p = subprocess.run([BIN, str(bad)], capture_output=True, text=True)
    assert p.returncode == 1 and "Failed to parse scene" in p.stderr  # renderer/Main.cpp:126-129


def test_window_closed_mid_run(tmp_path, scenes):
    """The reference's only stopping condition is its window (renderer/cpu/Scheduler.cpp:74: `while (preview->processEvents())`,
    Esc in renderer/Preview.cpp:216-234), and it shows every pass as it completes (Preview::update, :79-98, on the main thread: SDL).
    The headless stand-in closes at its K-th processEvents() call, mid-run, whatever the pass count is then: hip::Scheduler::run()
    must return without starting another launch (it overshoots by at most the launch in flight: one batch), must have called
    update() for every pass, in order, on the calling thread, and Image::pixels must hold the frame of the passes it reported."""
    sc = scenes["spheres_a169"]
    pod = str(tmp_path / "scene.pod")
    sc.write_pod(pod)
    out, raw = str(tmp_path / "o.png"), str(tmp_path / "o.raw")
    # no pass budget (--passes 0: until the window closes), batches of 3 passes, the window closes at the 5th look at the event queue
    cmd = [BIN, "-w", "160", "-h", "90", "-r", "hip", "--passes", "0", "--batch", "3", "--close-at-event", "5", "--gpus", "1", "-o", out, "--raw", raw,
           "--json", "--scene-pod", pod]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["preview_event_calls"] == 5           # asked once per batch, before it; the fifth answer ended the loop
    assert st["batch_passes"] == [3, 3, 3, 3] and st["passes"] == 12
    assert st["preview_updates"] == list(range(1, 13)) and st["preview_updates_on_owning_thread"] is True
    with HipRenderer(sc, 160, 90, exact=True) as r:
        for b in st["batch_passes"]:
            r.render(b)
        want = r.radiance()
        px = r.argb8()
    assert np.array_equal(np.fromfile(raw, np.float32).reshape(90, 160, 4).view(np.uint32), want.view(np.uint32))
    png = read_png(out)  # Image::pixels as run() left it: the last resolved frame, all 12 passes
    assert np.array_equal(png[..., 0], (px >> 16) & 255) and np.array_equal(png[..., 1], (px >> 8) & 255) and np.array_equal(png[..., 2], px & 255)
    # the automatic batch (no --batch): a window that is open gets a refresh per ~33 ms, never a launch of more than 16 passes
    cmd = [BIN, "-w", "160", "-h", "90", "-r", "hip", "--passes", "0", "--close-at-event", "4", "--gpus", "1", "-o", "", "--json", "--scene-pod", pod]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(st["batch_passes"]) == 3 and st["batch_passes"][0] == 1 and max(st["batch_passes"]) <= 16
    assert st["preview_updates"] == list(range(1, st["passes"] + 1))


def test_launches_of_a_large_scene_are_bounded(tmp_path, scenes):
    """A launch cannot be interrupted, so its length bounds how late run() notices anything. Round 4 launched 16 passes at a time
    without a preview whatever they cost (the 1000-sphere scene at 4K: 0.6 s per launch). Now the batch follows the measured time per
    pass: toward a 30 Hz refresh while a window is open, toward half a second with a null Preview*."""
    from kajo_amd.scene import stress_scene
    sc = stress_scene(scenes["spheres_a169"], 1000, 16)
    pod = str(tmp_path / "scene.pod")
    sc.write_pod(pod)
    base = [BIN, "-w", "2560", "-h", "1440", "-r", "hip", "--gpus", "1", "-o", "", "--json", "--scene-pod", pod, "--fast"]
    p = subprocess.run(base + ["--passes", "24"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["passes"] == 24 and st["batch_passes"][0] == 1 and sum(st["batch_passes"]) == 24
    assert max(st["batch_ms"][2:]) < 150.0, st["batch_ms"]   # planned for ~33 ms from the running estimate
    p = subprocess.run(base + ["--passes", "40", "--no-preview"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["passes"] == 40 and st["batch_passes"][0] == 2 and sum(st["batch_passes"]) == 40
    assert max(st["batch_ms"][1:]) < 900.0 and max(st["batch_passes"]) <= 16, (st["batch_ms"], st["batch_passes"])
    assert st["preview_updates"] == []  # nobody to tell
