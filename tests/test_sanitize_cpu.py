"""The host side under AddressSanitizer + UBSan (SURVEY.md section 5 "race detection / sanitizers"; CPU only: GPU sanitizers are not
available on the pool). tools/host_san.cpp is compiled from the PRODUCT's own sources -- kajo_amd/csrc/stage.cpp (object records, grid,
visibility lists), kajo_amd/host/scene/SceneLoader.cpp (Kajo's JSON dialect), kajo_amd/csrc/launch_order.h (cost order, parted launch
tail), launch_plan.h (LDS plan, launch shape) and render_args.h (tile slots, side-buffer slots) -- with -fsanitize=address,undefined and run
on the tests' scenes; the launch order, the launch shape and the side-buffer slots are also checked against a model written here."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("san")
    exe = str(d / "host_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "kajo_amd", "csrc"),
           "-I" + os.path.join(ROOT, "kajo_amd", "host"), os.path.join(ROOT, "tools", "host_san.cpp"),
           os.path.join(ROOT, "kajo_amd", "csrc", "stage.cpp"), os.path.join(ROOT, "kajo_amd", "host", "scene", "SceneLoader.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(*args, timeout=600):
        p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert p.returncode == 0, "host_san %s -> %d\n%s\n%s" % (" ".join(map(str, args)), p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        return p.stdout

    run.dir = d
    return run


@pytest.fixture(scope="module")
def stage_pods(san, scenes):
    """the tests' scenes as .pod files: -> their paths"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from kajo_amd.scene import stress_scene
    from test_shadow_lists_cpu import adversarial_scene
    a = scenes["spheres_a169"]
    files = []
    for name, sc in [("spheres", a), ("dialect", scenes["dialect_a1"]), ("caustics", scenes["caustics_a169"]), ("test", scenes["test_a1"]),
                     ("stress1000", stress_scene(a, 1000, 16)), ("stress300", stress_scene(a, 300, 8, seed=77)), ("stress120", stress_scene(a, 120, 1, seed=3))] + \
                    [("adv%d" % s, adversarial_scene(a, s)) for s in (1, 2, 3, 4)]:
        path = str(san.dir / (name + ".pod"))
        sc.write_pod(path)
        files.append(path)
    return files


def test_scene_staging(san, stage_pods):
    out = san("stage", *stage_pods)
    assert out.count(": ok") == 2 * len(stage_pods)


def test_general_grid_staging(san, scenes):
    """tests/general_grid_scenes.py's entries -- large scenes of general records that keep the grid: whole-box registration, four-word hot
    records behind sphereHotOffset, no visibility lists --, the open twin and a nudged twin that gets no grid: staged and planned clean.
    (Pods of their own: stage_pods' set is the key set of tests/golden/lds_plan.json.)"""
    import general_grid_scenes as G
    base = scenes["spheres_a169"]
    made = {name: G.entry(base, name) for name in G.ENTRIES}
    made["mixed_open"] = G.open_twin(made["mixed"])[0]
    made["ellipsoids_nudged"] = G.nudged(made["ellipsoids"], 7, np.diag(np.array([2, .5, 1.0000001], np.float32)), "ellipsoids_nudged")
    files = []
    for name, sc in made.items():
        files.append(str(san.dir / ("general_grid_%s.pod" % name)))
        sc.write_pod(files[-1])
    assert san("stage", *files).count(": ok") == 2 * len(files)
    assert len(san("plan", "lds", *files).splitlines()) == 9 * len(files)
    sizes = san("plan", "sizes", *files).splitlines()
    assert [" grid=1 lists=0 allTranslated=0" in line for line in sizes] == [name != "ellipsoids_nudged" for name in made], sizes
    assert " grid=0 lists=0 allTranslated=0" in sizes[-1]


def test_scene_loader(san):
    files = [os.path.join(ROOT, "kajo_amd", "data", n) for n in ("caustics.json", "dialect.json")]
    files += [os.path.join(ROOT, "tests", "golden", "scenes", n) for n in ("spheres.json", "test.json")]  # the reference's own scene files
    for aspect in (1.0, 1920.0 / 1080.0, 640.0 / 480.0):  # (the aspects of the six parsed scenes of tests/golden/scenes.npz)
        out = san("parse", aspect, *files)
        assert out.count(" spheres ") == len(files)


def model_order(trips, n, w, slots, parts):
    """launch_order.h restated: -> (nParted, order words)"""
    cost = trips.reshape(n, w).max(1) if n else np.zeros(0, np.uint32)
    plain = np.argsort(-cost.astype(np.int64), kind="stable").astype(np.uint32)
    per = slots // w
    n_parted = 0 if (n >= (1 << 28) or n < 2 * per) else min(n // 2, per * 4 // 8)
    if parts < 2 or n_parted == 0:
        return n_parted, plain
    head, tail = plain[:n - n_parted], plain[n - n_parted:]
    words = (tail[:, None] | (np.arange(parts, dtype=np.uint32)[None, :] << 28) | np.uint32(0x80000000)).reshape(-1)
    return n_parted, np.concatenate([head, words]).astype(np.uint32)


@pytest.mark.parametrize("n,w,parts", [(0, 1, 4), (1, 1, 4), (5000, 1, 4), (32400, 1, 4), (32400, 1, 2), (32400, 1, 8), (8100, 4, 3), (129600, 1, 7),
                                       (1 << 22, 1, 8)])
def test_launch_order_and_side_slots(san, n, w, parts):
    rng = np.random.default_rng(n + 7 * w + parts)
    trips = rng.integers(1, 2000, n * w, dtype=np.uint32)
    if n > 100:
        trips[:50] = trips[50]  # ties: equal costs keep image order
    slots, threads = 5120, 64 * w
    src, dst = str(san.dir / "order_in.bin"), str(san.dir / "order_out.bin")
    with open(src, "wb") as f:
        np.array([n, w, slots, parts, threads], np.uint32).tofile(f)
        trips.tofile(f)
    san("order", src, dst)  # (checks inside: every later part's side-buffer slots in range, none taken twice)
    got = np.fromfile(dst, np.uint32)
    n_parted, words = model_order(trips, n, w, slots, parts)
    assert got[0] == n_parted and got[1] == words.size
    assert np.array_equal(got[2:], words)
    if n_parted and parts >= 2:
        # what the fold kernel assumes (aux_kernels.hip): the j-th parted block's parts are physical workgroups partedFirst + j * parts + k,
        # and part k > 0 of it owns slots [(k - 1) * sideStride + j * threads, + threads) of the side buffers
        first = n - n_parted
        phys = np.arange(first, words.size, dtype=np.uint64)
        k = (words[first:] >> 28) & 7
        assert np.array_equal(k, (phys - first) % parts) and (words[first:] >> 31).all() and not (words[:first] >> 28).any()
        j = (phys - first) // parts
        assert np.array_equal(words[first:] & 0x0fffffff, words[first + j * parts] & 0x0fffffff)
        side = (k.astype(np.uint64) - 1) * (n_parted * threads) + j * threads
        assert side[k > 0].max() + threads <= (parts - 1) * n_parted * threads


def test_launch_order_through_the_c_abi():
    """kajo_hip_launch_order (host-only entry point of libkajo_hip.so) returns the same words."""
    import ctypes as C
    from kajo_amd import capi
    L = capi.lib()
    n, w, parts = 20000, 1, 4
    trips = np.random.default_rng(3).integers(1, 500, n * w, dtype=np.uint32)
    n_parted = C.c_uint32()
    need = L.kajo_hip_launch_order(trips.ctypes.data_as(C.c_void_p), n, w, 5120, parts, None, 0, C.byref(n_parted))
    want_parted, words = model_order(trips, n, w, 5120, parts)
    assert need == words.size and n_parted.value == want_parted == 2560
    out = np.zeros(need, np.uint32)
    assert L.kajo_hip_launch_order(trips.ctypes.data_as(C.c_void_p), n, w, 5120, parts, out.ctypes.data_as(C.c_void_p), need, None) == need
    assert np.array_equal(out, words)
    assert L.kajo_hip_launch_order(trips.ctypes.data_as(C.c_void_p), n, w, 5120, parts, out.ctypes.data_as(C.c_void_p), need - 1, None) == capi.KAJO_E_INVALID
    assert L.kajo_hip_launch_order(trips.ctypes.data_as(C.c_void_p), 1 << 28, w, 5120, parts, None, 0, None) == capi.KAJO_E_INVALID


@pytest.mark.parametrize("w,h,tile,owners", [(1920, 1080, (64, 16), 1), (1920, 1080, (64, 16), 8), (200, 70, (32, 8), 3), (3840, 2160, (64, 16), 8),
                                             (1, 1, (64, 16), 2), (8191, 33, (8, 32), 5)])
def test_tile_slots(san, w, h, tile, owners):
    out = san("tiles", w, h, tile[0], tile[1], owners)
    from kajo_amd.tiles import TileLayout
    assert "%d slots per owner" % TileLayout(w, h, owners, tile).slots_per_owner in out


def test_lds_plan(san, stage_pods):
    """launch_plan.h kajoLdsPlan on the staged scenes, per staging and numerics build, against the plans kajo_hip_create made before the
    decision moved out of it (tests/golden/lds_plan.json)."""
    import json
    out = san("plan", "lds", *stage_pods)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "lds_plan.json")))
    got = {}
    for line in out.splitlines():
        head, fields = line.split(": ", 1)
        path, staging, numerics = head.split()
        got["%s %s %s" % (os.path.basename(path)[:-4], staging, numerics)] = {k: int(v) for k, v in (kv.split("=") for kv in fields.split())}
    assert got.keys() == want.keys()
    for key in want:
        assert got[key] == want[key], key


def model_shape(pixel_blocks, now, n, cold_in_lds, no_split, mailbox, per_wave, passes_done, grouped, order_valid, n_parted):
    """launch_plan.h kajoLaunchShape restated: -> (startsInside, endsInside, launchGroups, split, chunks, parted)"""
    starts = grouped and passes_done % 4 != 0
    ends = grouped and (passes_done + now) % 4 != 0
    groups = now // 4 if not starts and not ends else 0
    small = cold_in_lds and not no_split
    split = 1
    if small:
        while pixel_blocks < 3 * 4096 and split < 16 and now % (split * 2) == 0 and pixel_blocks * split * 2 <= 8 * 4096:
            split *= 2
    while split > 1 and mailbox + now * 1024 + split * per_wave > 48 * 1024:
        split //= 2
    chunks = 1
    if small and pixel_blocks < 3 * 4096:
        nn = n * n
        for q in range(2, nn + 1):
            if now * q > 16:
                break
            if nn % q == 0 and pixel_blocks * now * q <= 8 * 4096 and mailbox + now * nn * 1024 + now * q * per_wave <= 48 * 1024:
                chunks = q
                if pixel_blocks * now * q >= 4096:
                    break
        if now * chunks <= split:
            chunks = 1
    parted = chunks == 1 and split == 1 and grouped and order_valid and n_parted > 0 and 2 <= groups <= 8
    return int(starts), int(ends), groups, split, chunks, int(parted)


def test_launch_shape(san):
    """launch_plan.h kajoLaunchShape against its restatement over frame sizes, pass counts and sample counts; with the cases its comments
    document."""
    import itertools
    frames = [(64, 64), (200, 70), (256, 144), (256, 256), (512, 512), (640, 360), (960, 540), (1280, 720), (1920, 1080), (3840, 2160)]
    # (small scene FAST / EXACT: spheres.json's plan; small scene STRICT: stress120's; large scene with lists: stress1000's)
    handles = [(1, 2112, 0, 1), (1, 22528, 0, 0), (0, 27184, 512, 0)]
    cases = []
    for (w, h), now, n, no_split, (cold, mailbox, per_wave, grouped), done, n_parted in itertools.product(
            frames, range(1, 33), (1, 3, 4, 5), (0, 1), handles, (0, 2, 16), (0, 512)):
        pixel_blocks = -(-w // 64) * -(-h // 16) * 16  # 64x16 tiles of sixteen 8x8 blocks
        cases.append((pixel_blocks, now, n, cold, no_split, mailbox, per_wave, done, grouped, 1, n_parted))
    src, dst = str(san.dir / "shape_in.bin"), str(san.dir / "shape_out.bin")
    np.array(cases, np.uint32).tofile(src)
    san("plan", "shape", src, dst)
    got = np.fromfile(dst, np.uint32).reshape(-1, 6)
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert tuple(g) == model_shape(*c), c
    shape = {c: tuple(g) for c, g in zip(cases, got)}
    # BASELINE configs[0]: one pass of 16 samples on 1024 pixel blocks -> four sample chunks per pass
    assert shape[(1024, 1, 4, 1, 0, 2112, 0, 0, 1, 1, 0)][3:5] == (1, 4)
    # 1920x1080 (32640 pixel blocks) at 16 passes: unsplit, four whole groups, the tail parted once the order is known
    assert shape[(32640, 16, 5, 1, 0, 2112, 0, 0, 1, 1, 512)] == (0, 0, 4, 1, 1, 1)
    assert shape[(32640, 16, 5, 1, 1, 2112, 0, 16, 1, 1, 512)] == (0, 0, 4, 1, 1, 1)
    # a launch that ends inside a group of four passes hands it over and is not parted
    assert shape[(32640, 2, 5, 1, 0, 2112, 0, 16, 1, 1, 512)] == (0, 1, 0, 1, 1, 0)
