"""The tile map on the CPU, at every tile shape the GPU tests use (tests/test_hip_tile_shapes.py) and the default: kajo_amd/tiles.py
TileLayout -- the host mirror that drives the gather and that the GPU tests read raw tile buffers through -- is a bijection between the
image's pixels and distinct in-range slots of the owners' buffers, and kajoTileSlot (kajo_amd/csrc/render_args.h), compiled as host code,
maps every pixel to the same owner and slot. Three of the shapes are not powers of two (3 or 5 waves across a tile, 12 across for 96x8):
there `%` and `/` by tileW >> 3 are not masks and shifts."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from kajo_amd.tiles import TileLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = [(8, 32), (32, 8), (24, 32), (40, 32), (96, 8), (128, 64)]
FRAMES = [(1, 1), (100, 75), (200, 77)]
WORLDS = [1, 2, 3, 8]
CASES = list(itertools.product(TILES + [(64, 16)], FRAMES, WORLDS))


def _id(case):
    (tw, th), (w, h), world = case
    return "%dx%d-%dx%d-%d" % (tw, th, w, h, world)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_layout_is_a_bijection_onto_distinct_slots(case):
    tile, (W, H), world = case
    lay = TileLayout(W, H, world, tile)
    ys, xs = np.mgrid[0:H, 0:W]
    owner, slot = lay.owner_and_slot(xs, ys)
    assert owner.min() >= 0 and owner.max() < world
    assert slot.min() >= 0 and slot.max() < lay.slots_per_owner
    flat = owner.astype(np.int64) * lay.slots_per_owner + slot
    assert np.unique(flat).size == W * H  # injective per owner
    assert sum(lay.owned_pixels(k) for k in range(world)) == W * H
    # the sizes kajo_hip_create derives (capi.cpp), restated: whole tiles, the tile count rounded UP on both axes and over the owners
    tiles = ((W + tile[0] - 1) // tile[0]) * ((H + tile[1] - 1) // tile[1])
    assert lay.n_tiles == tiles and lay.slots_per_owner == ((tiles + world - 1) // world) * tile[0] * tile[1]
    # a wave is one 8x8 pixel block aligned to 8, whatever the tile: its 64 slots are consecutive and start at a multiple of 64
    by, bx = (H - 1) // 8 * 8, (W - 1) // 8 * 8
    for x0, y0 in ((0, 0), (bx, by), (bx, 0), (0, by)):
        o, s = lay.owner_and_slot(xs[y0:y0 + 8, x0:x0 + 8], ys[y0:y0 + 8, x0:x0 + 8])
        assert (o == o[0, 0]).all() and s[0, 0] % 64 == 0
        assert np.array_equal(s - s[0, 0], ((ys[y0:y0 + 8, x0:x0 + 8] & 7) << 3) | (xs[y0:y0 + 8, x0:x0 + 8] & 7))
    # scatter a random frame into the owners' buffers, compose it back
    rng = np.random.default_rng(W * 131 + H * 7 + world + tile[0])
    frame = rng.standard_normal((H, W, 4)).astype(np.float32)
    buffers = np.full((world, lay.slots_per_owner, 4), np.nan, np.float32)
    buffers[owner, slot] = frame
    assert np.array_equal(lay.compose(buffers), frame)
    assert np.isnan(buffers).all(-1).sum() == world * lay.slots_per_owner - W * H  # (and nothing else was written)


SOURCE = r"""
// kajoTileSlot as host code: for every case (W H tileW tileH owners) on the command line, the slots per owner and then (owner, slot)
// of every pixel, row-major, as 32-bit words on stdout. The map is the one kajo_hip_create fills: launch_plan.h kajoFramePlan's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "launch_plan.h"

int main(int argc, char** argv)
{
    for (int a = 1; a + 4 < argc; a += 5) {
        KajoParams p{};
        p.tileW = atoi(argv[a + 2]);
        p.tileH = atoi(argv[a + 3]);
        p.tileCount = atoi(argv[a + 4]);
        const TileMap m = kajoFramePlan(atoi(argv[a]), atoi(argv[a + 1]), p, KajoLdsPlan(), Numerics::Fast).map;
        std::vector<uint32_t> out;
        out.push_back((uint32_t)m.slotsPerOwner);
        for (int y = 0; y < m.H; y++)
            for (int x = 0; x < m.W; x++) {
                int owner;
                uint32_t slot;
                kajoTileSlot(m, x, y, &owner, &slot);
                out.push_back((uint32_t)owner);
                out.push_back(slot);
            }
        if (fwrite(out.data(), sizeof(uint32_t), out.size(), stdout) != out.size())
            return 1;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_slots(tmp_path_factory):
    """-> the words the stand-alone program prints for CASES, one run"""
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("tileslot")
    src, exe = str(d / "tile_slots.cpp"), str(d / "tile_slots")
    with open(src, "w") as f:
        f.write(SOURCE)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "kajo_amd", "csrc"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args = [str(v) for (tw, th), (w, h), world in CASES for v in (w, h, tw, th, world)]
    p = subprocess.run([exe, *args], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    words = np.frombuffer(p.stdout, np.uint32)
    out, at = {}, 0
    for case in CASES:
        _, (w, h), _ = case
        out[case] = (int(words[at]), words[at + 1:at + 1 + 2 * w * h].reshape(h, w, 2))
        at += 1 + 2 * w * h
    assert at == words.size
    return out


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kajo_tile_slot_as_host_code_agrees_with_the_layout(host_slots, case):
    tile, (W, H), world = case
    lay = TileLayout(W, H, world, tile)
    slots_per_owner, got = host_slots[case]
    ys, xs = np.mgrid[0:H, 0:W]
    owner, slot = lay.owner_and_slot(xs, ys)
    assert slots_per_owner == lay.slots_per_owner
    assert np.array_equal(got[..., 0], owner) and np.array_equal(got[..., 1], slot), np.argwhere((got[..., 0] != owner) | (got[..., 1] != slot))[:5]
