"""kajo_hip_reset clears everything that sums passes (kajo_amd/csrc/capi.cpp clearAccumulators): a handle with every accumulating buffer --
COUNTERS | AOV | AOV_SPECULAR | AOV_MATTE | AOV_TILED | NOISE | ADAPTIVE, EXACT, 41x23, S = 4, spheres_a169, the adaptive rule of the case
spheres-S4-ppl16 (tests/adaptive_shape_cases.py), under which a unit retires at pass 16 -- rendered 32 passes, reset and rendered 32
again holds, in every reader, the bits of a fresh handle's 32 passes: the tile buffer, the AOV and matte tile buffers, the noise moments,
the adaptive state and pass plane; and its counters say 32 passes. As owner 0 of 1 and as owner 1 of 3. A buffer the reset forgot would
hold 64 passes' sums, or the first run's retirements."""
import ctypes as C

import numpy as np
import pytest

from kajo_amd.renderer import HipRenderer
from adaptive_shape_cases import PASSES
from test_hip_adaptive import FLOOR, SEED, same_records, u32
from test_hip_adaptive_launch_shapes import plan_of

pytestmark = pytest.mark.gpu

CASE = "spheres-S4-ppl16"
HIP = None


def device_words(ptr, nbytes):
    global HIP
    HIP = HIP or C.CDLL("libamdhip64.so")
    out = np.zeros(nbytes // 4, np.uint32)
    assert nbytes % 4 == 0 and nbytes > 0
    assert HIP.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), C.c_int(2)) == 0
    return out


def readers(r):
    """everything a caller can read of what the handle has summed"""
    r.wait()
    aov, aov_bytes, matte, matte_bytes = r.aov_tile_buffers()
    return dict(tiles=device_words(*r.tile_buffer()), aov_tiles=device_words(aov, aov_bytes), matte_tiles=device_words(matte, matte_bytes),
                moments=r.noise_moments(), state=r.adapt_state(), passes=r.adapt_passes(), counters=r.counters())


@pytest.mark.parametrize("owner,owners", [(0, 1), (1, 3)], ids=["owner-0-of-1", "owner-1-of-3"])
def test_a_reset_handle_renders_what_a_fresh_one_renders_in_every_reader(scenes, owner, owners):
    sc, W, H, S, kw, _, _, _, target = plan_of(scenes, CASE)
    assert (W, H, S) == (41, 23, 4) and kw == dict(exact=True, passes_per_launch=16)
    make = lambda: HipRenderer(sc, W, H, spp=S, seed=SEED, counters=True, aov=True, aov_specular=True, matte=True, aov_tiled=True, noise=True,
                               adaptive=dict(target=target, floor=FLOOR, allowance=0), tile_index=owner, tile_count=owners, **kw)
    with make() as fresh:
        want = readers(fresh.render(PASSES))
    with make() as r:
        r.render(PASSES)
        r.reset()
        assert r.adapt_state()["activeUnits"] == r.adapt_state()["units"] and r.counters()["passes"] == 0
        got = readers(r.render(PASSES))
    s = want["state"]
    # (the first retirement is at 16: plan_of; owner 1 of 3 has the frame's lower tile, most of it outside the image)
    assert s["activeUnits"] < s["units"] and s["lastDecisionPass"] >= 16, s
    if owners == 1:
        assert s["activeUnits"] > 0 and s["lastDecisionPass"] == PASSES, s
    assert want["tiles"].any() and want["aov_tiles"].any() and want["matte_tiles"].any() and want["moments"]["n"].any()
    for k in ("tiles", "aov_tiles", "matte_tiles", "passes"):
        assert np.array_equal(u32(got[k]), u32(want[k])), (k, np.flatnonzero(u32(got[k]).ravel() != u32(want[k]).ravel())[:8])
    assert same_records(got["moments"], want["moments"])
    assert got["state"] == want["state"], (got["state"], want["state"])
    assert got["counters"]["passes"] == PASSES == want["counters"]["passes"]
    for k in ("paths", "traversals", "vertices", "laneSlots", "shadowQueries", "launches"):
        assert got["counters"][k] == want["counters"][k], (k, got["counters"], want["counters"])
