"""The oracle's batched first-hit AOV replay (oracle/kajo_oracle.cpp koracle_aov, what tests/test_hip_aov.py holds the kernels to) pinned
bit for bit to the definition replayed one sample at a time in numpy: every camera ray from oraclelib.camera_ray, its closest hit from the
oracle's trace, and the two float4 sums of include/kajo_hip.h built by a sequential float32 loop in the defined order -- pass order, then
stratum sy * n + sx (np.sum would add pairwise: not that order). No GPU."""
import numpy as np
import pytest

from framelib import bits
from kajo_amd.scene import stress_scene
from oraclelib import OracleLib, available, camera_ray

pytestmark = pytest.mark.skipif(not available("oracle"), reason="oracle/libkajo_oracle.so not built (run __graft_entry__.build())")
SEED = 0o715517


def replay_per_sample(sc, passes, w, h, spp, seed=SEED):
    """(A, B) of include/kajo_hip.h for the passes numbered `passes`, one camera ray at a time."""
    o = OracleLib("oracle").create(sc, 1)
    n = int(np.sqrt(float(spp)))
    mats = np.concatenate([sc.planes[:, 16:38], sc.spheres[:, 16:38]]).astype(np.float32)  # by object id - 1: planes first
    diffuse, specular, transparency = mats[:, 4:7], mats[:, 8:11], mats[:, 16:19]
    lobes = np.minimum(np.maximum((diffuse + specular) + transparency, np.float32(0)), np.float32(1))
    bg = sc.background[:3].astype(np.float32)
    A = np.zeros((h * w, 4), np.float32)
    B = np.zeros((h * w, 4), np.float32)
    for p in passes:
        for s in range(n * n):
            O = np.empty((h * w, 3), np.float32)
            D = np.empty((h * w, 3), np.float32)
            for y in range(h):
                for x in range(w):
                    O[y * w + x], D[y * w + x], _ = camera_ray(o, w, h, spp, x, y, s, npass=p, seed=seed)
            t = o.trace(O, D)
            hit = t["idx"] != 0
            albedo = np.where(hit[:, None], lobes[np.maximum(t["idx"], 1) - 1], bg[None, :]).astype(np.float32)
            normal = np.where(hit[:, None], t["normal"], np.float32(0)).astype(np.float32)
            depth = np.where(hit, t["t"], np.float32(0)).astype(np.float32)
            # one float32 addition per word and sample (a miss adds zeros), in pass and stratum order
            A[:, :3] += albedo
            A[:, 3] += hit.astype(np.float32)
            B[:, :3] += normal
            B[:, 3] += depth
    return A.reshape(h, w, 4), B.reshape(h, w, 4)


def _scene(scenes, which):
    base = scenes["spheres_a169"]
    return {"small": base, "open": scenes["caustics_a169"], "grid60": stress_scene(base, 60, 4)}[which]


@pytest.mark.parametrize("which", ["small", "open", "grid60"])
@pytest.mark.parametrize("shape", [(48, 32, 32, (1, 2)), (13, 11, 16, (3, 70000)), (1, 7, 9, (65535, 65536, 65537))])
def test_batched_replay_is_the_per_sample_replay_bit_for_bit(scenes, which, shape):
    """The whole frame (one and three threads), a rectangle of it, and sums continued pass by pass; pass numbers across 2^16 on the
    small shapes."""
    w, h, spp, passes = shape
    sc = _scene(scenes, which)
    want = replay_per_sample(sc, passes, w, h, spp)
    assert (want[0][..., 3] > 0).any()
    o = OracleLib("oracle").create(sc, 1)
    x0, y0 = w // 3, h // 2
    for threads, rect in ((1, None), (3, None), (2, (x0, y0, w - x0, h - y0))):
        sums = None
        for p in passes:  # one call per pass, each continuing the last
            sums = o.aov(w, h, spp, passes=1, seed=SEED, first_pass=p, rect=rect, sums=sums, threads=threads)
        A, B = want if rect is None else (want[0][y0:, x0:], want[1][y0:, x0:])
        assert np.array_equal(bits(sums[0]), bits(A)), (which, shape, threads, rect, np.argwhere(sums[0] != A)[:4])
        assert np.array_equal(bits(sums[1]), bits(B)), (which, shape, threads, rect, np.argwhere(sums[1] != B)[:4])
    if list(passes) == list(range(passes[0], passes[0] + len(passes))):  # consecutive passes in one call
        A, B = o.aov(w, h, spp, passes=len(passes), seed=SEED, first_pass=passes[0])
        assert np.array_equal(bits(A), bits(want[0])) and np.array_equal(bits(B), bits(want[1]))
