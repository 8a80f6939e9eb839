"""The EXACT build has two one-light kernels for small scenes (integrator.inc.hip trace SIMPLE; launch.inc.hip picks): kajo_render_exact_simple
(kernel_exact_simple.cpp) for scenes of rigid planes and (centre, radius) spheres, without the loops for general records, and
kajo_render_exact for every other scene. Both must take the oracle's decisions. A (centre, radius) sphere walked by the general loop is,
operation for operation, the record's own arithmetic with a determinant of exactly 1: so the one-light scene with ONE sphere far
outside the room turned -- which no ray meets, but which sends the whole scene to the kernel of general scenes -- must give the simple
kernel's frame bit for bit, at frames of one and of several blocks and in the unsplit kernel too."""
import numpy as np
import pytest

from kajo_amd import capi
from kajo_amd.renderer import HipRenderer
from kajo_amd.scene import Scene, material, sphere_record

pytestmark = pytest.mark.gpu

SEED = 0o715517


def with_turned_sphere(base):
    """`base` plus a dark sphere far behind the camera's room under a rotation about y: a general record no ray can reach"""
    c, s = np.float32(np.cos(0.3)), np.float32(np.sin(0.3))
    M = np.eye(4, dtype=np.float32)
    M[0, 0], M[0, 2], M[2, 0], M[2, 2] = c, s, -s, c
    M[:3, 3] = (0.0, 500.0, 0.0)  # (the world is y-down: far below the floor plane)
    rec = sphere_record(M.T.reshape(16).copy(), material(diffuse=[0.5, 0.5, 0.5]), 0.25)
    return Scene(base.background, base.view, base.proj, np.concatenate([base.spheres, rec[None]]), base.planes, "turned")


@pytest.mark.parametrize("shape", [(64, 16, 3), (16, 16, 2), (72, 40, 5)])
def test_the_general_kernel_gives_the_simple_kernels_frame(scenes, shape):
    base = scenes["spheres_a169"]
    assert base.n_lights == 1
    gen = with_turned_sphere(base)
    w, h, passes = shape
    for flags in (0, capi.KAJO_FLAG_NO_SPLIT):
        frames = []
        for sc in (base, gen):
            with HipRenderer(sc, w, h, spp=16, seed=SEED, exact=True, flags=flags, counters=True) as r:
                frames.append((r.render(passes).radiance()[..., :3].copy(), r.counters()))
        (a, ca), (b, cb) = frames
        assert np.isfinite(a).all(-1).mean() > 0.99
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (shape, flags)
        assert (ca["traversals"], ca["vertices"]) == (cb["traversals"], cb["vertices"])
