"""Scenes for the EXACT build's fixed-count kernel instances (kajo_amd/csrc/fixed_counts.h, kernel_exact_fixed.cpp), built where they are used
(tests/test_fixed_kernel_cpu.py pins which kernel each runs; tests/test_hip_fixed_instance.py renders them). A simple one-light scene whose
(planes, spheres) are in the table runs its instance; the same scene with one (centre, radius) sphere more runs kajo_render_exact_simple, the
kernel the instance was stamped from -- and gives the same frame if no ray meets the new sphere."""
import numpy as np

from kajo_amd.scene import Scene, material, sphere_record, translate


def far_sphere_twin(base):
    """(`base` plus a dark (centre, radius) sphere far outside the room, appended LAST; ids): a pure translation, so the scene stays one of rigid
    planes and (centre, radius) spheres (allTranslated = 1), with one sphere more than `base`. ids[old object id] = new object id is the identity:
    nothing in front of the new record moves. In a closed room every ray meets a wall first, and no ray of the wave reaches the new sphere's
    line, so the walk skips it as a wave. Being the last record it IS what a ray that is not a number ends on in STRICT and EXACT (integrator.inc.hip
    trace) where `base` ends such a ray on its own last sphere: the callers check on the oracle that base and twin give one frame before they
    compare kernels."""
    rec = sphere_record(translate(0.0, 500.0, 0.0), material(diffuse=[0.5, 0.5, 0.5]), 0.25)  # (the world is y-down: far below the floor plane)
    ids = np.arange(1 + base.n_planes + base.n_spheres, dtype=np.int32)
    return Scene(base.background, base.view, base.proj, np.concatenate([base.spheres, rec[None]]), base.planes, base.name + "+far_sphere"), ids


def without_a_sphere(base):
    """`base` without its first sphere that is not a light: another image, one sphere fewer, still one light"""
    light = (base.spheres[:, 16:38][:, 12:16] != 0).any(1)
    k = int(np.flatnonzero(~light)[0])
    return Scene(base.background, base.view, base.proj, np.delete(base.spheres, k, axis=0), base.planes, base.name + "-sphere%d" % k)
