// fixed_counts.h -- the (planes, spheres) pairs the EXACT build has a one-light small-scene kernel instance for whose walk is compiled for
// exactly those counts (kernel_exact_fixed.cpp, integrator.inc.hip trace NP / NS). ONE table: the instances are stamped from it, the launcher
// (launch.inc.hip) picks by it, tools/host_san.cpp `plan kernel` prints its choice and tests/test_fixed_kernel_cpu.py reads it from this text.
// A scene's counts are fixed for its handle's life (kajo_hip_create stages the scene once): the same footing as allTranslated / planesRigid.
// Plain host arithmetic, no HIP. At most three entries: each is a whole render kernel in build time and library size.
//   (6, 5): the closed room of six walls and five spheres -- every one-light scene of the reference's data/, the benchmarked frame among them
#ifndef KAJO_FIXED_COUNTS_H
#define KAJO_FIXED_COUNTS_H

#define KAJO_FIXED_COUNTS(X) X(6, 5)

#define KAJO_FIXED_NAME(P, S) kajo_render_exact_p##P##s##S

// the instance of a simple one-light scene (rigid planes, (centre, radius) spheres, whole scene in LDS) of these counts, or null: it
// runs kajo_render_exact_simple
static inline const char* kajoFixedKernelName(int nPlanes, int nSpheres)
{
#define KAJO_FIXED_PICK(P, S) \
    if (nPlanes == P && nSpheres == S) \
        return "kajo_render_exact_p" #P "s" #S;
    KAJO_FIXED_COUNTS(KAJO_FIXED_PICK)
#undef KAJO_FIXED_PICK
    return nullptr;
}

#endif
