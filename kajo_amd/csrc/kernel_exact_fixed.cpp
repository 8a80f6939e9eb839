// EXACT numerics, a unit of its own: the instances of kajo_render_exact_simple (kernel_exact_simple.cpp) whose plane and sphere counts are
// compile-time constants -- fixed_counts.h lists them; kajo_render_exact_p6s5 is the benchmarked frame's -- so that the closest-hit walk
// (integrator.inc.hip trace NP / NS) is straight-line code: no counter, compare and branch per primitive, literal hit ids, record reads at
// constant offsets issued ahead of their use. The same operations on the same operands in the same order as the simple kernel, which
// goes on serving every simple one-light scene of other counts and is the twin these are tested against bit for bit
// (tests/test_hip_fixed_instance.py). kernel_exact.hip's launcher sends scenes here by their counts; its own kernels are what they were.
// HIP source (-x hip); build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, kernel_exact.hip's flags.
#define KAJO_STRICT 1
#define KAJO_EXACT 1
#ifndef KAJO_WAVES_PER_SIMD
#define KAJO_WAVES_PER_SIMD 5 // as kernel_exact.hip: 96 VGPRs, nothing spilled (tests/test_fixed_kernel_cpu.py)
#endif
#include "fixed_counts.h"
#define KAJO_FIXED_KERNELS KAJO_FIXED_COUNTS
#define KAJO_FIXED_UNROLL _Pragma("unroll")
#include "integrator.inc.hip"

#include <mutex>

// hipErrorInvalidDeviceFunction: no instance of these counts -- the launcher asks kajoFixedKernelName() first
extern "C" int kajo_render_exact_fixed_launch(const RenderArgs* args, unsigned grid, unsigned block, size_t ldsBytes, void* stream)
{
#define KAJO_FIXED_LAUNCH_ONE(P, S) \
    if (args->scene.nPlanes == P && args->scene.nSpheres == S) { \
        hipLaunchKernelGGL(KAJO_FIXED_NAME(P, S), dim3(grid), dim3(block), ldsBytes, static_cast<hipStream_t>(stream), *args); \
        return (int)hipGetLastError(); \
    }
    KAJO_FIXED_COUNTS(KAJO_FIXED_LAUNCH_ONE)
#undef KAJO_FIXED_LAUNCH_ONE
    return (int)hipErrorInvalidDeviceFunction;
}

// Dynamic LDS above the default: raised only, remembered per device, as launch.inc.hip's _set_lds (which calls this with the same bytes).
extern "C" int kajo_render_exact_fixed_set_lds(size_t ldsBytes)
{
    static size_t highWaterOfDevice[64] = {};
    static std::mutex guard;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess)
        return (int)e;
    if (device < 0 || device >= 64)
        return (int)hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(guard);
    if (ldsBytes <= highWaterOfDevice[device])
        return (int)hipSuccess;
#define KAJO_FIXED_SET_ONE(P, S) \
    if (e == hipSuccess) \
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(KAJO_FIXED_NAME(P, S)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    KAJO_FIXED_COUNTS(KAJO_FIXED_SET_ONE)
#undef KAJO_FIXED_SET_ONE
    if (e == hipSuccess)
        highWaterOfDevice[device] = ldsBytes;
    return (int)e;
}
