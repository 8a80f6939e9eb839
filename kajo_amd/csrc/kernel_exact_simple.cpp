// EXACT numerics, one kernel in a unit of its own: kajo_render_exact_simple, the one-light small-scene kernel (kernel_exact.hip's
// kajo_render_exact) for scenes of rigid planes and (centre, radius) spheres -- every scene of the reference's data/ -- without the loops
// for general sphere records and scaled planes (integrator.inc.hip trace SIMPLE): 2278 -> 1959 static vector instructions, +1.7 % on the
// benchmarked frame (profiles/r07_retire.txt). kernel_exact.hip's launcher sends such scenes here; its own kernels are what they were.
// HIP source (-x hip); build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, kernel_exact.hip's flags.
#define KAJO_STRICT 1
#define KAJO_EXACT 1
#ifndef KAJO_WAVES_PER_SIMD
#define KAJO_WAVES_PER_SIMD 5 // as kernel_exact.hip: 96 VGPRs, nothing spilled (tests/test_simple_kernel_resources_cpu.py)
#endif
#define KAJO_SIMPLE_KERNEL_NAME kajo_render_exact_simple
#include "integrator.inc.hip"

#include <mutex>

extern "C" int kajo_render_exact_simple_launch(const RenderArgs* args, unsigned grid, unsigned block, size_t ldsBytes, void* stream)
{
    hipLaunchKernelGGL(kajo_render_exact_simple, dim3(grid), dim3(block), ldsBytes, static_cast<hipStream_t>(stream), *args);
    return (int)hipGetLastError();
}

// Dynamic LDS above the default: raised only, remembered per device, as launch.inc.hip's _set_lds (which calls this with the same bytes).
extern "C" int kajo_render_exact_simple_set_lds(size_t ldsBytes)
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
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kajo_render_exact_simple), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    if (e == hipSuccess)
        highWaterOfDevice[device] = ldsBytes;
    return (int)e;
}
