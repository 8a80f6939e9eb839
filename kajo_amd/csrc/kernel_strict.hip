// STRICT numerics: bit-identical to the CPU oracle. Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#define KAJO_STRICT 1
#ifndef KAJO_INLINE_SHADOW
#define KAJO_INLINE_SHADOW 1 // small scenes answer shadow rays inside the light loop (integrator.inc.hip)
#endif
#define KAJO_KERNEL_NAME kajo_render_strict
#ifndef KAJO_STRICT_PRESAMPLE
#define KAJO_STRICT_PRESAMPLE 1 // small scenes of ONE light: their own instance, shadow ray in a trip of its own with the BSDF sampled in the light's visit
#endif
#if KAJO_STRICT_PRESAMPLE
#define KAJO_KERNEL_NAME_LIGHTS kajo_render_strict_lights // small scenes with several lights (or none): shadow walks inside the light loop
#endif
#define KAJO_KERNEL_NAME_BIG kajo_render_strict_big
#define KAJO_KERNEL_NAME_BIGLIST kajo_render_strict_biglist
// Large scenes, STRICT: an instance per home of the grid's cell lists (LDS: _lg; global memory: the plain names), each with typed loads and
// ONE walk -- a walk over a pointer of either home loads FLAT with a full wait behind every cell record, two walks in one kernel spill 20
// registers more. 1000 spheres / 16 lights: 3.25 -> 3.31 G paths/s. (FAST carries both walks in one kernel and measures 0.7 % faster so.)
#define KAJO_KERNEL_NAME_BIG_LG kajo_render_strict_big_lg
#define KAJO_KERNEL_NAME_BIGLIST_LG kajo_render_strict_biglist_lg
#define KAJO_KERNEL_NAME_SPLIT kajo_render_strict_split
#define KAJO_KAT_SHADE_NAME kajo_kat_shade_strict
#define KAJO_KAT_TRACE_NAME kajo_kat_trace_strict
#define KAJO_RESOLVE_NAME kajo_resolve_strict
#define KAJO_RESOLVE_TILES_NAME kajo_resolve_tiles_strict
#include "integrator.inc.hip"
#include "launch.inc.hip"
// first-hit AOVs (KAJO_FLAG_AOV): this instance serves the STRICT and the EXACT handles
#define KAJO_AOV_NAME kajo_aov_strict
#include "aov.inc.hip"
// exposure, tone curves and automatic exposure in the resolve (kajo_hip_tonemap_argb8): these instances serve the STRICT and the EXACT handles
#define KAJO_TONE_SUFFIX _strict
#include "tonemap.inc.hip"

// include/kajo_strictmath.h element-wise on the device (kajo_hip_kat_strictmath): the claim that these
// functions give identical bits on x86-64 and gfx950 is checked directly.
// fn: 0 sin, 1 cos, 2 asin, 3 acos, 4 pow(x, y); 5 x / y and 6 sqrt(x) as the STRICT and EXACT kernels form them (integrator.inc.hip kdiv, ksqrt),
// 7 the root as their sphere tests form it (ksqrtWalk)
extern "C" __global__ void __launch_bounds__(256) kajo_kat_math(int fn, int n, const float* x, const float* y, float* out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    float r;
    switch (fn) {
    case 0: r = kajo_sinf(x[i]); break;
    case 1: r = kajo_cosf(x[i]); break;
    case 2: r = kajo_asinf(x[i]); break;
    case 3: r = kajo_acosf(x[i]); break;
    case 5: r = kdiv(x[i], y[i]); break;
    case 6: r = ksqrt(x[i]); break;
    case 7: r = ksqrtWalk(x[i]); break;
    default: r = kajo_powf(x[i], y[i]); break;
    }
    out[i] = r;
}

extern "C" int kajo_kat_math_launch(int fn, int n, const void* x, const void* y, void* out, void* stream)
{
    hipLaunchKernelGGL(kajo_kat_math, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), fn, n,
                       static_cast<const float*>(x), static_cast<const float*>(y), static_cast<float*>(out));
    return (int)hipGetLastError();
}

// The same functions over EVERY binary32 argument (kajo_hip_kat_strictmath_sweep): binade b = sign * 256 + biased exponent holds the
// arguments with bits b << 23 | m, m = 0 .. 2^23 - 1, and gets two checksums over its results r(m) -- A = sum bits(r), B = sum bits(r) *
// (2 m + 1), both mod 2^64, a NaN counted as 0x7fc00000 (its sign and payload are not part of the contract) -- which the host build of
// the same header must reproduce word for word (tools/strictmath_binades.c, tests/golden/strictmath_binades.npz). B weighs a result
// with its position: two results swapped inside a binade leave A alone and move B.
// 64 workgroups a binade, 512 arguments a lane; a workgroup writes ONE partial pair and the host adds the 64 of a binade (no atomics).
// fn as above without 5 (binary); y is pow's exponent.
#define KAJO_SWEEP_BLOCKS_PER_BINADE 64
template <int FN>
__device__ __forceinline__ void sweepLane(uint32_t base, float y, uint64_t& A, uint64_t& B)
{
    for (uint32_t it = 0; it < 512u; it++) {
        const uint32_t u = base + (it << 8);
        const float x = __builtin_bit_cast(float, u);
        float r;
        if (FN == 0) r = kajo_sinf(x);
        else if (FN == 1) r = kajo_cosf(x);
        else if (FN == 2) r = kajo_asinf(x);
        else if (FN == 3) r = kajo_acosf(x);
        else if (FN == 6) r = ksqrt(x);
        else if (FN == 7) r = ksqrtWalk(x);
        else r = kajo_powf(x, y);
        const uint64_t bits = r != r ? 0x7fc00000u : __builtin_bit_cast(uint32_t, r);
        A += bits;
        B += bits * (uint64_t)(2u * (u & 0x7fffffu) + 1u);
    }
}

extern "C" __global__ void __launch_bounds__(256) kajo_kat_math_sweep(int fn, float y, unsigned long long* partial)
{
    const uint32_t binade = blockIdx.x / KAJO_SWEEP_BLOCKS_PER_BINADE, chunk = blockIdx.x % KAJO_SWEEP_BLOCKS_PER_BINADE;
    const uint32_t base = (binade << 23) | (chunk << 17) | threadIdx.x; // 2^23 / 64 = 2^17 arguments a workgroup, lanes interleaved
    uint64_t A = 0, B = 0;
    switch (fn) {
    case 0: sweepLane<0>(base, y, A, B); break;
    case 1: sweepLane<1>(base, y, A, B); break;
    case 2: sweepLane<2>(base, y, A, B); break;
    case 3: sweepLane<3>(base, y, A, B); break;
    case 6: sweepLane<6>(base, y, A, B); break;
    case 7: sweepLane<7>(base, y, A, B); break;
    default: sweepLane<4>(base, y, A, B); break;
    }
    __shared__ unsigned long long sums[2 * 256];
    sums[threadIdx.x] = A;
    sums[256 + threadIdx.x] = B;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            sums[threadIdx.x] += sums[threadIdx.x + w];
            sums[256 + threadIdx.x] += sums[256 + threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = sums[0];
        partial[2 * (size_t)blockIdx.x + 1] = sums[256];
    }
}

extern "C" int kajo_kat_math_sweep_launch(int fn, float y, void* partial, void* stream)
{
    hipLaunchKernelGGL(kajo_kat_math_sweep, dim3(512 * KAJO_SWEEP_BLOCKS_PER_BINADE), dim3(256), 0, static_cast<hipStream_t>(stream), fn, y,
                       static_cast<unsigned long long*>(partial));
    return (int)hipGetLastError();
}
