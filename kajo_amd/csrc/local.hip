// local.hip -- local tone mapping of one whole frame, between the glare and the meter (kajo_hip_local, kajo_hip_present_local_*; the
// definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, in every numerics build alike: the
// arithmetic is this file's own, so only its inputs depend on FAST / EXACT / STRICT.
//
// One lane per pixel, workgroups of 64x4 pixels, one float per pixel in the planes. Passes, each a kernel on the caller's stream:
//   lambda   source frame F (tile buffers through TileMap, or a row-major frame) -> the plane of log2 luminance; NaN marks a pixel
//            that does not count (a counting pixel's value lies in -16 .. 16)
//   atrous   one per iteration: B_i -> B_{i+1}, 5x5 taps at step 2^i weighted by the B-spline and the range term, renormalised over
//            the taps that are inside the image and count; a pixel that does not count stays NaN
//   apply    out = (m * exp2(L' - L)) P from the source frame, m formed again as `lambda` forms it, L and B_K read from the planes
// Plain gathers from global memory at every step: a plane is 4 bytes a pixel (8 MB at 1920x1080) and a wave's 64 lanes read one
// 256-byte run per tap, so the taps are served by the caches whatever the step. The 25 loads of a lane are issued before the first
// weight is formed. No LDS, no atomics, no cross-lane operation; the sums run in the definition's tap order (dy outer, dx inner). The
// source frame is only read.
#include <hip/hip_runtime.h>

#include <math.h>

#include "render_args.h"

namespace
{

__device__ inline float4 sourcePixel(const float4* src, const TileMap& map, int fromTiles, int x, int y)
{
    if (fromTiles) {
        int owner;
        uint32_t slot;
        kajoTileSlot(map, x, y, &owner, &slot);
        return src[(size_t)owner * map.slotsPerOwner + slot];
    }
    return src[(size_t)y * map.W + x];
}

// m = F.rgb / P; false where the pixel does not count
__device__ inline bool meanOf(float4 F, float passes, float3* m)
{
    *m = make_float3(F.x / passes, F.y / passes, F.z / passes);
    return isfinite(m->x) && isfinite(m->y) && isfinite(m->z);
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_local_lambda(const float4* __restrict__ src, TileMap map, int fromTiles, float passes,
                                                                     float* __restrict__ lambda)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    float3 m;
    float v = __builtin_nanf("");
    if (meanOf(sourcePixel(src, map, fromTiles, x, y), passes, &m)) {
        const float l = (0.2126f * fmaxf(m.x, 0.0f) + 0.7152f * fmaxf(m.y, 0.0f)) + 0.0722f * fmaxf(m.z, 0.0f);
        v = log2f(fminf(fmaxf(l, 0x1p-16f), 0x1p16f));
    }
    lambda[(size_t)y * map.W + x] = v;
}

// B_i -> B_{i+1} at step d
extern "C" __global__ void __launch_bounds__(256) kajo_local_atrous(const float* __restrict__ in, int W, int H, int d, float sigmaRange,
                                                                     float* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H)
        return;
    const size_t at = (size_t)y * W + x;
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float b[25];
    bool inside[25];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int qy = y + (j - 2) * d;
        const bool inY = qy >= 0 && qy < H;
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int qx = x + (i - 2) * d;
            const bool in2 = inY && qx >= 0 && qx < W;
            inside[5 * j + i] = in2;
            b[5 * j + i] = in[in2 ? (size_t)qy * W + qx : at]; // (a tap outside: weight 0, read from the centre)
        }
    }
    const float bp = b[12];
    if (isnan(bp)) {
        out[at] = bp;
        return;
    }
    float sw = 0.0f, sb = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; j++) {
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int k = 5 * j + i;
            const float bq = b[k];
            if (inside[k] && !isnan(bq)) {
                const float t = (bp - bq) / sigmaRange;
                const float wr = k == 12 ? 1.0f : exp2f(-(t * t));
                const float w = (h[i] * h[j]) * wr;
                sw += w;
                sb += w * bq;
            }
        }
    }
    out[at] = sb / sw;
}

// out = (m * exp2(L' - L)) P where the pixel counts, the source pixel where it does not; .w from the source
extern "C" __global__ void __launch_bounds__(256) kajo_local_apply(const float4* __restrict__ src, TileMap map, int fromTiles, float passes,
                                                                    const float* __restrict__ lambda, const float* __restrict__ base,
                                                                    float compression, float detail, float pivot, float4* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const size_t at = (size_t)y * map.W + x;
    const float4 F = sourcePixel(src, map, fromTiles, x, y);
    float4 r = F;
    float3 m;
    if (meanOf(F, passes, &m)) {
        const float L = lambda[at], B = base[at];
        const float mapped = (pivot + compression * (B - pivot)) + detail * (L - B);
        const float g = exp2f(mapped - L);
        r.x = (m.x * g) * passes;
        r.y = (m.y * g) * passes;
        r.z = (m.z * g) * passes;
    }
    out[at] = r;
}

// floats of one plane of a W x H frame (padded to 16 bytes); the stage's scratch is three of them: L, then the two of the ping-pong
extern "C" size_t kajo_local_plane(int W, int H)
{
    return ((size_t)W * H + 3) / 4 * 4;
}

// The stage on `stream`: src (tile buffers, or with fromTiles 0 a row-major frame) -> out (row-major frame, not the source), K =
// iterations in 0 .. 8. planes: three of kajo_local_plane.
extern "C" int kajo_local_launch(const void* src, const TileMap* map, int fromTiles, float passes, int iterations, float compression, float detail,
                                 float sigmaRange, float pivot, void* planes, void* out, void* stream)
{
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (map->W < 1 || map->H < 1 || iterations < 0 || iterations > 8)
        return (int)hipErrorInvalidValue;
    const size_t plane = kajo_local_plane(map->W, map->H);
    float* lambda = static_cast<float*>(planes);
    float* pingPong[2] = {lambda + plane, lambda + 2 * plane};
    const dim3 block(256), grid((map->W + 63) / 64, (map->H + 3) / 4);
    const float4* source = static_cast<const float4*>(src);
    hipLaunchKernelGGL(kajo_local_lambda, grid, block, 0, st, source, *map, fromTiles, passes, lambda);
    const float* base = lambda;
    for (int i = 0; i < iterations; i++) {
        hipLaunchKernelGGL(kajo_local_atrous, grid, block, 0, st, base, map->W, map->H, 1 << i, sigmaRange, pingPong[i & 1]);
        base = pingPong[i & 1];
    }
    hipLaunchKernelGGL(kajo_local_apply, grid, block, 0, st, source, *map, fromTiles, passes, static_cast<const float*>(lambda), base, compression,
                       detail, pivot, static_cast<float4*>(out));
    return (int)hipGetLastError();
}
