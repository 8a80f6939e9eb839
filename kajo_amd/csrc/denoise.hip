// denoise.hip -- edge-aware A-trous denoiser over one handle's whole frame, guided by the first-hit AOVs (kajo_hip_denoise;
// the filter's definition is in include/kajo_hip.h). Dammertz et al. 2010 with the spatial variance estimate of SVGF (Schied et al.
// 2017) scaling the luminance weight. Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, in every numerics build alike: the
// filter's arithmetic is this file's own, so only its inputs depend on FAST / EXACT / STRICT.
//
// One lane per pixel, workgroups of 64x4 pixels. Passes over the frame, each a kernel on the handle's stream:
//   prepare    accumulation (tile buffer, or a row-major frame: fromTiles) + AOV sums -> guide (N.xyz, z) and colour (e.rgb, 0)
//   variance   colour -> colour' (e.rgb, v0): the 3x3 variance of the luminance
//   atrous     one per iteration, step 2^i, colour ping-pong: (e, v) -> (e', v')
//   remodulate colour -> sums in the accumulation's units (in place)
// The accumulation and the AOV buffers are only read.
#include <hip/hip_runtime.h>

#include <math.h>

#include "render_args.h"

namespace
{

constexpr float kAlbedoFloor = 1e-3f;

struct DenoiseFrame
{
    int32_t W, H;
};

__device__ inline bool finite3(float4 c)
{
    return isfinite(c.x) && isfinite(c.y) && isfinite(c.z);
}

__device__ inline float luminance(float4 c)
{
    return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z;
}

// the frame to filter at pixel (x, y): the one owner's tile buffer through the tile map, or a row-major frame (a composed or staged one)
__device__ inline float4 sumAt(const float4* src, const TileMap& map, int fromTiles, int x, int y)
{
    if (!fromTiles)
        return src[(size_t)y * map.W + x];
    int owner;
    uint32_t slot;
    kajoTileSlot(map, x, y, &owner, &slot);
    return src[(size_t)owner * map.slotsPerOwner + slot];
}

__device__ inline float3 albedoOf(float4 A, float samples)
{
    return make_float3(fmaxf(A.x / samples, kAlbedoFloor), fmaxf(A.y / samples, kAlbedoFloor), fmaxf(A.z / samples, kAlbedoFloor));
}

// exp(-num / den) with exp(-0 / den) = 1 for every den (den = 0 included: a zero difference keeps its full weight)
__device__ inline float edgeWeight(float num, float den)
{
    return num == 0.0f ? 1.0f : expf(-(num / den));
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_denoise_prepare(const float4* src, TileMap map, int fromTiles, const float4* albedoHits,
                                                                        const float4* normalDepth, float passes, float samples,
                                                                        int demodulate, float4* guide, float4* colour)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const size_t i = (size_t)y * map.W + x;
    const float4 sum = sumAt(src, map, fromTiles, x, y);
    const float4 A = albedoHits[i];
    const float4 B = normalDepth[i];
    float4 e = make_float4(sum.x / passes, sum.y / passes, sum.z / passes, 0.0f);
    if (demodulate) {
        const float3 a = albedoOf(A, samples);
        e.x = e.x / a.x;
        e.y = e.y / a.y;
        e.z = e.z / a.z;
    }
    const float len2 = B.x * B.x + B.y * B.y + B.z * B.z;
    float4 g = make_float4(0.0f, 0.0f, 0.0f, A.w > 0.0f ? B.w / A.w : 0.0f);
    if (len2 > 0.0f) {
        const float len = sqrtf(len2);
        g.x = B.x / len;
        g.y = B.y / len;
        g.z = B.z / len;
    }
    guide[i] = g;
    colour[i] = e;
}

// v0: the variance of the luminance over the 3x3 window of pixels inside the image with a finite colour, formed about the window's
// mean (the same quantity as E[l^2] - E[l]^2 without its cancellation); 0 at a pixel whose own colour is not finite
extern "C" __global__ void __launch_bounds__(256) kajo_denoise_variance(const float4* colour, DenoiseFrame f, float4* out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= f.W || y >= f.H)
        return;
    const size_t i = (size_t)y * f.W + x;
    float4 c = colour[i];
    float l[9];
    bool ok[9];
    int n = 0;
    float mean = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int qx = x + k % 3 - 1, qy = y + k / 3 - 1;
        ok[k] = false;
        l[k] = 0.0f;
        if (qx >= 0 && qx < f.W && qy >= 0 && qy < f.H) {
            const float4 q = colour[(size_t)qy * f.W + qx];
            if (finite3(q)) {
                ok[k] = true;
                l[k] = luminance(q);
                mean += l[k];
                n++;
            }
        }
    }
    float v = 0.0f;
    if (finite3(c) && n > 0) {
        mean = mean / (float)n;
#pragma unroll
        for (int k = 0; k < 9; k++)
            if (ok[k])
                v += (l[k] - mean) * (l[k] - mean);
        v = v / (float)n;
    }
    c.w = v;
    out[i] = c;
}

// One A-trous iteration at step `step` (include/kajo_hip.h): colour (e.rgb, v) -> out (e'.rgb, v').
extern "C" __global__ void __launch_bounds__(256) kajo_denoise_atrous(const float4* guide, const float4* colour, DenoiseFrame f, int step,
                                                                       float sigmaLuminance, float sigmaNormal, float sigmaDepth, float4* out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= f.W || y >= f.H)
        return;
    const size_t i = (size_t)y * f.W + x;
    const float4 gp = guide[i];
    const float4 cp = colour[i];
    const bool centreFinite = finite3(cp);
    const bool normalP = gp.x != 0.0f || gp.y != 0.0f || gp.z != 0.0f;
    const float lp = luminance(cp);

    // luminance scale: sigmaLuminance * sqrt(g(v)) + 1e-6, g = the [1/4, 1/2, 1/4]^2 blur of v over the 3x3 pixels inside the image with a
    // finite colour, renormalised over them
    float lumDen = 1.0f;
    if (centreFinite) {
        const float h3[3] = {0.25f, 0.5f, 0.25f};
        float gs = 0.0f, gw = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= f.W || qy < 0 || qy >= f.H)
                    continue;
                const float4 q = colour[(size_t)qy * f.W + qx];
                if (!finite3(q))
                    continue;
                const float w = h3[dx + 1] * h3[dy + 1];
                gs += w * q.w;
                gw += w;
            }
        lumDen = sigmaLuminance * sqrtf(gs / gw) + 1e-6f;
    }

    const float h5[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float depthStep = sigmaDepth * (float)step / (float)max(f.W, f.H);
    float sw = 0.0f, sv = 0.0f;
    float3 se = make_float3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int dy = -2; dy <= 2; dy++)
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step, qy = y + dy * step;
            if (qx < 0 || qx >= f.W || qy < 0 || qy >= f.H)
                continue;
            const size_t j = (size_t)qy * f.W + qx;
            const float4 cq = colour[j];
            if (!finite3(cq))
                continue;
            const float4 gq = guide[j];
            float w = h5[dx + 2] * h5[dy + 2];
            if (dx != 0 || dy != 0) {
                const float zmax = fmaxf(fmaxf(gp.w, gq.w), 1e-4f);
                w *= edgeWeight(fabsf(gp.w - gq.w), depthStep * zmax * sqrtf((float)(dx * dx + dy * dy)));
            }
            if (normalP && (gq.x != 0.0f || gq.y != 0.0f || gq.z != 0.0f))
                w *= powf(fmaxf(gp.x * gq.x + gp.y * gq.y + gp.z * gq.z, 0.0f), sigmaNormal);
            if (centreFinite)
                w *= edgeWeight(fabsf(lp - luminance(cq)), lumDen);
            sw += w;
            se.x += w * cq.x;
            se.y += w * cq.y;
            se.z += w * cq.z;
            sv += w * w * cq.w;
        }
    float4 r;
    if (sw > 0.0f) {
        r = make_float4(se.x / sw, se.y / sw, se.z / sw, sv / (sw * sw));
    } else {
        const float nan = __builtin_nanf("");
        r = make_float4(nan, nan, nan, 0.0f);
    }
    out[i] = r;
}

// colour (e.rgb) -> sums in the accumulation's units: e * max(a, 1e-3) * P (demodulated) or e * P; .w from the accumulation. In place
// (colour == out): every lane reads and writes its own pixel only.
extern "C" __global__ void __launch_bounds__(256) kajo_denoise_remodulate(const float4* colour, const float4* src, TileMap map,
                                                                           int fromTiles, const float4* albedoHits, float passes,
                                                                           float samples, int demodulate, float4* out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const size_t i = (size_t)y * map.W + x;
    float4 e = colour[i];
    if (demodulate) {
        const float3 a = albedoOf(albedoHits[i], samples);
        e.x = e.x * a.x;
        e.y = e.y * a.y;
        e.z = e.z * a.z;
    }
    out[i] = make_float4(e.x * passes, e.y * passes, e.z * passes, sumAt(src, map, fromTiles, x, y).w);
}

// The whole filter for iterations >= 1 on `stream`: scratch = three float4 frames (guide, and the two colour buffers the
// iterations alternate between). *result = the frame that holds the result (scratch + 16 W H or + 32 W H). src: the frame to filter, the
// one owner's tile buffer (fromTiles) or row-major.
extern "C" int kajo_denoise_launch(const void* src, const TileMap* map, int fromTiles, const void* albedoHits, const void* normalDepth,
                                   float passes, float samples, int iterations, int demodulate, float sigmaLuminance, float sigmaNormal, float sigmaDepth,
                                   void* scratch, void** result, void* stream)
{
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t frame = (size_t)map->W * map->H;
    float4* guide = static_cast<float4*>(scratch);
    float4* buf[2] = {guide + frame, guide + 2 * frame};
    const DenoiseFrame f = {map->W, map->H};
    const dim3 grid((map->W + 63) / 64, (map->H + 3) / 4), block(256);
    hipLaunchKernelGGL(kajo_denoise_prepare, grid, block, 0, s, static_cast<const float4*>(src), *map, fromTiles,
                       static_cast<const float4*>(albedoHits), static_cast<const float4*>(normalDepth), passes, samples, demodulate, guide, buf[0]);
    hipLaunchKernelGGL(kajo_denoise_variance, grid, block, 0, s, buf[0], f, buf[1]);
    int cur = 1;
    for (int it = 0; it < iterations; it++) {
        hipLaunchKernelGGL(kajo_denoise_atrous, grid, block, 0, s, guide, buf[cur], f, 1 << it, sigmaLuminance, sigmaNormal, sigmaDepth,
                           buf[cur ^ 1]);
        cur ^= 1;
    }
    hipLaunchKernelGGL(kajo_denoise_remodulate, grid, block, 0, s, buf[cur], static_cast<const float4*>(src), *map, fromTiles,
                       static_cast<const float4*>(albedoHits), passes, samples, demodulate, buf[cur]);
    *result = buf[cur];
    return (int)hipGetLastError();
}
