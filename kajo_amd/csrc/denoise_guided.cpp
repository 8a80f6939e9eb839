// denoise_guided.cpp -- the noise-guided A-trous denoiser (KAJO_DENOISE_NOISE_GUIDED; the definition is in include/kajo_hip.h under the
// denoiser's). HIP source: hipcc -x hip --offload-arch=gfx950 -O3 -ffp-contract=off, in every numerics build alike. The filter is
// denoise.hip's, kernel for kernel: prepare, the iterations and remodulate are launched from here by declaration, so that a frame on which
// no pixel is measured comes out of the very same code. Only the v0 stage is this unit's own:
//   v0   colour (e.rgb, 0) -> colour' (e.rgb, v0). One lane per pixel, workgroups of 64x4 pixels. The pixel's m and se are the float32 words
//        kajo_hip_noise returns -- evaluated here from the moment record through the TileMap in binary64 (noise.hip's map, expression by
//        expression; 32 bytes a pixel) or read from two uploaded whole-frame planes (8 bytes a pixel). A measured pixel takes
//        (se / m * l(e))^2; any other the 3x3 spatial variance of denoise.hip's variance kernel, its expressions in its order, and only
//        those lanes read the window. No atomics, no LDS, no cross-lane operation.
// The accumulation, the AOV buffers and the records are only read.
#include <hip/hip_runtime.h>

#include <math.h>

#include "render_args.h"

// denoise.hip's frame argument (W, H) and the kernels taken from it
struct KajoGuidedFrame
{
    int32_t W, H;
};
extern "C" __global__ void kajo_denoise_prepare(const float4* src, TileMap map, int fromTiles, const float4* albedoHits, const float4* normalDepth,
                                                 float passes, float samples, int demodulate, float4* guide, float4* colour);
extern "C" __global__ void kajo_denoise_atrous(const float4* guide, const float4* colour, KajoGuidedFrame f, int step, float sigmaLuminance,
                                                float sigmaNormal, float sigmaDepth, float4* out);
extern "C" __global__ void kajo_denoise_remodulate(const float4* colour, const float4* src, TileMap map, int fromTiles, const float4* albedoHits,
                                                    float passes, float samples, int demodulate, float4* out);

namespace
{

// a slot's moment record as its two 16-byte halves (include/kajo_hip.h KajoNoiseMoments)
struct GuidedRecord
{
    double2 s;    // s1, s2
    ulonglong2 c; // n, bad
};
static_assert(sizeof(GuidedRecord) == 32, "include/kajo_hip.h KajoNoiseMoments");

__device__ inline bool finite3(float4 c)
{
    return isfinite(c.x) && isfinite(c.y) && isfinite(c.z);
}

__device__ inline float luminance(float4 c)
{
    return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z;
}

} // namespace

// records != null: the one owner's records through the map; else the planes mean / stdError (row-major, W * H words each)
extern "C" __global__ void __launch_bounds__(256) kajo_denoise_guided_v0(const float4* colour, TileMap map, const GuidedRecord* __restrict__ records,
                                                                          const float* __restrict__ mean, const float* __restrict__ stdError,
                                                                          float4* out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const size_t i = (size_t)y * map.W + x;
    float4 c = colour[i];
    float m, se;
    if (records) {
        // the estimate's evaluation (noise.hip kajo_noise_map), expression by expression
        int owner;
        uint32_t slot;
        kajoTileSlot(map, x, y, &owner, &slot);
        const double2 s = records[slot].s;
        const ulonglong2 cn = records[slot].c;
        const double n = (double)cn.x;
        const double md = cn.x > 0ull ? s.x / (4.0 * n) : 0.0;
        m = (float)md;
        se = -1.0f;
        if (cn.x >= 2ull) {
            const double v = fmax(s.y - s.x * s.x / n, 0.0) / (n - 1.0);
            const double e = sqrt(v / n) / 4.0;
            se = (float)e;
        }
    } else {
        m = mean[i];
        se = stdError[i];
    }
    bool measured = false;
    float v = 0.0f;
    if (finite3(c) && se >= 0.0f && m > 0.0f) {
        const float r = se / m;
        const float t = r * luminance(c);
        v = t * t;
        measured = isfinite(v);
    }
    if (!measured) {
        // denoise.hip kajo_denoise_variance, expression by expression
        float l[9];
        bool ok[9];
        int n = 0;
        float wmean = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const int qx = x + k % 3 - 1, qy = y + k / 3 - 1;
            ok[k] = false;
            l[k] = 0.0f;
            if (qx >= 0 && qx < map.W && qy >= 0 && qy < map.H) {
                const float4 q = colour[(size_t)qy * map.W + qx];
                if (finite3(q)) {
                    ok[k] = true;
                    l[k] = luminance(q);
                    wmean += l[k];
                    n++;
                }
            }
        }
        v = 0.0f;
        if (finite3(c) && n > 0) {
            wmean = wmean / (float)n;
#pragma unroll
            for (int k = 0; k < 9; k++)
                if (ok[k])
                    v += (l[k] - wmean) * (l[k] - wmean);
            v = v / (float)n;
        }
    }
    c.w = v;
    out[i] = c;
}

// kajo_denoise_launch (denoise.hip) with the v0 stage above in the variance kernel's place: the same scratch (three float4 frames), the same
// ping-pong, *result = the frame that holds the result. records: the one owner's moment records, or null with the two device planes.
extern "C" int kajo_denoise_guided_launch(const void* src, const TileMap* map, int fromTiles, const void* albedoHits, const void* normalDepth,
                                          float passes, float samples, int iterations, int demodulate, float sigmaLuminance, float sigmaNormal,
                                          float sigmaDepth, const void* records, const void* mean, const void* stdError, void* scratch, void** result,
                                          void* stream)
{
    if (map->W < 1 || map->H < 1 || (!records && (!mean || !stdError)))
        return (int)hipErrorInvalidValue;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t frame = (size_t)map->W * map->H;
    float4* guide = static_cast<float4*>(scratch);
    float4* buf[2] = {guide + frame, guide + 2 * frame};
    const KajoGuidedFrame f = {map->W, map->H};
    const dim3 grid((map->W + 63) / 64, (map->H + 3) / 4), block(256);
    hipLaunchKernelGGL(kajo_denoise_prepare, grid, block, 0, s, static_cast<const float4*>(src), *map, fromTiles,
                       static_cast<const float4*>(albedoHits), static_cast<const float4*>(normalDepth), passes, samples, demodulate, guide, buf[0]);
    hipLaunchKernelGGL(kajo_denoise_guided_v0, grid, block, 0, s, buf[0], *map, static_cast<const GuidedRecord*>(records),
                       static_cast<const float*>(mean), static_cast<const float*>(stdError), buf[1]);
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
