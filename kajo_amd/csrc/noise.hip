// noise.hip -- the per-pixel noise estimate of KAJO_FLAG_NOISE: batch means beside the render (kajo_hip_noise, kajo_hip_read_noise_moments;
// the definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, in every numerics build alike: the
// arithmetic is this file's own, so only its input -- the accumulation -- depends on FAST / EXACT / STRICT.
//
// Two kernels on the handle's stream, neither of which the render, AOV or display kernels know of:
//   update  behind the launch that completes a batch of KAJO_NOISE_BATCH_PASSES passes: one lane per slot of the owner's tile buffer, in
//           buffer order. T (16 bytes) and the baseline (16 bytes) in, the moment record (32 bytes: s1, s2 binary64, n, bad 64-bit counts)
//           in and out, T out as the new baseline: 112 bytes a slot. No atomics, no LDS, no cross-lane operation: a slot is one lane's.
//   map     on request: the records through the TileMap, a workgroup per 64x4 rectangle of the frame as the resolve has it -> the row-major
//           planes m, se, rel (float) and n (uint32), written for the owner's pixels only, and the histogram of rel under the meter's
//           bit-pattern rule: 516 counters in LDS, flushed with integer atomics (integer addition commutes: the same words whatever the
//           order, the number of workgroups or of owners). The caller zeroes the histogram in front of the launch.
#include <hip/hip_runtime.h>

#include <math.h>

#include "render_args.h"

#define KAJO_NOISE_BINS 514                      // include/kajo_hip.h KAJO_METER_BINS
#define KAJO_NOISE_WORDS (KAJO_NOISE_BINS + 2)   // include/kajo_hip.h KAJO_NOISE_HIST_WORDS: the bins, the unknown pixels, the pixels with bad > 0
#define KAJO_NOISE_MAX_GROUPS 2048               // workgroups of either kernel; beyond it a workgroup strides

namespace
{

// a slot's moment record as its two 16-byte halves
struct NoiseRecord
{
    double2 s;             // s1, s2
    ulonglong2 c;          // n, bad
};
static_assert(sizeof(NoiseRecord) == 32, "include/kajo_hip.h KajoNoiseMoments");

// the meter's bin of a non-negative float (include/kajo_hip.h): by its bit pattern, no logarithm
__device__ inline uint32_t binOf(float rel)
{
    const uint32_t k = (__float_as_uint(rel) & 0x7fffffffu) >> 19, base = (127u - 16u) << 4;
    return k < base ? 0u : min(k - base + 1u, (uint32_t)(KAJO_NOISE_BINS - 1));
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_noise_update(const float4* __restrict__ tiles, float4* __restrict__ baseline,
                                                                     NoiseRecord* __restrict__ records, uint32_t slots)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (size_t)gridDim.x * 256) {
        const float4 T = tiles[i];
        const float4 B = baseline[i];
        double2 s = records[i].s;
        ulonglong2 c = records[i].c;
        const float dx = T.x - B.x, dy = T.y - B.y, dz = T.z - B.z;
        const float y = 0.2126f * dx + 0.7152f * dy + 0.0722f * dz;
        if (isfinite(y)) {
            const double d = (double)y;
            c.x += 1ull;
            s.x += d;
            s.y += d * d;
        } else
            c.y += 1ull;
        records[i].s = s;
        records[i].c = c;
        baseline[i] = T;
    }
}

extern "C" __global__ void __launch_bounds__(256) kajo_noise_map(const NoiseRecord* __restrict__ records, TileMap map, int tileIndex, int rects,
                                                                  double floorL, float* __restrict__ mean, float* __restrict__ stdError,
                                                                  float* __restrict__ relative, uint32_t* __restrict__ batches,
                                                                  uint32_t* __restrict__ hist)
{
    __shared__ uint32_t bins[KAJO_NOISE_WORDS];
    for (int i = threadIdx.x; i < KAJO_NOISE_WORDS; i += 256)
        bins[i] = 0u;
    __syncthreads();
    const int rectsX = (map.W + 63) / 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int rect = blockIdx.x; rect < rects; rect += gridDim.x) {
        const int by = rect / rectsX, bx = rect - by * rectsX;
        const int x = bx * 64 + lx, y = by * 4 + ly;
        if (x >= map.W || y >= map.H)
            continue;
        int owner;
        uint32_t slot;
        kajoTileSlot(map, x, y, &owner, &slot);
        if (owner != tileIndex)
            continue;
        const double2 s = records[slot].s;
        const ulonglong2 c = records[slot].c;
        const double n = (double)c.x;
        const double md = c.x > 0ull ? s.x / (4.0 * n) : 0.0;
        const float m = (float)md;
        float se = -1.0f, rel = -1.0f;
        if (c.x >= 2ull) {
            const double v = fmax(s.y - s.x * s.x / n, 0.0) / (n - 1.0);
            const double e = sqrt(v / n) / 4.0;
            se = (float)e;
            rel = (float)(e / (fmax(md, 0.0) + floorL));
            atomicAdd(&bins[binOf(rel)], 1u);
        } else
            atomicAdd(&bins[KAJO_NOISE_BINS], 1u);
        if (c.y > 0ull)
            atomicAdd(&bins[KAJO_NOISE_BINS + 1], 1u);
        const size_t at = (size_t)y * map.W + x;
        mean[at] = m;
        stdError[at] = se;
        relative[at] = rel;
        batches[at] = (uint32_t)min(c.x, 0xffffffffull);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KAJO_NOISE_WORDS; i += 256)
        if (bins[i])
            atomicAdd(&hist[i], bins[i]);
}

static unsigned noiseGroups(unsigned long long jobs)
{
    return (unsigned)(jobs < KAJO_NOISE_MAX_GROUPS ? (jobs ? jobs : 1) : KAJO_NOISE_MAX_GROUPS);
}

// A batch is complete: the moments of the first `slots` slots of the owner's tile buffer take it in, the baseline becomes the buffer.
extern "C" int kajo_noise_update_launch(const void* tiles, void* baseline, void* records, uint32_t slots, void* stream)
{
    if (!slots)
        return (int)hipSuccess;
    hipLaunchKernelGGL(kajo_noise_update, dim3(noiseGroups(((unsigned long long)slots + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float4*>(tiles), static_cast<float4*>(baseline), static_cast<NoiseRecord*>(records), slots);
    return (int)hipGetLastError();
}

// The planes (W * H words each) and the histogram (KAJO_NOISE_WORDS words, zeroed by the caller on the same stream) of owner `tileIndex`.
extern "C" int kajo_noise_map_launch(const void* records, const TileMap* map, int tileIndex, double floorL, void* mean, void* stdError,
                                     void* relative, void* batches, void* hist, void* stream)
{
    if (map->W < 1 || map->H < 1)
        return (int)hipErrorInvalidValue;
    const int rects = ((map->W + 63) / 64) * ((map->H + 3) / 4);
    hipLaunchKernelGGL(kajo_noise_map, dim3(noiseGroups((unsigned long long)rects)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const NoiseRecord*>(records), *map, tileIndex, rects, floorL, static_cast<float*>(mean),
                       static_cast<float*>(stdError), static_cast<float*>(relative), static_cast<uint32_t*>(batches),
                       static_cast<uint32_t*>(hist));
    return (int)hipGetLastError();
}
