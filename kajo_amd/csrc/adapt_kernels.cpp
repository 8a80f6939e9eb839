// adapt_kernels.cpp -- the device half of adaptive sampling (KAJO_FLAG_ADAPTIVE with KAJO_FLAG_NOISE; the definition is in
// include/kajo_hip.h "Adaptive sampling", the rule in adapt_math.h). HIP source: hipcc -x hip --offload-arch=gfx950 -O3 -ffp-contract=off,
// in every numerics build alike. Three kernels on the handle's stream, which the render, AOV and display kernels know nothing of:
//   step    behind every launch of a handle that has retired a unit: one lane per slot of the owner's tile buffer, in buffer order. A slot
//           of a retired unit becomes its baseline times P / (4 n) (16 + 16 bytes in, 16 out); a slot of an active unit, at a batch
//           boundary only, gets the noise estimate's update -- its expressions in its order (112 bytes). No atomics, no LDS, no
//           cross-lane operation: a slot is one lane's.
//   select  at a decision: a workgroup per unit, a wave per pixel block. Every lane evaluates its slot's relative error in binary64; a
//           ballot and a population count give the block's loud pixels; the unit's waves meet in LDS and one lane writes the state word.
//   passes  on request: the per-pixel pass count through the TileMap, a workgroup per 64x4 rectangle of the frame as the resolve has it.
#include <hip/hip_runtime.h>

#include <math.h>

#include "adapt_math.h"
#include "render_args.h"

#define KAJO_ADAPT_MAX_GROUPS 2048 // workgroups of step and passes; beyond it a workgroup strides

namespace
{

// a slot's moment record as its two 16-byte halves (include/kajo_hip.h KajoNoiseMoments)
struct AdaptRecord
{
    double2 s;    // s1, s2
    ulonglong2 c; // n, bad
};
static_assert(sizeof(AdaptRecord) == 32, "include/kajo_hip.h KajoNoiseMoments");

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_adapt_step(float4* __restrict__ tiles, float4* __restrict__ baseline,
                                                                   AdaptRecord* __restrict__ records, const uint32_t* __restrict__ state,
                                                                   uint32_t slots, uint32_t unitShift, int32_t boundary, int32_t P)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (size_t)gridDim.x * 256) {
        if (state[i >> unitShift] != KAJO_ADAPT_ACTIVE) {
            // retired: the uniform-equivalent sum of P passes from the slot's own 4 n (a slot without a batch of its own has nothing to extend)
            const ulonglong2 c = records[i].c;
            if (c.x) {
                const float4 B = baseline[i];
                const float f = kajo::adaptFactor(P, c.x);
                tiles[i] = make_float4(B.x * f, B.y * f, B.z * f, B.w * f);
            }
        } else if (boundary) {
            // active, a batch is complete: the estimate's update (noise.hip), expression by expression
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
}

extern "C" __global__ void __launch_bounds__(256) kajo_adapt_select(const AdaptRecord* __restrict__ records, uint32_t* __restrict__ state,
                                                                     AdaptGeom g, AdaptRule r)
{
    __shared__ uint32_t quiet[4];
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    const double2 s = records[slot].s;
    const ulonglong2 c = records[slot].c;
    int px, py;
    const bool loud = kajo::adaptSlotPixel(g, slot, &px, &py) && kajo::adaptLoud(s.x, s.y, c.x, r);
    const uint32_t nLoud = (uint32_t)__popcll(__ballot(loud));
    if ((threadIdx.x & 63u) == 0u)
        quiet[threadIdx.x >> 6] = nLoud <= r.allowance ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t waves = blockDim.x >> 6; // 1, 2 or 4
        uint32_t all = quiet[0];
        if (waves > 1u)
            all &= quiet[1];
        if (waves > 2u)
            all &= quiet[2] & quiet[3];
        if (all) // (a unit that is not quiet keeps its word: retirement is permanent)
            state[blockIdx.x] = KAJO_ADAPT_RETIRED;
    }
}

extern "C" __global__ void __launch_bounds__(256) kajo_adapt_passes(const AdaptRecord* __restrict__ records, const uint32_t* __restrict__ state,
                                                                     TileMap map, int tileIndex, int rects, uint32_t unitShift, uint32_t P,
                                                                     uint32_t* __restrict__ plane)
{
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
        uint32_t p = P;
        if (state[slot >> unitShift] != KAJO_ADAPT_ACTIVE)
            p = (uint32_t)min(4ull * records[slot].c.x, 0xffffffffull);
        plane[(size_t)y * map.W + x] = p;
    }
}

static unsigned adaptGroups(unsigned long long jobs)
{
    return (unsigned)(jobs < KAJO_ADAPT_MAX_GROUPS ? (jobs ? jobs : 1) : KAJO_ADAPT_MAX_GROUPS);
}

// Behind a launch that brought the handle to P passes: the first `slots` slots of the owner's tile buffer, units of 1 << unitShift slots.
extern "C" int kajo_adapt_step_launch(void* tiles, void* baseline, void* records, const void* state, uint32_t slots, uint32_t unitShift,
                                      int boundary, int P, void* stream)
{
    if (!slots)
        return (int)hipSuccess;
    hipLaunchKernelGGL(kajo_adapt_step, dim3(adaptGroups(((unsigned long long)slots + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<float4*>(tiles), static_cast<float4*>(baseline), static_cast<AdaptRecord*>(records),
                       static_cast<const uint32_t*>(state), slots, unitShift, (int32_t)boundary, (int32_t)P);
    return (int)hipGetLastError();
}

// A decision over `units` units of unitThreads = 64, 128 or 256 slots each: the records hold units * unitThreads slots at least.
extern "C" int kajo_adapt_select_launch(const void* records, void* state, const AdaptGeom* geom, const AdaptRule* rule, uint32_t units,
                                        uint32_t unitThreads, void* stream)
{
    if (!units)
        return (int)hipSuccess;
    if (unitThreads != 64 && unitThreads != 128 && unitThreads != 256)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kajo_adapt_select, dim3(units), dim3(unitThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdaptRecord*>(records), static_cast<uint32_t*>(state), *geom, *rule);
    return (int)hipGetLastError();
}

// The pass plane (W * H words) of owner `tileIndex` of a handle at P passes.
extern "C" int kajo_adapt_passes_launch(const void* records, const void* state, const TileMap* map, int tileIndex, uint32_t unitShift, uint32_t P,
                                        void* plane, void* stream)
{
    if (map->W < 1 || map->H < 1)
        return (int)hipErrorInvalidValue;
    const int rects = ((map->W + 63) / 64) * ((map->H + 3) / 4);
    hipLaunchKernelGGL(kajo_adapt_passes, dim3(adaptGroups((unsigned long long)rects)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdaptRecord*>(records), static_cast<const uint32_t*>(state), *map, tileIndex, rects, unitShift, P,
                       static_cast<uint32_t*>(plane));
    return (int)hipGetLastError();
}
