// grade.hip -- the grade of one whole frame, between the denoiser and the lens: white balance and an ASC CDL op over the frame, then up to
// four per-object regrades weighted by the coverage mattes (kajo_hip_grade, kajo_hip_present_grade_argb8 and its gathered twin; the
// definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, in every numerics build alike: the
// arithmetic is grade_math.h's, the host's own lines, so only the stage's inputs depend on FAST / EXACT / STRICT.
//
// One lane per pixel, workgroups of 64x4 pixels. A lane reads its source pixel (tile buffers through TileMap, or a row-major frame: one
// global_load_dwordx4), forms the mean, applies the ops and writes one global_store_dwordx4 into a row-major frame. Two instances:
//   kajo_grade_global   the global op alone: 32 bytes a pixel, no LDS
//   kajo_grade_regions  ... then the regions. The lane reads its pixel's coverage table once (64 bytes, as matte.hip's mask kernel) and
//                       forms every region's sum of selected counts in ONE walk of the eight slots. The regions' id bitsets (matte.hip's
//                       format: bit i of word i / 32, nObjects + 1 bits, region k's at k * words) are staged in LDS by the workgroup: the
//                       lookups are addressed by a slot's id, which differs from lane to lane, so the scalar cache could not serve them,
//                       while neighbouring pixels mostly see the same few objects and a ds_read_b32 at one address is a broadcast.
//                       It is a separate instance so that the global one does not carry the table's sixteen registers.
// The parameters (five ops, four amounts) are a block in device memory read at wave-uniform addresses through the scalar cache; power.c
// != 1, saturation != 1 and the region count are scalar branches, so a white-balance-only grade never enters the binary64 kajo_powf.
// A pixel that does not count (a channel of the mean not finite) is written as it was read. No atomics, no cross-lane work, no FLAT
// access, no scratch: a pixel depends on the inputs through image coordinates only. The source, the tables and the block are only read.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "grade_math.h"
#include "render_args.h"

namespace
{

constexpr int kMaxRegions = 4; // KAJO_GRADE_MAX_REGIONS

// the parameter block's head (capi.cpp gradePlan writes it); behind it the bitsets uint32 [kMaxRegions][words]
struct GradeOpArgs
{
    float slope[3], offset[3], power[3], saturation;
    float amount; // of a region; the global op's is not read
    float pad;
};
struct GradeBlock
{
    GradeOpArgs op[1 + kMaxRegions]; // the global op, then the regions'
};

typedef const __attribute__((address_space(4))) GradeBlock* BlockPtr; // constant address space: s_load

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

// the op of the block at a wave-uniform index, as values (scalar registers)
__device__ inline GradeOpArgs opOf(BlockPtr block, int k)
{
    GradeOpArgs o;
    for (int c = 0; c < 3; c++) {
        o.slope[c] = block->op[k].slope[c];
        o.offset[c] = block->op[k].offset[c];
        o.power[c] = block->op[k].power[c];
    }
    o.saturation = block->op[k].saturation;
    o.amount = block->op[k].amount;
    o.pad = 0.0f;
    return o;
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_grade_global(const float4* __restrict__ src, TileMap map, int fromTiles, float passes,
                                                                     const GradeBlock* __restrict__ blockGlobal, float4* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const BlockPtr block = (BlockPtr)(uintptr_t)blockGlobal;
    const float4 F = sourcePixel(src, map, fromTiles, x, y);
    const float m[3] = {F.x / passes, F.y / passes, F.z / passes};
    float4 o = F;
    if (kajo::gradeFinite(m[0]) && kajo::gradeFinite(m[1]) && kajo::gradeFinite(m[2])) {
        float c[3];
        kajo::gradeOp(opOf(block, 0), m, c);
        o = make_float4(c[0] * passes, c[1] * passes, c[2] * passes, F.w);
    }
    out[(size_t)y * map.W + x] = o;
}

extern "C" __global__ void __launch_bounds__(256) kajo_grade_regions(const float4* __restrict__ src, TileMap map, int fromTiles, float passes,
                                                                      const GradeBlock* __restrict__ blockGlobal, int nRegions,
                                                                      const uint4* __restrict__ ids, const uint4* __restrict__ counts,
                                                                      const uint32_t* __restrict__ selected, uint32_t words, uint32_t nObjects,
                                                                      float samples, float4* __restrict__ out)
{
    extern __shared__ uint32_t sBits[]; // [nRegions][words]
    for (uint32_t i = threadIdx.x; i < (uint32_t)nRegions * words; i += 256)
        sBits[i] = selected[i];
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const BlockPtr block = (BlockPtr)(uintptr_t)blockGlobal;
    const size_t at = (size_t)y * map.W + x;
    const float4 F = sourcePixel(src, map, fromTiles, x, y);
    const float m[3] = {F.x / passes, F.y / passes, F.z / passes};
    if (!(kajo::gradeFinite(m[0]) && kajo::gradeFinite(m[1]) && kajo::gradeFinite(m[2]))) {
        out[at] = F;
        return;
    }
    // every region's sum in one walk of the table
    const uint4 i0 = ids[2 * at], i1 = ids[2 * at + 1], c0 = counts[2 * at], c1 = counts[2 * at + 1];
    const uint32_t slotId[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
    const uint32_t slotCount[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    uint32_t sum0 = 0, sum1 = 0, sum2 = 0, sum3 = 0;
#pragma unroll
    for (int s = 0; s < 8; s++) {
        // (an empty slot adds its 0; the bound only keeps the read inside the bitset whatever the table holds, as matte.hip's)
        const uint32_t id = slotId[s] <= nObjects ? slotId[s] : 0u;
        const uint32_t word = id >> 5, bit = id & 31u;
        sum0 += ((sBits[word] >> bit) & 1u) ? slotCount[s] : 0u;
        if (nRegions > 1)
            sum1 += ((sBits[words + word] >> bit) & 1u) ? slotCount[s] : 0u;
        if (nRegions > 2)
            sum2 += ((sBits[2 * words + word] >> bit) & 1u) ? slotCount[s] : 0u;
        if (nRegions > 3)
            sum3 += ((sBits[3 * words + word] >> bit) & 1u) ? slotCount[s] : 0u;
    }
    float c[3];
    kajo::gradeOp(opOf(block, 0), m, c);
#pragma unroll 1
    for (int k = 0; k < nRegions; k++) {
        const uint32_t sum = k == 0 ? sum0 : k == 1 ? sum1 : k == 2 ? sum2 : sum3;
        const GradeOpArgs op = opOf(block, 1 + k);
        kajo::gradeRegion(op, op.amount, kajo::gradeMask(sum, samples), c);
    }
    out[at] = make_float4(c[0] * passes, c[1] * passes, c[2] * passes, F.w);
}

// bytes of the parameter block in front of the bitsets
extern "C" size_t kajo_grade_block_bytes(void)
{
    return sizeof(GradeBlock);
}

// The stage on `stream`: src (tile buffers, or with fromTiles 0 a row-major frame) -> out (row-major frame, not the source). block: the
// parameter block and, with regions, the bitsets behind it (device). nRegions == 0: ids, counts are not read.
extern "C" int kajo_grade_launch(const void* src, const TileMap* map, int fromTiles, float passes, const void* block, int nRegions, const void* ids,
                                 const void* counts, unsigned words, unsigned nObjects, float samples, void* out, void* stream)
{
    if (map->W < 1 || map->H < 1 || nRegions < 0 || nRegions > kMaxRegions)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((map->W + 63) / 64, (map->H + 3) / 4), threads(256);
    const GradeBlock* b = static_cast<const GradeBlock*>(block);
    if (nRegions == 0) {
        hipLaunchKernelGGL(kajo_grade_global, grid, threads, 0, st, static_cast<const float4*>(src), *map, fromTiles, passes, b,
                           static_cast<float4*>(out));
        return (int)hipGetLastError();
    }
    const size_t lds = (size_t)nRegions * words * sizeof(uint32_t);
    if (!ids || !counts || words < 1 || (size_t)nObjects + 1 > (size_t)words * 32 || lds > 64 * 1024)
        return (int)hipErrorInvalidValue;
    const uint32_t* selected = reinterpret_cast<const uint32_t*>(static_cast<const char*>(block) + sizeof(GradeBlock));
    hipLaunchKernelGGL(kajo_grade_regions, grid, threads, lds, st, static_cast<const float4*>(src), *map, fromTiles, passes, b, nRegions,
                       static_cast<const uint4*>(ids), static_cast<const uint4*>(counts), selected, (uint32_t)words, (uint32_t)nObjects, samples,
                       static_cast<float4*>(out));
    return (int)hipGetLastError();
}
