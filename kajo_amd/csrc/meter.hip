// meter.hip -- the luminance histogram of one whole frame, at the end of the display chain and in front of the tone curves (kajo_hip_meter,
// kajo_hip_present_metered_*; the definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, in every
// numerics build alike: the arithmetic is this file's own, so only its inputs depend on FAST / EXACT / STRICT.
//
// A scatter with integer counts, where every other stage is a stencil or a gather: integer addition commutes, so the counts are exact and
// the same words whatever the order of the adds, the number of workgroups or the number of tile owners. Two kernels on the caller's stream:
//   hist   source frame F (tile buffers through TileMap, or a row-major frame) -> one row of KAJO_METER_ROW words per workgroup. A capped
//          one-dimensional grid strides over the frame's 64x4 rectangles, four rectangles a trip (the four float4 loads of a lane are
//          issued before the first add). The workgroup's 514 counters live in LDS and are bumped with LDS integer adds; the pixels that
//          do not count are counted per wave with a ballot, in a register, and added to one more LDS word at the end. The row leaves
//          with plain stores: no global atomics, nothing to zero between calls.
//   sum    per column (514 bins, and the pixels that do not count beside them) eight threads add a strided share of the rows each, in
//          index order, and the first adds the eight shares in order -> the result. (One thread per column, as the despeckle sums its
//          counts, was measured first: 480 dependent round trips to L2, 66 us, five times the histogram kernel at 1920x1080.)
// Lanes outside the image work on the nearest pixel inside and count nothing. The source frame is only read.
#include <hip/hip_runtime.h>

#include <math.h>

#include "render_args.h"

#define KAJO_METER_BINS 514                   // include/kajo_hip.h
#define KAJO_METER_ROW (KAJO_METER_BINS + 1)  // a workgroup's row of the partials: the bins, then its pixels that do not count
#define KAJO_METER_MAX_GROUPS 480             // 480 rows of 515 words = 988,800 bytes: the partials stay under 1 MB at any frame size
#define KAJO_METER_UNROLL 4                   // rectangles a workgroup takes per trip

namespace
{

// the float4 index of pixel (x, y): kajoTileSlot with its two axes apart (a wave's row is one y), or the row-major index
__device__ inline size_t pixelSlot(const TileMap& map, int tiled, int x, int y)
{
    if (!tiled)
        return (size_t)y * map.W + x;
    const int tx = x / map.tileW, ix = x - tx * map.tileW;
    const int ty = y / map.tileH, iy = y - ty * map.tileH;
    const int tile = ty * map.tilesX + tx, tileSlots = (map.tileW >> 3) * (map.tileH >> 3) * 64;
    const size_t inTile = (size_t)(((iy >> 3) * (map.tileW >> 3) + (ix >> 3)) * 64 + (((iy & 7) << 3) | (ix & 7)));
    const size_t first = map.tileCount == 1 ? (size_t)tile * tileSlots
                                            : (size_t)(tile % map.tileCount) * map.slotsPerOwner + (size_t)(tile / map.tileCount) * tileSlots;
    return first + inTile;
}

// the bin of a pixel that counts (include/kajo_hip.h): by the bit pattern of its luminance, no logarithm
__device__ inline uint32_t binOf(float3 m)
{
    const float l = 0.2126f * fmaxf(m.x, 0.0f) + 0.7152f * fmaxf(m.y, 0.0f) + 0.0722f * fmaxf(m.z, 0.0f);
    const uint32_t k = (__float_as_uint(l) & 0x7fffffffu) >> 19, base = (127u - 16u) << 4;
    return k < base ? 0u : min(k - base + 1u, (uint32_t)(KAJO_METER_BINS - 1));
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_meter_hist(const float4* __restrict__ src, TileMap map, int fromTiles, float passes,
                                                                   int rects, uint32_t* __restrict__ partials)
{
    __shared__ uint32_t bins[KAJO_METER_ROW];
    for (int i = threadIdx.x; i < KAJO_METER_ROW; i += 256)
        bins[i] = 0u;
    __syncthreads();
    const int rectsX = (map.W + 63) / 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    uint32_t notCounting = 0; // (the wave's: the same in all its lanes)
    for (int first = blockIdx.x; first < rects; first += KAJO_METER_UNROLL * gridDim.x) {
        float4 F[KAJO_METER_UNROLL];
        bool inside[KAJO_METER_UNROLL];
#pragma unroll
        for (int j = 0; j < KAJO_METER_UNROLL; j++) {
            const int r = first + j * gridDim.x;
            const bool live = r < rects;
            const int rect = live ? r : first;
            const int by = rect / rectsX, bx = rect - by * rectsX;
            const int gx = bx * 64 + lx, gy = by * 4 + ly;
            inside[j] = live && gx < map.W && gy < map.H;
            F[j] = src[pixelSlot(map, fromTiles, min(gx, map.W - 1), min(gy, map.H - 1))];
        }
#pragma unroll
        for (int j = 0; j < KAJO_METER_UNROLL; j++) {
            const float3 m = make_float3(F[j].x / passes, F[j].y / passes, F[j].z / passes);
            const bool counts = isfinite(m.x) && isfinite(m.y) && isfinite(m.z);
            if (inside[j] && counts)
                atomicAdd(&bins[binOf(m)], 1u);
            notCounting += (uint32_t)__popcll(__ballot(inside[j] && !counts));
        }
    }
    if (lx == 0 && notCounting)
        atomicAdd(&bins[KAJO_METER_BINS], notCounting);
    __syncthreads();
    uint32_t* row = partials + (size_t)blockIdx.x * KAJO_METER_ROW;
    for (int i = threadIdx.x; i < KAJO_METER_ROW; i += 256)
        row[i] = bins[i];
}

// result[c] = the sum of column c over the rows 0 .. groups: c < 514 the bins, c = 514 the pixels that do not count. A workgroup takes
// KAJO_METER_SUM_COLUMNS columns, eight threads a column: thread s of a column adds the rows s, s + 8, ... and thread 0 the eight shares.
#define KAJO_METER_SUM_COLUMNS 32
extern "C" __global__ void __launch_bounds__(256) kajo_meter_sum(const uint32_t* __restrict__ partials, int groups, uint32_t* __restrict__ result)
{
    __shared__ uint32_t share[8][KAJO_METER_SUM_COLUMNS];
    const int column = threadIdx.x & (KAJO_METER_SUM_COLUMNS - 1), s = threadIdx.x / KAJO_METER_SUM_COLUMNS;
    const int c = blockIdx.x * KAJO_METER_SUM_COLUMNS + column;
    uint32_t total = 0;
    if (c < KAJO_METER_ROW) {
#pragma unroll 4
        for (int g = s; g < groups; g += 8)
            total += partials[(size_t)g * KAJO_METER_ROW + c];
    }
    share[s][column] = total;
    __syncthreads();
    if (s == 0 && c < KAJO_METER_ROW) {
#pragma unroll
        for (int i = 1; i < 8; i++)
            total += share[i][column];
        result[c] = total;
    }
}

// 64x4 rectangles of a W x H frame
static int meterRects(int W, int H)
{
    return ((W + 63) / 64) * ((H + 3) / 4);
}

// workgroups of `hist` over a W x H frame = the rows of the partials array: one per rectangle up to the cap, beyond which a workgroup
// takes further rectangles (a second trip once the frame has more than KAJO_METER_UNROLL times the cap)
extern "C" int kajo_meter_groups(int W, int H)
{
    const int rects = meterRects(W, H);
    return rects < KAJO_METER_MAX_GROUPS ? rects : KAJO_METER_MAX_GROUPS;
}

// The stage on `stream`: src (tile buffers, or with fromTiles 0 a row-major frame) -> result, KAJO_METER_ROW words (the 514 bins, then the
// pixels that do not count). partials: kajo_meter_groups rows of KAJO_METER_ROW words.
extern "C" int kajo_meter_launch(const void* src, const TileMap* map, int fromTiles, float passes, void* partials, void* result, void* stream)
{
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (map->W < 1 || map->H < 1)
        return (int)hipErrorInvalidValue;
    const int groups = kajo_meter_groups(map->W, map->H);
    hipLaunchKernelGGL(kajo_meter_hist, dim3(groups), dim3(256), 0, st, static_cast<const float4*>(src), *map, fromTiles, passes,
                       meterRects(map->W, map->H), static_cast<uint32_t*>(partials));
    hipLaunchKernelGGL(kajo_meter_sum, dim3((KAJO_METER_ROW + KAJO_METER_SUM_COLUMNS - 1) / KAJO_METER_SUM_COLUMNS), dim3(256), 0, st, static_cast<const uint32_t*>(partials), groups,
                       static_cast<uint32_t*>(result));
    return (int)hipGetLastError();
}
