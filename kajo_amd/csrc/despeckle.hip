// despeckle.hip -- repair of NaN / Inf pixels and clamp of fireflies over one whole frame, in front of the denoiser, the glare and the tone
// curves (kajo_hip_despeckle, kajo_hip_present_*; the definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3
// -ffp-contract=off, in every numerics build alike: the arithmetic is this file's own, so only its inputs depend on FAST / EXACT / STRICT.
//
// One lane per pixel, workgroups of 64x4 pixels, float4 per pixel. Passes, each a kernel on the caller's stream:
//   clamp    source frame F (tile buffers through TileMap, or a row-major frame) -> C (row-major): 9 float4 loads, the r-th largest of the
//            8 neighbours' luminances from a compare-exchange network in registers, one 16-byte store
//   repair   C -> out (row-major, or in the tile layout of the map, which the denoiser reads as it reads the accumulation): a pixel that
//            counts is copied; one that does not gathers 8 taps and, where none of them counts, 24 (rare: the divergence is confined to
//            the waves that hold such a pixel)
//   counts   the workgroups' counts of clamped and repaired pixels -> two 64-bit words
// A tap outside the image is read from the lane's own pixel and excluded (luminance -1, weight 0): the gathers have no divergent branch.
// Lanes outside the image work on the nearest pixel inside and store nothing. The counts come from a wave ballot, one word per wave
// through LDS and one per workgroup into a partials array with plain stores: no atomics, no order between workgroups, every sum in a
// fixed order. The source frame is only read.
#include <hip/hip_runtime.h>

#include <math.h>

#include "render_args.h"

namespace
{

__device__ inline size_t pixelSlot(const TileMap& map, int tiled, int x, int y)
{
    if (tiled) {
        int owner;
        uint32_t slot;
        kajoTileSlot(map, x, y, &owner, &slot);
        return (size_t)owner * map.slotsPerOwner + slot;
    }
    return (size_t)y * map.W + x;
}

// kajoTileSlot with its two axes apart, so that the nine taps of `clamp` share three divisions per axis: a column gives its tile column
// and its part of the slot, a row its tile row * tilesX and its part; the float4 index of a pixel is then that of its tile's first slot
// (owner * slotsPerOwner + (tile / tileCount) * the tile's slots) + both parts. Row-major frames: tile 0, the parts x and y * W.
struct Axis
{
    int tile;
    size_t part;
};

__device__ inline Axis columnOf(const TileMap& map, int tiled, int x)
{
    if (!tiled)
        return Axis{0, (size_t)x};
    const int tx = x / map.tileW, ix = x - tx * map.tileW;
    return Axis{tx, (size_t)((ix >> 3) * 64 + (ix & 7))};
}

__device__ inline Axis rowOf(const TileMap& map, int tiled, int y)
{
    if (!tiled)
        return Axis{0, (size_t)y * map.W};
    const int ty = y / map.tileH, iy = y - ty * map.tileH;
    return Axis{ty * map.tilesX, (size_t)((iy >> 3) * (map.tileW >> 3) * 64 + ((iy & 7) << 3))};
}

__device__ inline size_t pixelSlot(const TileMap& map, int tiled, Axis column, Axis row)
{
    size_t first = 0;
    if (tiled) {
        const int tile = column.tile + row.tile, tileSlots = (map.tileW >> 3) * (map.tileH >> 3) * 64;
        first = map.tileCount == 1 ? (size_t)tile * tileSlots
                                   : (size_t)(tile % map.tileCount) * map.slotsPerOwner + (size_t)(tile / map.tileCount) * tileSlots;
    }
    return first + column.part + row.part;
}

// m = F.rgb / P; true where the pixel counts (m finite in all three channels)
__device__ inline bool meanOf(float4 F, float passes, float3* m)
{
    *m = make_float3(F.x / passes, F.y / passes, F.z / passes);
    return isfinite(m->x) && isfinite(m->y) && isfinite(m->z);
}

__device__ inline float luminanceOf(float3 m)
{
    return 0.2126f * fmaxf(m.x, 0.0f) + 0.7152f * fmaxf(m.y, 0.0f) + 0.0722f * fmaxf(m.z, 0.0f);
}

// the larger of the two into a, the smaller into b (no NaN reaches the network: an excluded tap is -1)
__device__ inline void exchange(float& a, float& b)
{
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    a = hi;
    b = lo;
}

__device__ inline void sort4(float& a, float& b, float& c, float& d)
{
    exchange(a, b);
    exchange(c, d);
    exchange(a, c);
    exchange(b, d);
    exchange(b, c);
}

// The r-th largest (r = 1..4) of v[0..7]: both halves sorted, the top four of their merge picked by one bitonic half-cleaner
// (max(a_i, b_{3-i})) and sorted by the two stages a bitonic sequence of four needs. 18 compare-exchanges, all in registers.
__device__ inline float largest(float v[8], int r)
{
    sort4(v[0], v[1], v[2], v[3]);
    sort4(v[4], v[5], v[6], v[7]);
    float c0 = fmaxf(v[0], v[7]), c1 = fmaxf(v[1], v[6]), c2 = fmaxf(v[2], v[5]), c3 = fmaxf(v[3], v[4]);
    exchange(c0, c2);
    exchange(c1, c3);
    exchange(c0, c1);
    exchange(c2, c3);
    return r == 1 ? c0 : r == 2 ? c1 : r == 3 ? c2 : c3;
}

// the workgroup's number of lanes with `flag`, into partials[workgroup]: ballot per wave, the four waves' words summed in order by lane 0
__device__ inline void countInto(bool flag, uint32_t* partials)
{
    __shared__ uint32_t perWave[4];
    const uint32_t n = (uint32_t)__popcll(__ballot(flag));
    if ((threadIdx.x & 63) == 0)
        perWave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0)
        partials[blockIdx.y * gridDim.x + blockIdx.x] = ((perWave[0] + perWave[1]) + perWave[2]) + perWave[3];
}

} // namespace

// Step 1 of include/kajo_hip.h: F -> C, row-major
extern "C" __global__ void __launch_bounds__(256) kajo_despeckle_clamp(const float4* src, TileMap map, int fromTiles, float passes, float factor,
                                                                        int rank, float floorL, float4* clamped, uint32_t* partials)
{
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool inside = gx < map.W && gy < map.H;
    const int x = min(gx, map.W - 1), y = min(gy, map.H - 1);
    // (columns x - 1 .. x + 1 and rows y - 1 .. y + 1; one outside the image stands for the lane's own, and its taps are excluded below)
    Axis column[3], row[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int qx = x + i - 1, qy = y + i - 1;
        column[i] = columnOf(map, fromTiles, qx >= 0 && qx < map.W ? qx : x);
        row[i] = rowOf(map, fromTiles, qy >= 0 && qy < map.H ? qy : y);
    }
    const float4 F = src[pixelSlot(map, fromTiles, column[1], row[1])];
    float3 m;
    const bool counts = meanOf(F, passes, &m);
    const float l = luminanceOf(m);
    float v[8];
    int n = 0;
#pragma unroll
    for (int t = 0; t < 9; t++) {
        if (t == 4)
            continue;
        const int qx = x + t % 3 - 1, qy = y + t / 3 - 1;
        const bool in = qx >= 0 && qx < map.W && qy >= 0 && qy < map.H;
        float3 mq;
        const bool ok = meanOf(src[pixelSlot(map, fromTiles, column[in ? t % 3 : 1], row[in ? t / 3 : 1])], passes, &mq) && in;
        v[t < 4 ? t : t - 1] = ok ? luminanceOf(mq) : -1.0f;
        n += ok ? 1 : 0;
    }
    const float b = factor * fmaxf(largest(v, min(rank, n)), floorL);
    const bool clamp = counts && n >= 3 && l > b;
    float4 C = F;
    if (clamp) {
        const float s = b / l;
        C.x = (m.x * s) * passes;
        C.y = (m.y * s) * passes;
        C.z = (m.z * s) * passes;
    }
    if (inside)
        clamped[(size_t)y * map.W + x] = C;
    countInto(inside && clamp, partials);
}

// Step 2: C (the clamped frame, row-major; or with the clamp off the source itself) -> out
extern "C" __global__ void __launch_bounds__(256) kajo_despeckle_repair(const float4* src, TileMap map, int fromTiles, float passes, float4* out,
                                                                         int toTiles, uint32_t* partials)
{
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool inside = gx < map.W && gy < map.H;
    const int x = min(gx, map.W - 1), y = min(gy, map.H - 1);
    float4 C = src[pixelSlot(map, fromTiles, x, y)];
    float3 m;
    bool repaired = false;
    if (!meanOf(C, passes, &m)) {
        float3 sum = make_float3(0.0f, 0.0f, 0.0f);
        float n = 0.0f;
        for (int reach = 1; reach <= 2 && n == 0.0f; reach++)
            for (int dy = -reach; dy <= reach; dy++)
                for (int dx = -reach; dx <= reach; dx++) {
                    const int qx = x + dx, qy = y + dy;
                    const bool in = qx >= 0 && qx < map.W && qy >= 0 && qy < map.H && (dx != 0 || dy != 0);
                    float3 mq;
                    if (meanOf(src[pixelSlot(map, fromTiles, in ? qx : x, in ? qy : y)], passes, &mq) && in) {
                        sum.x += mq.x;
                        sum.y += mq.y;
                        sum.z += mq.z;
                        n += 1.0f;
                    }
                }
        if (n != 0.0f) {
            C.x = (sum.x / n) * passes;
            C.y = (sum.y / n) * passes;
            C.z = (sum.z / n) * passes;
            repaired = true;
        }
    }
    if (inside)
        out[pixelSlot(map, toTiles, x, y)] = C;
    countInto(inside && repaired, partials);
}

// counts[0] = the sum of clampPartials[0 .. groups) (0 where null), counts[1] = that of repairPartials: one workgroup, each lane a strided
// share, the 256 shares summed in lane order
extern "C" __global__ void __launch_bounds__(256) kajo_despeckle_counts(const uint32_t* clampPartials, const uint32_t* repairPartials, int groups,
                                                                         long long* counts)
{
    __shared__ long long share[2][256];
    long long a = 0, b = 0;
    for (int i = threadIdx.x; i < groups; i += 256) {
        a += clampPartials ? clampPartials[i] : 0u;
        b += repairPartials[i];
    }
    share[0][threadIdx.x] = a;
    share[1][threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x < 2) {
        long long total = 0;
        for (int i = 0; i < 256; i++)
            total += share[threadIdx.x][i];
        counts[threadIdx.x] = total;
    }
}

// workgroups of one pass over a W x H frame = the words of each of the two partials arrays
extern "C" int kajo_despeckle_groups(int W, int H)
{
    return ((W + 63) / 64) * ((H + 3) / 4);
}

// The stage on `stream`: src (tile buffers, or with fromTiles 0 a row-major frame) -> out (row-major, or with toTiles in the tile layout
// of *map, which must then have one owner; not the source). clamped: a row-major frame of scratch (not read with factor 0: the clamp is
// off and `repair` reads the source); partials: 2 * kajo_despeckle_groups words; counts: two 64-bit words (pixels clamped, repaired).
extern "C" int kajo_despeckle_launch(const void* src, const TileMap* map, int fromTiles, float passes, float factor, int rank, float floorL,
                                     void* clamped, void* out, int toTiles, void* partials, void* counts, void* stream)
{
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (map->W < 1 || map->H < 1 || (toTiles && map->tileCount != 1))
        return (int)hipErrorInvalidValue;
    const dim3 block(256), grid((map->W + 63) / 64, (map->H + 3) / 4);
    const int groups = kajo_despeckle_groups(map->W, map->H);
    uint32_t* clampPartials = static_cast<uint32_t*>(partials);
    uint32_t* repairPartials = clampPartials + groups;
    const float4* source = static_cast<const float4*>(src);
    if (factor != 0.0f) {
        hipLaunchKernelGGL(kajo_despeckle_clamp, grid, block, 0, st, source, *map, fromTiles, passes, factor, rank, floorL,
                           static_cast<float4*>(clamped), clampPartials);
        source = static_cast<const float4*>(clamped);
        fromTiles = 0;
    } else
        clampPartials = nullptr;
    hipLaunchKernelGGL(kajo_despeckle_repair, grid, block, 0, st, source, *map, fromTiles, passes, static_cast<float4*>(out), toTiles,
                       repairPartials);
    hipLaunchKernelGGL(kajo_despeckle_counts, dim3(1), block, 0, st, clampPartials, repairPartials, groups, static_cast<long long*>(counts));
    return (int)hipGetLastError();
}
