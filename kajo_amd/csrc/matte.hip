// matte.hip -- readers of the per-pixel object-coverage tables the _matte AOV instances keep (KAJO_FLAG_AOV_MATTE; aov.inc.hip;
// kajo_hip_read_matte, kajo_hip_matte_mask; the definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3
// -ffp-contract=off, in every numerics build alike: the tables are integers, and the one float operation per pixel is this file's own.
//
// A table is two uint4 of ids and two uint4 of counts per pixel, row-major: eight slots (id, count), count 0 = empty, the filled slots
// a prefix. One lane per pixel, workgroups of 64x4 pixels dealt row by row from a one-dimensional grid (a frame of any shape create()
// accepts). Each kernel on the caller's stream:
//   rank      table -> the eight slots in order: count descending, ties by id ascending, empty slots last and written as (-1, 0). A
//             fixed network of 19 compare-exchanges (Batcher's odd-even merge sort of eight) on named registers.
//   mask      table + a bitset of selected ids (bit i of word i / 32, nObjects + 1 bits) -> float32(sum of the selected slots' counts) /
//             samples, one division per pixel; 0 with no sample
//   dominant  table -> the id rank would put first, as float32 (-1 where the table is empty)
// The tables are only read. No atomics, no LDS, nothing spilled: lanes outside the frame leave at once (there is no barrier).
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace
{

struct Slot
{
    uint32_t count, id;
};

// a goes in front of b: the larger count, then the smaller id
__device__ inline bool before(Slot a, Slot b)
{
    return a.count > b.count || (a.count == b.count && a.id < b.id);
}

__device__ inline void exchange(Slot& a, Slot& b)
{
    const bool swap = before(b, a);
    const Slot first = swap ? b : a, second = swap ? a : b;
    a = first;
    b = second;
}

__device__ inline void sort4(Slot& a, Slot& b, Slot& c, Slot& d)
{
    exchange(a, b);
    exchange(c, d);
    exchange(a, c);
    exchange(b, d);
    exchange(b, c);
}

// the lane's pixel, or false for a lane outside the frame
__device__ inline bool pixelOf(int W, int H, size_t* at)
{
    const int groupsX = (W + 63) >> 6;
    const int gx = (int)(blockIdx.x % (unsigned)groupsX) * 64 + (int)(threadIdx.x & 63);
    const long long gy = (long long)(blockIdx.x / (unsigned)groupsX) * 4 + (threadIdx.x >> 6);
    *at = (size_t)gy * W + gx;
    return gx < W && gy < H;
}

__device__ inline void loadTable(const uint4* ids, const uint4* counts, size_t at, Slot s[8])
{
    const uint4 i0 = ids[2 * at], i1 = ids[2 * at + 1], c0 = counts[2 * at], c1 = counts[2 * at + 1];
    s[0] = Slot{c0.x, i0.x};
    s[1] = Slot{c0.y, i0.y};
    s[2] = Slot{c0.z, i0.z};
    s[3] = Slot{c0.w, i0.w};
    s[4] = Slot{c1.x, i1.x};
    s[5] = Slot{c1.y, i1.y};
    s[6] = Slot{c1.z, i1.z};
    s[7] = Slot{c1.w, i1.w};
}

__device__ inline int32_t idOrNone(Slot s)
{
    return s.count ? (int32_t)s.id : -1;
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_matte_rank(const uint4* ids, const uint4* counts, int W, int H, int4* rankedIds,
                                                                   uint4* rankedCounts)
{
    size_t at;
    if (!pixelOf(W, H, &at))
        return;
    Slot s[8];
    loadTable(ids, counts, at, s);
    sort4(s[0], s[1], s[2], s[3]);
    sort4(s[4], s[5], s[6], s[7]);
    exchange(s[0], s[4]);
    exchange(s[1], s[5]);
    exchange(s[2], s[6]);
    exchange(s[3], s[7]);
    exchange(s[2], s[4]);
    exchange(s[3], s[5]);
    exchange(s[1], s[2]);
    exchange(s[3], s[4]);
    exchange(s[5], s[6]);
    rankedIds[2 * at] = make_int4(idOrNone(s[0]), idOrNone(s[1]), idOrNone(s[2]), idOrNone(s[3]));
    rankedIds[2 * at + 1] = make_int4(idOrNone(s[4]), idOrNone(s[5]), idOrNone(s[6]), idOrNone(s[7]));
    rankedCounts[2 * at] = make_uint4(s[0].count, s[1].count, s[2].count, s[3].count);
    rankedCounts[2 * at + 1] = make_uint4(s[4].count, s[5].count, s[6].count, s[7].count);
}

extern "C" __global__ void __launch_bounds__(256) kajo_matte_mask(const uint4* ids, const uint4* counts, int W, int H, const uint32_t* selected,
                                                                   uint32_t nObjects, float samples, float* mask)
{
    size_t at;
    if (!pixelOf(W, H, &at))
        return;
    Slot s[8];
    loadTable(ids, counts, at, s);
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        // (an empty slot adds its 0; an id is a hit of this scene's walk, the bound only keeps the read inside the bitset whatever the table holds)
        const uint32_t id = s[k].id <= nObjects ? s[k].id : 0u;
        sum += ((selected[id >> 5] >> (id & 31u)) & 1u) ? s[k].count : 0u;
    }
    mask[at] = samples > 0.0f ? (float)sum / samples : 0.0f;
}

extern "C" __global__ void __launch_bounds__(256) kajo_matte_dominant(const uint4* ids, const uint4* counts, int W, int H, float* dominant)
{
    size_t at;
    if (!pixelOf(W, H, &at))
        return;
    Slot s[8];
    loadTable(ids, counts, at, s);
    Slot best = s[0];
#pragma unroll
    for (int k = 1; k < 8; k++)
        best = before(s[k], best) ? s[k] : best;
    dominant[at] = (float)idOrNone(best);
}

namespace
{
unsigned groupsOf(int W, int H)
{
    return (unsigned)(((long long)(W + 63) / 64) * (((long long)H + 3) / 4));
}
} // namespace

// ids, counts: the tables (device). rankedIds: int32 [W * H][8], rankedCounts: uint32 [W * H][8] (device).
extern "C" int kajo_matte_rank_launch(const void* ids, const void* counts, int W, int H, void* rankedIds, void* rankedCounts, void* stream)
{
    if (W < 1 || H < 1)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kajo_matte_rank, dim3(groupsOf(W, H)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint4*>(ids),
                       static_cast<const uint4*>(counts), W, H, static_cast<int4*>(rankedIds), static_cast<uint4*>(rankedCounts));
    return (int)hipGetLastError();
}

// selected: the bitset, (nObjects + 1 + 31) / 32 words (device); mask, dominant: float [W * H] (device), either may be null
extern "C" int kajo_matte_mask_launch(const void* ids, const void* counts, int W, int H, const void* selected, unsigned nObjects, float samples,
                                      void* mask, void* dominant, void* stream)
{
    if (W < 1 || H < 1)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(groupsOf(W, H)), block(256);
    if (mask)
        hipLaunchKernelGGL(kajo_matte_mask, grid, block, 0, st, static_cast<const uint4*>(ids), static_cast<const uint4*>(counts), W, H,
                           static_cast<const uint32_t*>(selected), (uint32_t)nObjects, samples, static_cast<float*>(mask));
    if (dominant)
        hipLaunchKernelGGL(kajo_matte_dominant, grid, block, 0, st, static_cast<const uint4*>(ids), static_cast<const uint4*>(counts), W, H,
                           static_cast<float*>(dominant));
    return (int)hipGetLastError();
}
