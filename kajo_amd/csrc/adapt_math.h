// adapt_math.h -- the rule of adaptive sampling (include/kajo_hip.h "Adaptive sampling"), host and device: when a pixel is loud, where a
// slot of the tile buffer lies in the image, and the factor a retired slot's baseline is extended by. adapt_kernels.cpp's kernels and
// capi.cpp's kajo_hip_adapt_evaluate are compiled from these same lines, as grade.hip's and kajo_hip_grade_pixels are from grade_math.h:
// what a test reads from the host is what the device decides. binary64 / float32 IEEE, no contraction (the pragma below on the host;
// -ffp-contract=off for the device), in the order written. Pure functions, no state. The filter of the launch order is host only.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KAM_FN __host__ __device__ static inline
#else
#define KAM_FN static inline
#pragma STDC FP_CONTRACT OFF
#endif

// a unit's state word
#define KAJO_ADAPT_ACTIVE 0u
#define KAJO_ADAPT_RETIRED 1u

// where the slots of an owner's tile buffer lie: the fields of RenderArgs the render kernel forms a slot's pixel from
struct AdaptGeom
{
    int32_t W, H, tileW, tileH, tilesX, tileIndex, tileCount, nTilesOwned;
};

// the decision's numbers (KajoAdaptParams, checked by capi.cpp)
struct AdaptRule
{
    float target, floorL;
    uint32_t allowance;
};

namespace kajo
{

// The pixel of a slot, by the render kernel's own arithmetic (integrator.inc.hip: wave -> owned tile -> tile -> 8x8 block -> lane)
KAM_FN bool adaptSlotPixel(const AdaptGeom& g, uint32_t slot, int* px, int* py)
{
    const int lane = (int)(slot & 63u);
    const int wave = (int)(slot >> 6);
    const int wavesPerTile = (g.tileW >> 3) * (g.tileH >> 3);
    const int ownedTile = wave / wavesPerTile;
    const int wb = wave - ownedTile * wavesPerTile;
    const int tile = g.tileIndex + ownedTile * g.tileCount;
    const int tx = tile % g.tilesX, ty = tile / g.tilesX;
    const int bxi = wb % (g.tileW >> 3), byi = wb / (g.tileW >> 3);
    *px = tx * g.tileW + bxi * 8 + (lane & 7);
    *py = ty * g.tileH + byi * 8 + (lane >> 3);
    return ownedTile < g.nTilesOwned && *px < g.W && *py < g.H;
}

// The relative error of a record: the estimate's evaluation in binary64, rounded to float32 as its map has it; -1 with fewer than two batches
KAM_FN float adaptRel(double s1, double s2, uint64_t count, float floorL)
{
    if (count < 2ull)
        return -1.0f;
    const double n = (double)count;
    const double md = s1 / (4.0 * n);
    const double v = fmax(s2 - s1 * s1 / n, 0.0) / (n - 1.0);
    const double e = sqrt(v / n) / 4.0;
    return (float)(e / (fmax(md, 0.0) + (double)floorL));
}

// A pixel is loud while its error is unknown or above the target; a record's `bad` does not count
KAM_FN bool adaptLoud(double s1, double s2, uint64_t count, const AdaptRule& r)
{
    return count < 2ull || adaptRel(s1, s2, count, r.floorL) > r.target;
}

// What a retired slot's baseline is multiplied by for a frame of P passes: the slot has 4 n of its own
KAM_FN float adaptFactor(int32_t P, uint64_t count)
{
    return (float)((double)P / (double)(4ull * count));
}

} // namespace kajo

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

// The launch order of an adaptive handle: `order` (n units, the most expensive first; NULL: image order) with the retired units
// (state[u] != 0) taken out; for the SPLIT kernels, whose workgroup is a pixel block, the active units' pixel blocks instead.
inline void kajoAdaptOrder(const uint32_t* order, size_t n, const uint32_t* state, unsigned wavesPerBlock, bool split, std::vector<uint32_t>& out)
{
    out.clear();
    for (size_t i = 0; i < n; i++) {
        const uint32_t u = order ? order[i] : (uint32_t)i;
        if (state[u] != KAJO_ADAPT_ACTIVE)
            continue;
        if (!split)
            out.push_back(u);
        else
            for (unsigned k = 0; k < wavesPerBlock; k++)
                out.push_back(u * wavesPerBlock + k);
    }
}
#endif
