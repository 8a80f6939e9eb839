// checkpoint_kernels.cpp -- the kernels of checkpoints (include/kajo_hip.h "Checkpoints"; checkpoint.cpp drives them): a plane of the handle's state
// between its own layout and the canonical order -- the owner's in-image pixels, y ascending then x (checkpoint_math.h) -- and a plane's
// digest. Compiled once, for every numerics build: integer copies and integer sums, nothing of the numerics.
//   pack     one lane per owned pixel, by its index r in canonical order: the pixel's record, `parts` pieces of `vecs` 16-byte vectors from
//            `parts` consecutive arrays of `elems` pieces -- a tile-layout array (the piece at kajoTileSlot's slot) or a row-major whole
//            frame -- to record r of the staging buffer
//   unpack   one lane per piece of the destination arrays: the record of the pixel it belongs to, or zero where it belongs to none (padding,
//            a slot outside the image): the restored buffer is defined everywhere
//   digest   the sum modulo 2^64 of the terms of a staged plane's words: per lane, then per wave by lane shuffles, per workgroup through LDS,
//            one partial sum per workgroup; digest_sum, one workgroup, adds the partial sums. No atomics; plain vector stores.
#include <hip/hip_runtime.h>

#include "checkpoint_math.h"

namespace
{

__device__ inline TileMap mapOf(const KajoCkptGeom& g)
{
    TileMap m;
    m.W = g.W;
    m.H = g.H;
    m.tileW = g.tileW;
    m.tileH = g.tileH;
    m.tilesX = g.tilesX;
    m.tileCount = g.tileCount;
    m.slotsPerOwner = 0;
    return m;
}

constexpr unsigned kThreads = 256;

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_ckpt_pack(const uint4* __restrict__ src, KajoCkptGeom g, const uint32_t* __restrict__ prefix,
                                                                 uint32_t pixels, uint32_t parts, uint32_t vecs, uint32_t elems, int tiled,
                                                                 uint4* __restrict__ dst)
{
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= pixels)
        return;
    int x, y;
    kajoCkptPixel(g, prefix, r, &x, &y);
    uint32_t e = (uint32_t)y * (uint32_t)g.W + (uint32_t)x;
    if (tiled) {
        int owner;
        kajoTileSlot(mapOf(g), x, y, &owner, &e);
    }
    for (uint32_t k = 0; k < parts; k++)
        for (uint32_t v = 0; v < vecs; v++)
            dst[((size_t)r * parts + k) * vecs + v] = src[((size_t)k * elems + e) * vecs + v];
}

extern "C" __global__ void __launch_bounds__(256) kajo_ckpt_unpack(const uint4* __restrict__ src, KajoCkptGeom g, const uint32_t* __restrict__ prefix,
                                                                   uint32_t parts, uint32_t vecs, uint32_t elems, int tiled, uint4* __restrict__ dst)
{
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= elems)
        return;
    int x, y;
    bool inside;
    if (tiled) {
        inside = kajoCkptSlotPixel(g, e, &x, &y);
    } else {
        y = (int)(e / (uint32_t)g.W);
        x = (int)(e - (uint32_t)y * (uint32_t)g.W);
        inside = y < g.H && kajoCkptOwns(g, x, y);
    }
    const uint32_t r = inside ? kajoCkptRank(g, prefix, x, y) : 0u;
    for (uint32_t k = 0; k < parts; k++)
        for (uint32_t v = 0; v < vecs; v++)
            dst[((size_t)k * elems + e) * vecs + v] = inside ? src[((size_t)r * parts + k) * vecs + v] : make_uint4(0u, 0u, 0u, 0u);
}

// staged: `pixels` records of 4 * vecs words in canonical order; partial[blockIdx.x]: the sum of the terms this workgroup's lanes met
extern "C" __global__ void __launch_bounds__(256) kajo_ckpt_digest(const uint4* __restrict__ staged, KajoCkptGeom g, const uint32_t* __restrict__ prefix,
                                                                   uint32_t pixels, uint32_t vecs, unsigned long long* __restrict__ partial)
{
    __shared__ unsigned long long waves[kThreads / 64];
    const uint32_t w = vecs * 4u;
    unsigned long long sum = 0;
    for (unsigned long long r = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; r < pixels; r += (unsigned long long)gridDim.x * kThreads) {
        int x, y;
        kajoCkptPixel(g, prefix, (uint32_t)r, &x, &y);
        const uint64_t p = (uint64_t)y * (uint32_t)g.W + (uint32_t)x;
        for (uint32_t v = 0; v < vecs; v++) {
            const uint4 q = staged[r * vecs + v];
            sum += kajoCkptTerm(p, w, 4u * v, q.x);
            sum += kajoCkptTerm(p, w, 4u * v + 1u, q.y);
            sum += kajoCkptTerm(p, w, 4u * v + 2u, q.z);
            sum += kajoCkptTerm(p, w, 4u * v + 3u, q.w);
        }
    }
    for (int offset = 32; offset > 0; offset >>= 1)
        sum += __shfl_down(sum, offset, 64);
    if ((threadIdx.x & 63u) == 0)
        waves[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (unsigned i = 0; i < kThreads / 64; i++)
            total += waves[i];
        partial[blockIdx.x] = total;
    }
}

extern "C" __global__ void __launch_bounds__(256) kajo_ckpt_digest_sum(const unsigned long long* __restrict__ partial, uint32_t n,
                                                                       unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long waves[kThreads / 64];
    unsigned long long sum = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kThreads)
        sum += partial[i];
    for (int offset = 32; offset > 0; offset >>= 1)
        sum += __shfl_down(sum, offset, 64);
    if ((threadIdx.x & 63u) == 0)
        waves[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (unsigned i = 0; i < kThreads / 64; i++)
            total += waves[i];
        *out = total;
    }
}

// ---- launchers (handle.h) ------------------------------------------------------------------------------------------------------------

extern "C" int kajo_ckpt_pack_launch(const void* src, const KajoCkptGeom* g, const void* prefix, uint32_t pixels, uint32_t parts, uint32_t vecs,
                                     uint32_t elems, int tiled, void* staged, void* stream)
{
    if (pixels == 0)
        return (int)hipSuccess;
    hipLaunchKernelGGL(kajo_ckpt_pack, dim3((pixels + kThreads - 1) / kThreads), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint4*>(src), *g, static_cast<const uint32_t*>(prefix), pixels, parts, vecs, elems, tiled,
                       static_cast<uint4*>(staged));
    return (int)hipGetLastError();
}

extern "C" int kajo_ckpt_unpack_launch(const void* staged, const KajoCkptGeom* g, const void* prefix, uint32_t parts, uint32_t vecs, uint32_t elems,
                                       int tiled, void* dst, void* stream)
{
    if (elems == 0)
        return (int)hipSuccess;
    hipLaunchKernelGGL(kajo_ckpt_unpack, dim3((elems + kThreads - 1) / kThreads), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint4*>(staged), *g, static_cast<const uint32_t*>(prefix), parts, vecs, elems, tiled,
                       static_cast<uint4*>(dst));
    return (int)hipGetLastError();
}

// workgroups of the digest of `pixels` records: its partial sums (at most KAJO_CKPT_DIGEST_GROUPS of them)
extern "C" unsigned kajo_ckpt_digest_groups(uint32_t pixels)
{
    const unsigned groups = (pixels + kThreads - 1) / kThreads;
    return groups < 1u ? 1u : groups > 1024u ? 1024u : groups;
}

extern "C" int kajo_ckpt_digest_launch(const void* staged, const KajoCkptGeom* g, const void* prefix, uint32_t pixels, uint32_t vecs, void* partials,
                                       void* out, void* stream)
{
    const unsigned groups = kajo_ckpt_digest_groups(pixels);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kajo_ckpt_digest, dim3(groups), dim3(kThreads), 0, s, static_cast<const uint4*>(staged), *g,
                       static_cast<const uint32_t*>(prefix), pixels, vecs, static_cast<unsigned long long*>(partials));
    hipLaunchKernelGGL(kajo_ckpt_digest_sum, dim3(1), dim3(kThreads), 0, s, static_cast<const unsigned long long*>(partials), groups,
                       static_cast<unsigned long long*>(out));
    return (int)hipGetLastError();
}
