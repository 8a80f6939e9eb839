// encode.cpp -- the encode of one whole frame, in place of the tone kernels' 8-bit word: exposure and tone curve, a transfer function from
// a table, optional dither, and one 10/16-bit, half-float or 8-bit word per pixel (kajo_hip_encode, kajo_hip_encode_present and its
// gathered twin; the definition is in include/kajo_hip.h "The encode"). HIP source in a .cpp file, as adapt_kernels.cpp. Build: hipcc
// -x hip --offload-arch=gfx950 -O3 -ffp-contract=off, once, in every numerics build alike: the arithmetic is encode_math.h's, the host's
// own lines, so only the stage's input depends on FAST / EXACT / STRICT. The device evaluates no pow, exp or log.
//
// One kernel, kajo_encode, workgroups of 256 lanes. A workgroup first copies the transfer's table (encode_math.h: 8194 floats, 32776
// bytes; not for LINEAR, which reads none) into LDS with 8-byte loads, then walks 64x4-pixel blocks of the frame blockIdx.x, + gridDim.x,
// ...: the launch has at most kMaxGroups workgroups, so a 1920x1080 frame pays the 32 KiB of staging once per eight blocks and not once
// per 256 pixels. The lookups are addressed by a pixel's value, which differs from lane to lane: LDS serves them at one ds_read_b64
// (T_i, S_i) and one ds_read_b32 (the cap T_i+1) per channel. A lane reads its pixel (tile buffers through TileMap, or a row-major
// frame: one global_load_dwordx4) and writes one global_store_dword or, for the 8-byte formats, one global_store_dwordx2. The format,
// transfer, curve and flags are kernel arguments: every branch on them is scalar. No atomics, no cross-lane work, no scratch; a pixel
// depends on the inputs through its frame coordinates only, so the image is the same for any number of tile owners. LDS: 32776 bytes.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "encode_math.h"
#include "render_args.h"

namespace
{

constexpr unsigned kMaxGroups = 1024; // four workgroups for each of 256 compute units: 4 x 32 KiB of LDS a unit

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

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_encode(const float4* __restrict__ src, TileMap map, int fromTiles, kajo::EncodeArgs a,
                                                               const float2* __restrict__ table, void* __restrict__ dst)
{
    __shared__ float2 sTable[kajo::kEncodeTableWords / 2];
    const bool tabled = a.format != kajo::kEncodeRgba16f && a.transfer != kajo::kEncodeLinear;
    if (tabled) {
        for (int i = threadIdx.x; i < kajo::kEncodeTableWords / 2; i += 256)
            sTable[i] = table[i];
        __syncthreads();
    }
    const float* T = reinterpret_cast<const float*>(sTable);
    const bool wide = a.format == kajo::kEncodeRgba16 || a.format == kajo::kEncodeRgba16f;
    const unsigned nbx = (unsigned)(map.W + 63) / 64, nby = (unsigned)(map.H + 3) / 4;
    for (unsigned b = blockIdx.x; b < nbx * nby; b += gridDim.x) {
        const int x = (int)(b % nbx) * 64 + (int)(threadIdx.x & 63);
        const int y = (int)(b / nbx) * 4 + (int)(threadIdx.x >> 6);
        if (x >= map.W || y >= map.H)
            continue;
        const float4 F = sourcePixel(src, map, fromTiles, x, y);
        const uint64_t word = kajo::encodePixel(a, T, F.x, F.y, F.z, (uint32_t)x, (uint32_t)y);
        const size_t at = (size_t)y * map.W + x;
        if (wide)
            static_cast<uint2*>(dst)[at] = make_uint2((uint32_t)word, (uint32_t)(word >> 32));
        else
            static_cast<uint32_t*>(dst)[at] = (uint32_t)word;
    }
}

// words of the table the kernel stages: what the host uploads
extern "C" size_t kajo_encode_table_words(void)
{
    return (size_t)kajo::kEncodeTableWords;
}

// The stage on `stream`: src (tile buffers, or with fromTiles 0 a row-major frame) -> dst (W * H words of 4 or 8 bytes, row-major).
// table: kEncodeTableWords floats in device memory, 8-byte aligned; may be null where none is read (LINEAR, RGBA16F).
extern "C" int kajo_encode_launch(const void* src, const TileMap* map, int fromTiles, const kajo::EncodeArgs* a, const void* table, void* dst,
                                  void* stream)
{
    const bool tabled = a->format != kajo::kEncodeRgba16f && a->transfer != kajo::kEncodeLinear;
    if (map->W < 1 || map->H < 1 || !src || !dst || (tabled && !table) || a->format > kajo::kEncodeRgba16f || a->transfer > kajo::kEncodeLinear)
        return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((map->W + 63) / 64) * (unsigned)((map->H + 3) / 4);
    hipLaunchKernelGGL(kajo_encode, dim3(blocks < kMaxGroups ? blocks : kMaxGroups), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float4*>(src), *map, fromTiles, *a, static_cast<const float2*>(table), dst);
    return (int)hipGetLastError();
}
