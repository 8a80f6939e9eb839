// lens.hip -- depth of field of one whole frame, between the denoiser and the glare (kajo_hip_lens, kajo_hip_lens_coc,
// kajo_hip_present_lens_argb8; the definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, in every
// numerics build alike: the arithmetic is this file's own, so only its inputs depend on FAST / EXACT / STRICT.
//
// An image-space approximation of a thin lens: one depth per pixel (the depth AOV), a gather over the discs of the neighbours; nothing
// behind a foreground object can be revealed. Two kernels on the caller's stream:
//   prepare  one lane per pixel, workgroups of 64x4. Reads the AOV sums A.w (hits) and B.w (depth) and, unless only the planes are asked
//            for (kajo_hip_lens_coc), the source frame F (tile buffers through TileMap, or a row-major frame). Writes the planes z and r
//            of the definition and the tap record {m.rgb, r}; a pixel that does not count is marked by the record {0, 0, 0, -1}: with
//            r_q = -1 the definition's own arithmetic gives c = 0 and w = +0 whatever p is, so such a tap needs no branch.
//   gather   the hot path: one lane per output pixel, workgroups of 32x16 pixels (8 waves, each two rows of 32). The workgroup stages its
//            tile plus a halo of maxRadius pixels -- at most 64x48 records, 60 KiB -- in LDS: neighbouring outputs share almost the whole
//            window, and two workgroups fit the CU's 160 KiB. The records are float4 (one ds_read_b128 a tap: 16 consecutive lanes read
//            256 consecutive bytes, every 16-byte slot of the bank row once) beside a plane of z (ds_read_b32: the two rows of a wave
//            are its two 32-lane halves, which never conflict). Taps outside the image are staged as records that do not count. The tap
//            distances d = sqrtf(dx^2 + dy^2) are a 17x17 table in LDS formed once per workgroup (one correctly rounded square root
//            each), read at a wave-uniform address.
//            Window bound: while it stages, the workgroup takes the largest r in tile plus halo; with t = rmax + 1 no tap with d >= t
//            can have c > 0, so the loops run over |dy| <= K = ceil(t) - 1 and per row over |dx| <= min(K, floor(sqrt(t^2 - dy^2)) + 1).
//            A tap with c == 0 adds +-0 to sums that start at +0, the order of the remaining taps is the definition's (dy outer, dx
//            inner): the bound cannot change a bit, and an in-focus region costs a few taps a pixel.
// No atomics, no order between workgroups, no FMA: the output at a pixel depends on the inputs through image coordinates only. The source
// frame and the AOVs are only read.
#include <hip/hip_runtime.h>

#include <math.h>

#include "render_args.h"

namespace
{

constexpr int kMaxRadius = 16; // KAJO_LENS_MAX_RADIUS
constexpr int kTileW = 32, kTileH = 16;
constexpr int kRegionW = kTileW + 2 * kMaxRadius, kRegionH = kTileH + 2 * kMaxRadius; // 64 x 48
constexpr int kDistN = kMaxRadius + 1;

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

// z, r and (with a source) the tap record of every pixel
extern "C" __global__ void __launch_bounds__(256) kajo_lens_prepare(const float4* __restrict__ src, TileMap map, int fromTiles, float passes,
                                                                     const float4* __restrict__ albedoHits, const float4* __restrict__ normalDepth,
                                                                     float aperture, float focusDistance, float maxRadius,
                                                                     float4* __restrict__ tap, float* __restrict__ radius, float* __restrict__ depth)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const size_t at = (size_t)y * map.W + x;
    const float a = albedoHits[at].w, b = normalDepth[at].w;
    float z = __builtin_inff();
    if (a > 0.0f) {
        const float q = b / a;
        if (isfinite(q) && q > 0.0f)
            z = q;
    }
    const float u = fabsf(1.0f - focusDistance / z);
    const float r = fminf((aperture * (float)map.H) * u, maxRadius);
    radius[at] = r;
    depth[at] = z;
    if (tap) {
        const float4 F = sourcePixel(src, map, fromTiles, x, y);
        const float mx = F.x / passes, my = F.y / passes, mz = F.z / passes;
        const bool counts = isfinite(mx) && isfinite(my) && isfinite(mz);
        tap[at] = counts ? make_float4(mx, my, mz, r) : make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    }
}

// out = the gather of the definition where the pixel counts, the source pixel where it does not; .w from the source. R = maxRadius.
extern "C" __global__ void __launch_bounds__(512) kajo_lens_gather(const float4* __restrict__ src, TileMap map, int fromTiles, float passes,
                                                                    const float4* __restrict__ tap, const float* __restrict__ depth, int R,
                                                                    float4* __restrict__ out)
{
    __shared__ float4 sTap[kRegionW * kRegionH];
    __shared__ float sZ[kRegionW * kRegionH];
    __shared__ float sDist[kDistN * kDistN];
    __shared__ float sMax[8];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    for (int i = tid; i < kDistN * kDistN; i += 512) {
        const int ay = i / kDistN, ax = i - ay * kDistN;
        sDist[i] = sqrtf((float)(ax * ax + ay * ay));
    }
    // the tile and its halo; the largest r among the records that count
    const int regionW = kTileW + 2 * R, regionH = kTileH + 2 * R;
    float rmax = 0.0f;
    for (int i = tid; i < regionW * regionH; i += 512) {
        const int ry = i / regionW, rx = i - ry * regionW;
        const int gx = x0 - R + rx, gy = y0 - R + ry;
        float4 t = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        float z = 0.0f;
        if (gx >= 0 && gx < map.W && gy >= 0 && gy < map.H) {
            const size_t g = (size_t)gy * map.W + gx;
            t = tap[g];
            z = depth[g];
        }
        sTap[ry * kRegionW + rx] = t;
        sZ[ry * kRegionW + rx] = z;
        rmax = fmaxf(rmax, t.w);
    }
    for (int off = 32; off > 0; off >>= 1)
        rmax = fmaxf(rmax, __shfl_xor(rmax, off));
    if ((tid & 63) == 0)
        sMax[tid >> 6] = rmax;
    __syncthreads();

    const int lx = tid & (kTileW - 1), ly = tid / kTileW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= map.W || y >= map.H)
        return;
    const size_t at = (size_t)y * map.W + x;
    const float4 F = sourcePixel(src, map, fromTiles, x, y);
    const int centre = (ly + R) * kRegionW + (lx + R);
    const float rp = sTap[centre].w, zp = sZ[centre];
    if (rp < 0.0f) {
        out[at] = F;
        return;
    }
    rmax = sMax[0];
    for (int i = 1; i < 8; i++)
        rmax = fmaxf(rmax, sMax[i]);
    // the window: c > 0 needs d < re + 1 <= t
    const float t = rmax + 1.0f;
    const int K = __builtin_amdgcn_readfirstlane(min(R, (int)ceilf(t) - 1));
    const float pi = 3.14159265358979323846f;
    float sumW = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int dy = -K; dy <= K; dy++) {
        const int ady = dy < 0 ? -dy : dy;
        const int kx = min(K, (int)sqrtf(fmaxf(t * t - (float)(dy * dy), 0.0f)) + 1);
        const int row = centre + dy * kRegionW;
        for (int dx = -kx; dx <= kx; dx++) {
            const float4 q = sTap[row + dx];
            const float zq = sZ[row + dx];
            const float d = sDist[ady * kDistN + (dx < 0 ? -dx : dx)];
            const float re = zq <= zp ? q.w : fminf(q.w, rp);
            const float te = re + 1.0f;
            const float c = fminf(fmaxf(te - d, 0.0f), 1.0f);
            if (c > 0.0f) {
                const float w = c / (1.0f + pi * (re * te));
                sumW += w;
                sx += w * q.x;
                sy += w * q.y;
                sz += w * q.z;
            }
        }
    }
    out[at] = make_float4((sx / sumW) * passes, (sy / sumW) * passes, (sz / sumW) * passes, F.w);
}

// floats of one plane of a W x H frame (padded to 16 bytes). The stage's scratch: the planes r and z, then the tap records float4 [W * H]
// (from a 16-byte boundary), then the output frame float4 [W * H]
extern "C" size_t kajo_lens_plane(int W, int H)
{
    return ((size_t)W * H + 3) / 4 * 4;
}

// The planes alone on `stream`: scratch as above; r at its start, z one plane further
extern "C" int kajo_lens_coc_launch(const TileMap* map, const void* albedoHits, const void* normalDepth, float aperture, float focusDistance,
                                    int maxRadius, void* scratch, void* stream)
{
    if (map->W < 1 || map->H < 1 || maxRadius < 1 || maxRadius > kMaxRadius)
        return (int)hipErrorInvalidValue;
    const size_t plane = kajo_lens_plane(map->W, map->H);
    float* radius = static_cast<float*>(scratch);
    const dim3 block(256), grid((map->W + 63) / 64, (map->H + 3) / 4);
    hipLaunchKernelGGL(kajo_lens_prepare, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const float4*>(nullptr), *map, 0, 1.0f,
                       static_cast<const float4*>(albedoHits), static_cast<const float4*>(normalDepth), aperture, focusDistance, (float)maxRadius,
                       static_cast<float4*>(nullptr), radius, radius + plane);
    return (int)hipGetLastError();
}

// The stage on `stream`: src (tile buffers, or with fromTiles 0 a row-major frame) -> out (row-major frame, not the source)
extern "C" int kajo_lens_launch(const void* src, const TileMap* map, int fromTiles, float passes, const void* albedoHits, const void* normalDepth,
                                float aperture, float focusDistance, int maxRadius, void* scratch, void* out, void* stream)
{
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (map->W < 1 || map->H < 1 || maxRadius < 1 || maxRadius > kMaxRadius)
        return (int)hipErrorInvalidValue;
    const size_t plane = kajo_lens_plane(map->W, map->H);
    float* radius = static_cast<float*>(scratch);
    float* depth = radius + plane;
    float4* tap = reinterpret_cast<float4*>(radius + 2 * plane);
    const float4* source = static_cast<const float4*>(src);
    hipLaunchKernelGGL(kajo_lens_prepare, dim3((map->W + 63) / 64, (map->H + 3) / 4), dim3(256), 0, st, source, *map, fromTiles, passes,
                       static_cast<const float4*>(albedoHits), static_cast<const float4*>(normalDepth), aperture, focusDistance, (float)maxRadius, tap,
                       radius, depth);
    hipLaunchKernelGGL(kajo_lens_gather, dim3((map->W + kTileW - 1) / kTileW, (map->H + kTileH - 1) / kTileH), dim3(512), 0, st, source, *map,
                       fromTiles, passes, static_cast<const float4*>(tap), static_cast<const float*>(depth), maxRadius,
                       static_cast<float4*>(out));
    return (int)hipGetLastError();
}
