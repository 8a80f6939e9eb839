// glare.hip -- glare (bloom) pyramid over one whole frame, in front of the tone curves (kajo_hip_glare, kajo_hip_display_*; the
// definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, in every numerics build alike: the
// arithmetic is this file's own, so only its inputs depend on FAST / EXACT / STRICT.
//
// One lane per output pixel, workgroups of 64x4 pixels, float4 per pixel at every level (.w = 0). Passes, each a kernel on the caller's
// stream:
//   bright   source frame (tile buffers through TileMap, or a row-major frame) -> B0
//   reduce   one per level: B_k -> B_{k+1}, half the size, 4x4 taps [1 3 3 1]^2 renormalised over the taps inside B_k
//   expand   one per level: U_k = (B_k + (n - k) up(U_{k+1})) / (n - k + 1), up = 2x2 taps [3 1]^2 renormalised over the taps inside
//   apply    out = (m + strength (up(U_1) - B0)) P from the source frame, m and B0 formed again as `bright` forms them
// Plain gathers from global memory: neighbouring lanes share three quarters of `reduce`'s taps through the caches. No LDS, no atomics,
// no cross-lane operation; every sum has a fixed order. The source frame is only read.
#include <hip/hip_runtime.h>

#include <math.h>

#include "render_args.h"

namespace
{

struct GlareLevel
{
    int32_t w, h;
};

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

// m = F.rgb / P and B0 = max(m, 0) k of one pixel; false (B0 = 0) where the pixel does not count
__device__ inline bool brightOf(float4 F, float passes, float threshold, float4* m, float4* b0)
{
    *m = make_float4(F.x / passes, F.y / passes, F.z / passes, 0.0f);
    *b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(isfinite(m->x) && isfinite(m->y) && isfinite(m->z)))
        return false;
    const float3 x = make_float3(fmaxf(m->x, 0.0f), fmaxf(m->y, 0.0f), fmaxf(m->z, 0.0f));
    float k = 1.0f;
    if (threshold != 0.0f) {
        const float l = 0.2126f * x.x + 0.7152f * x.y + 0.0722f * x.z;
        k = fmaxf(l - threshold, 0.0f) / fmaxf(l, 1e-6f);
    }
    *b0 = make_float4(x.x * k, x.y * k, x.z * k, 0.0f);
    return true;
}

// up(U)(x, y): per axis the tap at x >> 1 with weight 3 and its neighbour towards x with weight 1, over the taps inside U
__device__ inline float4 upsample(const float4* U, GlareLevel u, int x, int y)
{
    const int x0 = x >> 1, y0 = y >> 1;
    const int x1 = x0 + ((x & 1) ? 1 : -1), y1 = y0 + ((y & 1) ? 1 : -1);
    const bool inX = x1 >= 0 && x1 < u.w, inY = y1 >= 0 && y1 < u.h;
    const float wx1 = inX ? 1.0f : 0.0f, wy1 = inY ? 1.0f : 0.0f;
    const int cx1 = inX ? x1 : x0, cy1 = inY ? y1 : y0; // (a tap outside: weight 0, read from the tap inside)
    const float4 a = U[(size_t)y0 * u.w + x0], b = U[(size_t)y0 * u.w + cx1];
    const float4 c = U[(size_t)cy1 * u.w + x0], d = U[(size_t)cy1 * u.w + cx1];
    const float norm = (3.0f + wx1) * (3.0f + wy1);
    float4 r;
    r.x = (3.0f * (3.0f * a.x + wx1 * b.x) + wy1 * (3.0f * c.x + wx1 * d.x)) / norm;
    r.y = (3.0f * (3.0f * a.y + wx1 * b.y) + wy1 * (3.0f * c.y + wx1 * d.y)) / norm;
    r.z = (3.0f * (3.0f * a.z + wx1 * b.z) + wy1 * (3.0f * c.z + wx1 * d.z)) / norm;
    r.w = 0.0f;
    return r;
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_glare_bright(const float4* src, TileMap map, int fromTiles, float passes, float threshold,
                                                                     float4* b0)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    float4 m, b;
    brightOf(sourcePixel(src, map, fromTiles, x, y), passes, threshold, &m, &b);
    b0[(size_t)y * map.W + x] = b;
}

// B_k (size in) -> B_{k+1} (size out = (in + 1) / 2 per axis)
extern "C" __global__ void __launch_bounds__(256) kajo_glare_reduce(const float4* in, GlareLevel s, float4* out, GlareLevel d)
{
    const int X = blockIdx.x * 64 + (threadIdx.x & 63);
    const int Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X >= d.w || Y >= d.h)
        return;
    const float g[4] = {1.0f, 3.0f, 3.0f, 1.0f};
    float wx[4], wy[4];
    int qx[4], qy[4];
    float sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int px = 2 * X + i - 1, py = 2 * Y + i - 1;
        const bool inX = px >= 0 && px < s.w, inY = py >= 0 && py < s.h;
        wx[i] = inX ? g[i] : 0.0f;
        wy[i] = inY ? g[i] : 0.0f;
        qx[i] = inX ? px : 2 * X; // (a tap outside: weight 0, read from a tap inside)
        qy[i] = inY ? py : 2 * Y;
        sx += wx[i];
        sy += wy[i];
    }
    float3 acc = make_float3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float4* row = in + (size_t)qy[j] * s.w;
        float3 r = make_float3(0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float4 v = row[qx[i]];
            r.x += wx[i] * v.x;
            r.y += wx[i] * v.y;
            r.z += wx[i] * v.z;
        }
        acc.x += wy[j] * r.x;
        acc.y += wy[j] * r.y;
        acc.z += wy[j] * r.z;
    }
    const float norm = sx * sy;
    out[(size_t)Y * d.w + X] = make_float4(acc.x / norm, acc.y / norm, acc.z / norm, 0.0f);
}

// U_k = (B_k + a up(U_{k+1})) / (a + 1), a = n - k
extern "C" __global__ void __launch_bounds__(256) kajo_glare_expand(const float4* bk, GlareLevel s, const float4* next, GlareLevel u, float a, float4* out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= s.w || y >= s.h)
        return;
    const size_t i = (size_t)y * s.w + x;
    const float4 b = bk[i];
    const float4 up = upsample(next, u, x, y);
    const float den = a + 1.0f;
    out[i] = make_float4((b.x + a * up.x) / den, (b.y + a * up.y) / den, (b.z + a * up.z) / den, 0.0f);
}

// out = (m + strength (up(U_1) - B0)) P where the pixel counts, the source pixel where it does not; .w from the source
extern "C" __global__ void __launch_bounds__(256) kajo_glare_apply(const float4* src, TileMap map, int fromTiles, float passes, float threshold,
                                                                    float strength, const float4* u1, GlareLevel u, float4* out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const float4 F = sourcePixel(src, map, fromTiles, x, y);
    float4 m, b, r = F;
    if (brightOf(F, passes, threshold, &m, &b)) {
        const float4 G = upsample(u1, u, x, y);
        r.x = (m.x + strength * (G.x - b.x)) * passes;
        r.y = (m.y + strength * (G.y - b.y)) * passes;
        r.z = (m.z + strength * (G.z - b.z)) * passes;
    }
    out[(size_t)y * map.W + x] = r;
}

// n of include/kajo_hip.h for a W x H frame: min(levels, the reductions that bring the frame to 1 x 1); *pixels (may be null) = the
// float4 slots of the scratch the pyramid of n levels takes: B0, B_1 .. B_n, U_1 .. U_{n-1}
extern "C" int kajo_glare_plan(int W, int H, int levels, size_t* pixels)
{
    int n = 0;
    size_t reduced = 0;
    for (int w = W, h = H; n < levels && (w > 1 || h > 1); n++) {
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        reduced += (size_t)w * h;
    }
    if (pixels)
        *pixels = (size_t)W * H + 2 * reduced;
    return n;
}

// The whole pyramid of n >= 1 levels (kajo_glare_plan) on `stream`: src (tile buffers, or with fromTiles 0 a row-major frame) -> out
// (row-major frame, not the source). scratch: kajo_glare_plan's slots for n levels or more.
extern "C" int kajo_glare_launch(const void* src, const TileMap* map, int fromTiles, float passes, int n, float strength, float threshold,
                                 void* scratch, void* out, void* stream)
{
    const hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int kMaxLevels = 32;
    if (n < 1 || n > kMaxLevels)
        return (int)hipErrorInvalidValue;
    GlareLevel size[kMaxLevels + 1];
    float4* B[kMaxLevels + 1];
    float4* U[kMaxLevels + 1];
    size[0] = {map->W, map->H};
    B[0] = static_cast<float4*>(scratch);
    float4* next = B[0] + (size_t)map->W * map->H;
    for (int k = 1; k <= n; k++) {
        size[k] = {(size[k - 1].w + 1) / 2, (size[k - 1].h + 1) / 2};
        B[k] = next;
        next += (size_t)size[k].w * size[k].h;
    }
    for (int k = 1; k < n; k++) {
        U[k] = next;
        next += (size_t)size[k].w * size[k].h;
    }
    U[n] = B[n];
    const dim3 block(256);
    auto gridOf = [](GlareLevel s) { return dim3((s.w + 63) / 64, (s.h + 3) / 4); };
    const float4* source = static_cast<const float4*>(src);
    hipLaunchKernelGGL(kajo_glare_bright, gridOf(size[0]), block, 0, st, source, *map, fromTiles, passes, threshold, B[0]);
    for (int k = 0; k < n; k++)
        hipLaunchKernelGGL(kajo_glare_reduce, gridOf(size[k + 1]), block, 0, st, B[k], size[k], B[k + 1], size[k + 1]);
    for (int k = n - 1; k >= 1; k--)
        hipLaunchKernelGGL(kajo_glare_expand, gridOf(size[k]), block, 0, st, B[k], size[k], U[k + 1], size[k + 1], (float)(n - k), U[k]);
    hipLaunchKernelGGL(kajo_glare_apply, gridOf(size[0]), block, 0, st, source, *map, fromTiles, passes, threshold, strength, U[1], size[1],
                       static_cast<float4*>(out));
    return (int)hipGetLastError();
}
