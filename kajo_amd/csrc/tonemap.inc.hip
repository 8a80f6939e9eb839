// tonemap.inc.hip -- exposure, tone curves and automatic exposure in the image resolve (include/kajo_hip.h kajo_hip_tonemap_argb8; the
// definition is written there), included by kernel_fast.hip and kernel_strict.hip behind integrator.inc.hip: the mean and the display
// transform are formed with the build's own kdiv / kpow, in the same expressions as the resolve kernels, so that the default parameters give
// the resolve's image bit for bit. The STRICT instances serve STRICT and EXACT handles, as the resolve's do.
//
// Kernels, each on the handle's stream, each in two forms: reading through a TileMap (a handle's own tile buffer or `tileCount` gathered
// ones) or reading a row-major float4 frame (the composed frame, the denoiser's output).
//   logavg  auto exposure, stage 1: one workgroup per fixed 64x16 rectangle of the image, numbered in image order. Lane l of wave w takes
//           column l and rows 4k + w, k = 0..3, of the rectangle -- the same pixels in the same order whatever holds them -- and sums
//           log(1e-4 + max(l(m), 0)) of those that count in float64; the wave by a ds_swizzle butterfly (xor 1 .. 16), the two half-waves and
//           the four waves in a fixed order through LDS. Writes (sum, count) of the rectangle as one double2. No atomics.
//   scale   stage 2: one workgroup sums the partials -- lane t the rectangles t, t + 256, ... in order, then the same fixed reduction --
//           and writes s = 2^exposure * key / Lavg to a device word.
//   map     one lane per pixel (the resolve's shapes: 64x4 pixels per workgroup from tiles, 256 consecutive pixels from a frame): mean,
//           exposure, curve, display transform, one ARGB8 word. s comes from the device word when the frame's own log-average sets it.
#define KAJO_TONE_NAME(k) KAJO_CAT(k, KAJO_TONE_SUFFIX)

namespace
{

constexpr int kToneRectW = 64, kToneRectH = 16; // the logavg rectangle: 256 lanes x 4 rows

// The pixel (x, y) of the frame: through the tile map, or row-major
template <bool Tiles>
KDEV float4 toneLoad(const float4* src, const TileMap& map, int x, int y)
{
    if (Tiles) {
        int owner;
        uint32_t slot;
        kajoTileSlot(map, x, y, &owner, &slot);
        return src[(size_t)owner * map.slotsPerOwner + slot];
    }
    return src[(size_t)y * map.W + x];
}

// v of the lane `lane ^ Xor` (Xor < 32: inside the half-wave), ds_swizzle's bit-mask mode: and 0x1f, or 0, xor Xor
template <int Xor>
KDEV double toneSwizzle(double v)
{
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)b, 0x1f | (Xor << 10));
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)(b >> 32), 0x1f | (Xor << 10));
    return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}

// The sum over the half-wave, in every lane of it. Each step adds the same two values in both lanes of a pair (a + b = b + a), so the
// result is one value per half-wave and a function of the lanes' values alone.
KDEV double toneHalfWaveSum(double v)
{
    v += toneSwizzle<1>(v);
    v += toneSwizzle<2>(v);
    v += toneSwizzle<4>(v);
    v += toneSwizzle<8>(v);
    v += toneSwizzle<16>(v);
    return v;
}

// (sum, count) of the workgroup's 256 lanes into thread 0's return value: half-waves through LDS, summed in half-wave order
KDEV double2 toneGroupSum(double sum, double count)
{
    __shared__ double2 half[8];
    sum = toneHalfWaveSum(sum);
    count = toneHalfWaveSum(count);
    if ((threadIdx.x & 31) == 0)
        half[threadIdx.x >> 5] = make_double2(sum, count);
    __syncthreads();
    double2 r = make_double2(0.0, 0.0);
    if (threadIdx.x == 0)
        for (int k = 0; k < 8; k++) {
            r.x += half[k].x;
            r.y += half[k].y;
        }
    return r;
}

// the mean of a pixel counts: all three channels finite
KDEV bool toneCounts(float r, float g, float b)
{
    return isfinite(r) && isfinite(g) && isfinite(b);
}

template <bool Tiles>
KDEV void toneLogAvg(const float4* src, const TileMap& map, float passes, double2* partials)
{
    const int x = blockIdx.x * kToneRectW + (threadIdx.x & 63);
    const int y0 = blockIdx.y * kToneRectH + (threadIdx.x >> 6);
    float4 a[4];
    for (int k = 0; k < 4; k++) // (the four loads first: they are in flight together)
        a[k] = (x < map.W && y0 + 4 * k < map.H) ? toneLoad<Tiles>(src, map, x, y0 + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
    double sum = 0.0, count = 0.0;
    for (int k = 0; k < 4; k++) {
        const float r = kdiv(a[k].x, passes), g = kdiv(a[k].y, passes), b = kdiv(a[k].z, passes);
        if (x < map.W && y0 + 4 * k < map.H && toneCounts(r, g, b)) {
            const double l = 0.2126 * (double)r + 0.7152 * (double)g + 0.0722 * (double)b;
            sum += log(1e-4 + fmax(l, 0.0));
            count += 1.0;
        }
    }
    const double2 s = toneGroupSum(sum, count);
    if (threadIdx.x == 0)
        partials[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// y of the curve for the exposed colour x, then the resolve's display transform (integrator.inc.hip KAJO_RESOLVE_NAME, the same expressions)
KDEV uint32_t toneWord(float4 a, float passes, const ToneArgs& t, float s)
{
    const float m[3] = {kdiv(a.x, passes), kdiv(a.y, passes), kdiv(a.z, passes)};
    const float x[3] = {m[0] * s, m[1] * s, m[2] * s};
    const bool counts = toneCounts(m[0], m[1], m[2]);
    float y[3];
    if (counts && t.curve == KAJO_TONE_CURVE_REINHARD) {
        // Ld / L = (1 + L / white^2) / (1 + L), or 1 / (1 + L) without a white point
        const float L = 0.2126f * x[0] + 0.7152f * x[1] + 0.0722f * x[2];
        const float ratio = t.white > 0.0f ? kdiv(1.0f + kdiv(L, t.white * t.white), 1.0f + L) : kdiv(1.0f, 1.0f + L);
        for (int k = 0; k < 3; k++)
            y[k] = L > 0.0f ? fminf(fmaxf(x[k] * ratio, 0.0f), 1.0f) : 0.0f;
    } else if (counts && t.curve == KAJO_TONE_CURVE_ACES) {
        for (int k = 0; k < 3; k++) {
            const float v = fminf(x[k], 1e4f); // (the curve is above 1 from x = 7.24 on: the bound changes no output, and keeps v * v finite)
            y[k] = fminf(fmaxf(kdiv(v * (2.51f * v + 0.03f), v * (2.43f * v + 0.59f) + 0.14f), 0.0f), 1.0f);
        }
    } else {
        for (int k = 0; k < 3; k++)
            y[k] = fminf(fmaxf(x[k], 0.0f), 1.0f);
    }
    int out[3];
    for (int k = 0; k < 3; k++) {
        const float v = kpow(y[k], 1 / 2.2f);
        out[k] = (int)(v * 255.f + .5f);
    }
    const int al = (int)(1.f * 255.f + .5f);
    return ((uint32_t)al << 24) | ((uint32_t)out[0] << 16) | ((uint32_t)out[1] << 8) | (uint32_t)out[2];
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) KAJO_TONE_NAME(kajo_tone_logavg_tiles)(const float4* gathered, TileMap map, float passes,
                                                                                          double2* partials)
{
    toneLogAvg<true>(gathered, map, passes, partials);
}

extern "C" __global__ void __launch_bounds__(256) KAJO_TONE_NAME(kajo_tone_logavg_frame)(const float4* frame, TileMap map, float passes,
                                                                                          double2* partials)
{
    toneLogAvg<false>(frame, map, passes, partials);
}

extern "C" __global__ void __launch_bounds__(256) KAJO_TONE_NAME(kajo_tone_scale)(const double2* partials, int count, ToneArgs t, float* scale)
{
    double sum = 0.0, n = 0.0;
    int r = threadIdx.x;
    for (; r + 7 * 256 < count; r += 8 * 256) { // (eight loads in flight, then the same additions in the same order)
        double2 p[8];
        for (int k = 0; k < 8; k++)
            p[k] = partials[r + k * 256];
        for (int k = 0; k < 8; k++) {
            sum += p[k].x;
            n += p[k].y;
        }
    }
    for (; r < count; r += 256) {
        const double2 p = partials[r];
        sum += p.x;
        n += p.y;
    }
    const double2 s = toneGroupSum(sum, n);
    if (threadIdx.x == 0) {
        const double a = s.y > 0.0 ? (double)t.key / exp(s.x / s.y) : 1.0;
        scale[0] = (float)((double)t.exposureScale * a);
    }
}

extern "C" __global__ void __launch_bounds__(256) KAJO_TONE_NAME(kajo_tone_map_tiles)(const float4* gathered, TileMap map, float passes, ToneArgs t,
                                                                                       const float* scale, uint32_t* dst)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    const float s = scale ? scale[0] : t.exposureScale;
    dst[(size_t)y * map.W + x] = toneWord(toneLoad<true>(gathered, map, x, y), passes, t, s);
}

extern "C" __global__ void __launch_bounds__(256) KAJO_TONE_NAME(kajo_tone_map_frame)(const float4* frame, int count, float passes, ToneArgs t,
                                                                                       const float* scale, uint32_t* dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const float s = scale ? scale[0] : t.exposureScale;
    dst[i] = toneWord(frame[i], passes, t, s);
}

// The whole tone mapping on `stream`. map: the frame's geometry and, with fromTiles, the tile map `src` is read through; otherwise `src` is
// the row-major frame. scratch: kajo_tone_scratch_bytes(W, H) bytes, the scale word at its start. With t->autoExposure the three stages run
// and the map reads s from the scale word; without, s = t->exposureScale and nothing is written to the scratch.
extern "C" int KAJO_CAT(KAJO_TONE_NAME(kajo_tone), _launch)(const void* src, const TileMap* map, int fromTiles, float passes, const ToneArgs* t, void* scratch,
                                                void* dst, void* stream)
{
    const hipStream_t st = static_cast<hipStream_t>(stream);
    float* scale = nullptr;
    if (t->autoExposure) {
        scale = static_cast<float*>(scratch);
        double2* partials = reinterpret_cast<double2*>(static_cast<char*>(scratch) + KAJO_TONE_PARTIALS_OFFSET);
        const dim3 rects((map->W + kToneRectW - 1) / kToneRectW, (map->H + kToneRectH - 1) / kToneRectH);
        if (fromTiles)
            hipLaunchKernelGGL(KAJO_TONE_NAME(kajo_tone_logavg_tiles), rects, dim3(256), 0, st, static_cast<const float4*>(src), *map, passes, partials);
        else
            hipLaunchKernelGGL(KAJO_TONE_NAME(kajo_tone_logavg_frame), rects, dim3(256), 0, st, static_cast<const float4*>(src), *map, passes, partials);
        hipLaunchKernelGGL(KAJO_TONE_NAME(kajo_tone_scale), dim3(1), dim3(256), 0, st, partials, (int)(rects.x * rects.y), *t, scale);
    }
    if (fromTiles)
        hipLaunchKernelGGL(KAJO_TONE_NAME(kajo_tone_map_tiles), dim3((map->W + 63) / 64, (map->H + 3) / 4), dim3(256), 0, st,
                           static_cast<const float4*>(src), *map, passes, *t, scale, static_cast<uint32_t*>(dst));
    else {
        const int count = map->W * map->H;
        hipLaunchKernelGGL(KAJO_TONE_NAME(kajo_tone_map_frame), dim3((count + 255) / 256), dim3(256), 0, st, static_cast<const float4*>(src), count,
                           passes, *t, scale, static_cast<uint32_t*>(dst));
    }
    return (int)hipGetLastError();
}
