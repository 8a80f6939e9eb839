// encode_math.h -- the arithmetic of the encode stage (include/kajo_hip.h "The encode"), host and device: the tone curve on a pixel's
// mean, the lookup in a transfer table, the dither hash, the quantisation and the float -> half conversion. encode.cpp's kernel and
// present.cpp's kajo_hip_encode_pixels are compiled from these same lines, as grade.hip and kajo_hip_grade_pixels are from grade_math.h:
// what a test reads from the host is what the device computes. float32 IEEE with correctly rounded division, no contraction (the pragma
// below on the host; -ffp-contract=off for the device), in the order written; no pow, exp or log anywhere: the transfers are tables the
// host forms in binary64 (encode_host.h). Pure functions, no state.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define KEM_FN __host__ __device__ static inline
#else
#define KEM_FN static inline
#endif

namespace kajo
{

// The table: E knots per binade over [2^-32, 1), entry i = (T_i, S_i) at words 2 i and 2 i + 1; the last entry, i = 32 E, is
// (T64(1), the slope below 2^-32). E = 128 is the smallest power of two that keeps the table within a quarter of a 16-bit code of the
// analytic transfers (the sweep).
constexpr int kEncodeLog2E = 7;
constexpr int kEncodeBinades = 32;
constexpr int kEncodeKnots = kEncodeBinades << kEncodeLog2E;     // knots below 1.0
constexpr int kEncodeTableWords = 2 * (kEncodeKnots + 1);        // 8194 floats, 32776 bytes
constexpr uint32_t kEncodeBase = (uint32_t)(127 - kEncodeBinades) << kEncodeLog2E; // the index bits of 2^-32

// KajoEncodeParams' enumerators, as the kernel numbers them (present.cpp asserts that they are the header's)
enum : uint32_t
{
    kEncodeArgb8 = 0,
    kEncodeRgb10a2 = 1,
    kEncodeRgba16 = 2,
    kEncodeRgba16f = 3,
    kEncodeGamma22 = 0,
    kEncodeSrgb = 1,
    kEncodePq = 2,
    kEncodeLinear = 3,
    kEncodeDither = 1,
    kEncodeScene = 2,
};

// what a pixel's words depend on besides the pixel: by value to the kernel, and kajo_hip_encode_pixels' own
struct EncodeArgs
{
    uint32_t format, transfer, flags;
    int32_t curve;     // KAJO_TONE_CURVE_* of render_args.h
    float scale;       // s = 2^exposure
    float white;       // REINHARD's white point, 0 = none
    uint32_t seed;     // of the dither
    float passes;      // P
};

KEM_FN uint32_t encodeBits(float f)
{
    uint32_t b;
    __builtin_memcpy(&b, &f, sizeof b);
    return b;
}

KEM_FN float encodeFloat(uint32_t b)
{
    float f;
    __builtin_memcpy(&f, &b, sizeof f);
    return f;
}

KEM_FN bool encodeFinite(float x)
{
    return (encodeBits(x) & 0x7f800000u) != 0x7f800000u;
}

// max(t, 0) and min(t, 1) as the stage means them: 0 for a NaN and +0 for -0; a NaN never reaches the min
KEM_FN float encodeMax0(float t)
{
    return t > 0.0f ? t : 0.0f;
}

KEM_FN float encodeMin1(float t)
{
    return t < 1.0f ? t : 1.0f;
}

// x = m * s and y = curve(x): tonemap.inc.hip toneWord's expressions in its order. counts: all three channels of m are finite; a pixel
// that does not count is mapped by CLAMP.
KEM_FN void encodeCurve(const EncodeArgs& a, const float m[3], float x[3], float y[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const bool counts = encodeFinite(m[0]) && encodeFinite(m[1]) && encodeFinite(m[2]);
    for (int k = 0; k < 3; k++)
        x[k] = m[k] * a.scale;
    if (counts && a.curve == 1) { // REINHARD
        const float L = (0.2126f * x[0] + 0.7152f * x[1]) + 0.0722f * x[2];
        const float ratio = a.white > 0.0f ? (1.0f + L / (a.white * a.white)) / (1.0f + L) : 1.0f / (1.0f + L);
        for (int k = 0; k < 3; k++)
            y[k] = L > 0.0f ? encodeMin1(encodeMax0(x[k] * ratio)) : 0.0f;
    } else if (counts && a.curve == 2) { // ACES
        for (int k = 0; k < 3; k++) {
            const float v = x[k] < 1e4f ? x[k] : 1e4f;
            y[k] = encodeMin1(encodeMax0((v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f)));
        }
    } else {
        for (int k = 0; k < 3; k++)
            y[k] = encodeMin1(encodeMax0(x[k]));
    }
}

// v = T(y) for y in [0, 1] (what the curves give): the knot below y by its top bits, one exact subtraction, one multiply, one add, and
// the next knot's value as a cap, which keeps v non-decreasing across knots
KEM_FN float encodeLookup(const float* table, float y)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (y >= 1.0f)
        return table[2 * kEncodeKnots];
    const uint32_t bits = encodeBits(y);
    const uint32_t top = bits >> (23 - kEncodeLog2E);
    if (top < kEncodeBase) // y < 2^-32 (and +0)
        return y * table[2 * kEncodeKnots + 1];
    const uint32_t i = top - kEncodeBase; // < kEncodeKnots: y < 1
    const float yk = encodeFloat(top << (23 - kEncodeLog2E));
    const float t = table[2 * i] + (y - yk) * table[2 * i + 1];
    const float cap = table[2 * i + 2];
    return t < cap ? t : cap;
}

// The dither's hash, modulo 2^32: the row's word (py, channel and seed through a multiply-xorshift finaliser), then a step of the golden
// ratio per pixel of the row -- along a row the offsets are an additive recurrence, which spreads them evenly over short runs
KEM_FN uint32_t encodeHash(uint32_t px, uint32_t py, uint32_t channel, uint32_t seed)
{
    uint32_t h = py * 0x85EBCA6Bu;
    h ^= channel * 0xC2B2AE35u;
    h ^= seed;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h + px * 0x9E3779B9u;
}

// d of the quantiser: ((hash >> 8) + 0.5) 2^-24 in float32 (the sum rounds to even from 2^23 on; d lies in (0, 1])
KEM_FN float encodeDither(uint32_t px, uint32_t py, uint32_t channel, uint32_t seed)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return ((float)(encodeHash(px, py, channel, seed) >> 8) + 0.5f) * 5.9604644775390625e-8f;
}

// code = floor(v M + d) clamped to [0, M], for v in [0, 1]: the sum is not negative, so the conversion's truncation is the floor
KEM_FN uint32_t encodeQuantise(float v, float maxCode, float d)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float q = v * maxCode + d;
    const uint32_t c = (uint32_t)(int32_t)q;
    const uint32_t m = (uint32_t)(int32_t)maxCode;
    return c < m ? c : m;
}

// float32 -> binary16, round to nearest even, by integer operations; for finite f of magnitude below 65520 (the stage hands it [0, 65504])
KEM_FN uint32_t encodeHalf(float f)
{
    const uint32_t b = encodeBits(f);
    const uint32_t sign = (b >> 16) & 0x8000u;
    const uint32_t a = b & 0x7fffffffu;
    if (a < 0x33000000u) // below 2^-25, and 2^-25 itself: the tie goes to the even 0
        return sign;
    if (a < 0x38800000u) { // below 2^-14: a subnormal half, the significand in units of 2^-24
        const uint32_t s = 126u - (a >> 23); // 14 .. 24
        const uint32_t m = (a & 0x7fffffu) | 0x800000u;
        const uint32_t h = m >> s, rem = m & ((1u << s) - 1u), halfway = 1u << (s - 1u);
        return sign | (h + ((rem > halfway || (rem == halfway && (h & 1u))) ? 1u : 0u));
    }
    const uint32_t r = a - 0x38000000u;
    const uint32_t h = r >> 13, rem = r & 0x1fffu;
    return sign | (h + ((rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ? 1u : 0u));
}

// One pixel: F.rgb the sums over passes, (px, py) its place in the whole frame -> the word (a 4-byte format's in the low half).
// table: the transfer's, not read for LINEAR
KEM_FN uint64_t encodePixel(const EncodeArgs& a, const float* table, float F0, float F1, float F2, uint32_t px, uint32_t py)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float m[3] = {F0 / a.passes, F1 / a.passes, F2 / a.passes};
    float x[3], y[3];
    encodeCurve(a, m, x, y);
    uint32_t c[3];
    if (a.format == kEncodeRgba16f) {
        for (int k = 0; k < 3; k++) {
            float v = y[k];
            if (a.flags & kEncodeScene) {
                v = encodeMax0(x[k]);
                v = v < 65504.0f ? v : 65504.0f;
            }
            c[k] = encodeHalf(v);
        }
        return (uint64_t)c[0] | ((uint64_t)c[1] << 16) | ((uint64_t)c[2] << 32) | ((uint64_t)0x3C00u << 48);
    }
    const float maxCode = a.format == kEncodeArgb8 ? 255.0f : a.format == kEncodeRgb10a2 ? 1023.0f : 65535.0f;
    for (int k = 0; k < 3; k++) {
        const float v = a.transfer == kEncodeLinear ? y[k] : encodeLookup(table, y[k]);
        const float d = (a.flags & kEncodeDither) ? encodeDither(px, py, (uint32_t)k, a.seed) : 0.5f;
        c[k] = encodeQuantise(v, maxCode, d);
    }
    if (a.format == kEncodeArgb8)
        return 0xFF000000u | (c[0] << 16) | (c[1] << 8) | c[2];
    if (a.format == kEncodeRgb10a2)
        return 0xC0000000u | (c[0] << 20) | (c[1] << 10) | c[2];
    return (uint64_t)c[0] | ((uint64_t)c[1] << 16) | ((uint64_t)c[2] << 32) | ((uint64_t)0xFFFFu << 48);
}

// The float view (include/kajo_hip.h "The float view"; encode_view.cpp and present.cpp's kajo_hip_encode_view_pixels) cuts encodePixel in
// two and resamples between the halves. The lines are encodePixel's.

// true: the view resamples scene-linear x (RGBA16F with SCENE), not the curve's y
KEM_FN bool encodeViewScene(const EncodeArgs& a)
{
    return a.format == kEncodeRgba16f && (a.flags & kEncodeScene) != 0;
}

// The front: F.rgb the sums over passes -> L, steps 1-3 (with SCENE what step 6 would round to half). Finite, in [0, 1] or [0, 65504].
KEM_FN void encodeFront(const EncodeArgs& a, float F0, float F1, float F2, float L[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float m[3] = {F0 / a.passes, F1 / a.passes, F2 / a.passes};
    float x[3], y[3];
    encodeCurve(a, m, x, y);
    for (int k = 0; k < 3; k++) {
        float v = y[k];
        if (encodeViewScene(a)) {
            v = encodeMax0(x[k]);
            v = v < 65504.0f ? v : 65504.0f;
        }
        L[k] = v;
    }
}

// The clamp behind the resampling: Lanczos has negative lobes and a row's weights sum to 1 only within count * 2^-24
KEM_FN float encodeViewClamp(const EncodeArgs& a, float r)
{
    const float t = encodeMax0(r);
    if (encodeViewScene(a))
        return t < 65504.0f ? t : 65504.0f;
    return encodeMin1(t);
}

// The back: q (clamped) in place of y -- with SCENE of the clamped x --, (px, py) the OUTPUT pixel -> the word, steps 4-6
KEM_FN uint64_t encodeBack(const EncodeArgs& a, const float* table, const float q[3], uint32_t px, uint32_t py)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    uint32_t c[3];
    if (a.format == kEncodeRgba16f) {
        for (int k = 0; k < 3; k++)
            c[k] = encodeHalf(q[k]);
        return (uint64_t)c[0] | ((uint64_t)c[1] << 16) | ((uint64_t)c[2] << 32) | ((uint64_t)0x3C00u << 48);
    }
    const float maxCode = a.format == kEncodeArgb8 ? 255.0f : a.format == kEncodeRgb10a2 ? 1023.0f : 65535.0f;
    for (int k = 0; k < 3; k++) {
        const float v = a.transfer == kEncodeLinear ? q[k] : encodeLookup(table, q[k]);
        const float d = (a.flags & kEncodeDither) ? encodeDither(px, py, (uint32_t)k, a.seed) : 0.5f;
        c[k] = encodeQuantise(v, maxCode, d);
    }
    if (a.format == kEncodeArgb8)
        return 0xFF000000u | (c[0] << 16) | (c[1] << 8) | c[2];
    if (a.format == kEncodeRgb10a2)
        return 0xC0000000u | (c[0] << 20) | (c[1] << 10) | c[2];
    return (uint64_t)c[0] | ((uint64_t)c[1] << 16) | ((uint64_t)c[2] << 32) | ((uint64_t)0xFFFFu << 48);
}

} // namespace kajo
