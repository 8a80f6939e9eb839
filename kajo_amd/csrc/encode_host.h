// encode_host.h -- the host half of the encode stage (include/kajo_hip.h "The encode"): the refusals of KajoEncodeParams, the transfer
// tables in binary64 rounded once to float32, and the definition over an array of means through encode_math.h, the kernel's own lines.
// Pure host code without HIP and without the handle: present.cpp's kajo_hip_encode_table, kajo_hip_encode_bytes and
// kajo_hip_encode_pixels are these functions behind the library's error text, and tools/encode_san.cpp runs them under the sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "encode_math.h"
#include "kajo_hip.h"

namespace kajo
{

static_assert(sizeof(KajoEncodeParams) == 32, "include/kajo_hip.h states the size");
static_assert(KAJO_ENCODE_ARGB8 == kEncodeArgb8 && KAJO_ENCODE_RGB10A2 == kEncodeRgb10a2 && KAJO_ENCODE_RGBA16 == kEncodeRgba16 &&
                  KAJO_ENCODE_RGBA16F == kEncodeRgba16f && KAJO_TRANSFER_GAMMA22 == kEncodeGamma22 && KAJO_TRANSFER_SRGB == kEncodeSrgb &&
                  KAJO_TRANSFER_PQ == kEncodePq && KAJO_TRANSFER_LINEAR == kEncodeLinear && KAJO_ENCODE_DITHER == kEncodeDither &&
                  KAJO_ENCODE_SCENE == kEncodeScene && KAJO_ENCODE_TABLE_WORDS == kEncodeTableWords,
              "encode_math.h numbers the formats, transfers and flags as include/kajo_hip.h does");

// The refusals of KajoEncodeParams in the header's order: the text, or null for parameters that pass
inline const char* encodeRefusal(const KajoEncodeParams* p)
{
    if (!p)
        return "null encode parameters";
    if (p->format > KAJO_ENCODE_RGBA16F)
        return "unknown encode format";
    if (p->transfer > KAJO_TRANSFER_LINEAR)
        return "unknown encode transfer";
    if (p->flags & ~(KAJO_ENCODE_DITHER | KAJO_ENCODE_SCENE))
        return "unknown encode flag";
    for (uint32_t r : p->reserved)
        if (r != 0)
            return "encode reserved fields must be 0";
    if (p->format == KAJO_ENCODE_RGBA16F && p->transfer != KAJO_TRANSFER_LINEAR)
        return "the half-float format stores linear values: its transfer must be linear";
    if ((p->flags & KAJO_ENCODE_SCENE) && p->format != KAJO_ENCODE_RGBA16F)
        return "scene-linear output needs the half-float format";
    if ((p->flags & KAJO_ENCODE_DITHER) && p->format == KAJO_ENCODE_RGBA16F)
        return "dither is for the integer formats";
    if (p->transfer == KAJO_TRANSFER_PQ && !(std::isfinite(p->peakNits) && p->peakNits > 0.0f && p->peakNits <= 10000.0f))
        return "encode peak luminance must be finite and in (0, 10000] nits";
    return nullptr;
}

inline size_t encodePixelBytes(uint32_t format)
{
    return format == KAJO_ENCODE_RGBA16 || format == KAJO_ENCODE_RGBA16F ? 8 : 4;
}

// T64 of the definition
inline double encodeT64(uint32_t transfer, double peakNits, double y)
{
    if (transfer == KAJO_TRANSFER_GAMMA22)
        return std::pow(y, 1.0 / 2.2);
    if (transfer == KAJO_TRANSFER_SRGB)
        return y <= 0.0031308 ? 12.92 * y : 1.055 * std::pow(y, 1.0 / 2.4) - 0.055;
    if (transfer == KAJO_TRANSFER_PQ) {
        const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
        const double lp = std::pow(y * peakNits / 10000.0, m1);
        return std::pow((c1 + c2 * lp) / (1.0 + c3 * lp), m2);
    }
    return y;
}

// The table of a tabulated transfer: kEncodeTableWords floats, the layout of encode_math.h
inline void encodeTable(uint32_t transfer, float peakNits, float* words)
{
    const double peak = (double)peakNits;
    double y0 = (double)encodeFloat(kEncodeBase << (23 - kEncodeLog2E)), t0 = encodeT64(transfer, peak, y0);
    const double low = y0, tLow = t0;
    for (int i = 0; i < kEncodeKnots; i++) {
        const double y1 = (double)encodeFloat((kEncodeBase + (uint32_t)i + 1u) << (23 - kEncodeLog2E)), t1 = encodeT64(transfer, peak, y1);
        words[2 * i] = (float)t0;
        words[2 * i + 1] = (float)((t1 - t0) / (y1 - y0));
        y0 = y1;
        t0 = t1;
    }
    words[2 * kEncodeKnots] = (float)t0;
    words[2 * kEncodeKnots + 1] = (float)(tLow / low);
}

// The definition over n pixels of means (EncodeArgs::passes is 1: the division leaves a mean as it is). table: the transfer's, not read
// where the format or the transfer needs none. out: n words of encodePixelBytes(a.format); written with memcpy, so any alignment will do.
inline void encodePixels(const EncodeArgs& a, const float* table, const float* meanRgb, int64_t n, int32_t x0, int32_t y0, int32_t rowWidth, void* out)
{
    const size_t bytes = encodePixelBytes(a.format);
    char* o = static_cast<char*>(out);
    for (int64_t i = 0; i < n; i++) {
        const uint32_t px = (uint32_t)x0 + (uint32_t)(i % rowWidth), py = (uint32_t)y0 + (uint32_t)(i / rowWidth);
        const uint64_t w = encodePixel(a, table, meanRgb[3 * i], meanRgb[3 * i + 1], meanRgb[3 * i + 2], px, py);
        std::memcpy(o + (size_t)i * bytes, &w, bytes); // (little-endian: a 4-byte format's word is the low half)
    }
}

} // namespace kajo
