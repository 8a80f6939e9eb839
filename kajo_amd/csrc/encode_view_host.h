// encode_view_host.h -- the host half of the float view (include/kajo_hip.h "The float view"): the definition over a whole frame of means
// through encode_math.h and the view's own weight rows (view_weights.h), the lines encode_view.cpp compiles for the device. Pure host code
// without HIP and without the handle: present.cpp's kajo_hip_encode_view_pixels is this function behind the library's refusals, and
// tools/encode_view_san.cpp runs it under the sanitizers.
#pragma once

#include <vector>

#include "encode_host.h"
#include "view_weights.h"

namespace kajo
{

// The definition over a W x H frame of means (EncodeArgs::passes is 1: the division leaves a mean as it is). ax, ay: viewAxis of the
// rectangle over W and H. table: the transfer's, not read where the format or the transfer needs none. out: outW * outH words of
// encodePixelBytes(a.format), outW = ax's rows, outH = ay's; written with memcpy, so any alignment will do.
inline void encodeViewPixels(const EncodeArgs& a, const float* table, const float* meanRgb, int32_t W, const ViewAxis& ax, const ViewAxis& ay, void* out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int32_t outW = (int32_t)ax.first.size(), outH = (int32_t)ay.first.size();
    const int32_t row0 = ay.lo, rows = ay.hi - ay.lo;
    // the front and the horizontal pass, over the source rows the vertical pass reads: T[y - row0][i]
    std::vector<float> L((size_t)W * 3), T((size_t)rows * outW * 3);
    for (int32_t y = 0; y < rows; y++) {
        const float* line = meanRgb + (size_t)(row0 + y) * W * 3;
        for (int32_t j = ax.lo; j < ax.hi; j++)
            encodeFront(a, line[3 * j], line[3 * j + 1], line[3 * j + 2], &L[(size_t)j * 3]);
        for (int32_t i = 0; i < outW; i++) {
            const float* w = &ax.weights[(size_t)i * ax.stride];
            const int32_t f = ax.first[(size_t)i], n = ax.count[(size_t)i];
            float acc[3] = {0.0f, 0.0f, 0.0f};
            for (int32_t k = 0; k < n; k++)
                for (int c = 0; c < 3; c++)
                    acc[c] = acc[c] + w[k] * L[(size_t)(f + k) * 3 + c];
            std::memcpy(&T[((size_t)y * outW + i) * 3], acc, sizeof acc);
        }
    }
    const size_t bytes = encodePixelBytes(a.format);
    char* o = static_cast<char*>(out);
    for (int32_t oy = 0; oy < outH; oy++) {
        const float* w = &ay.weights[(size_t)oy * ay.stride];
        const int32_t f = ay.first[(size_t)oy], n = ay.count[(size_t)oy];
        for (int32_t i = 0; i < outW; i++) {
            float acc[3] = {0.0f, 0.0f, 0.0f};
            for (int32_t k = 0; k < n; k++)
                for (int c = 0; c < 3; c++)
                    acc[c] = acc[c] + w[k] * T[((size_t)(f + k - row0) * outW + i) * 3 + c];
            const float q[3] = {encodeViewClamp(a, acc[0]), encodeViewClamp(a, acc[1]), encodeViewClamp(a, acc[2])};
            const uint64_t word = encodeBack(a, table, q, (uint32_t)i, (uint32_t)oy);
            std::memcpy(o + ((size_t)oy * outW + i) * bytes, &word, bytes); // (little-endian: a 4-byte format's word is the low half)
        }
    }
}

} // namespace kajo
