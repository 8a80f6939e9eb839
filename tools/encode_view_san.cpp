// encode_view_san.cpp -- the float view's host code (kajo_amd/csrc/encode_view_host.h: the body of kajo_hip_encode_view_pixels;
// encode_math.h and view_weights.h: the lines encode_view.cpp compiles for the device and the rows it reads) under AddressSanitizer +
// UBSan on the host: every accepted format x transfer x flags under the three curves and the four filters over a 24 x 24 frame of edge
// values -- zeros of both signs, subnormals, values that overflow, NaN and the infinities -- at a fractional sub-rectangle, a
// minification and a magnification; then the largest tap rows, 4096 x 1 -> 64 x 1 and 1 x 4096 -> 1 x 64 under LANCZOS3 (384 taps).
// tests/test_encode_view_cpu.py builds and runs it and compares the checksum of the words it prints with the library's over the same inputs.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -Iinclude -Ikajo_amd/csrc tools/encode_view_san.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "encode_view_host.h"

namespace
{

uint64_t sum = 0;
size_t words = 0;

// one view of a W x H frame of means: false if an axis is refused
bool run(const kajo::EncodeArgs& a, const std::vector<float>& table, const std::vector<float>& mean, int W, int H, double x0, double y0, double x1,
         double y1, int outW, int outH, uint32_t filter)
{
    if (!kajo::viewAxisValid(W, x0, x1, outW, filter) || !kajo::viewAxisValid(H, y0, y1, outH, filter))
        return false;
    kajo::ViewAxis ax, ay;
    if (!kajo::viewAxis(W, x0, x1, outW, filter, &ax) || !kajo::viewAxis(H, y0, y1, outH, filter, &ay))
        return false;
    const size_t bytes = kajo::encodePixelBytes(a.format);
    // (exactly the image's size, on the heap: a read or write past it is the sanitizer's to see)
    std::vector<unsigned char> out((size_t)outW * outH * bytes);
    kajo::encodeViewPixels(a, table.data(), mean.data(), W, ax, ay, out.data());
    for (size_t i = 0; i < (size_t)outW * outH; i++) {
        uint64_t w = 0;
        std::memcpy(&w, out.data() + i * bytes, bytes);
        sum = sum * 1099511628211ull + w;
        words++;
    }
    return true;
}

} // namespace

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float values[] = {0.0f, -0.0f, 1e-45f, 1e-40f, 1.17549435e-38f, 0x1p-33f, 0x1p-32f, 1e-6f, 0.18f, 0.5f, 0.99999994f, 1.0f,
                            1.0000001f, 3.5f, 65504.0f, 65520.0f, 1e30f, 3.4e38f, -1.0f, -1e-40f, -3.4e38f, nan, inf, -inf};
    const int N = (int)(sizeof values / sizeof values[0]);
    std::vector<float> mean; // N x N: r by row, b by column
    for (float r : values)
        for (float b : values) {
            mean.push_back(r);
            mean.push_back(0.25f);
            mean.push_back(b);
        }
    std::vector<float> line((size_t)4096 * 3); // the edge values again and again
    for (size_t i = 0; i < 4096; i++) {
        line[3 * i] = values[i % N];
        line[3 * i + 1] = 0.25f;
        line[3 * i + 2] = values[(i / N) % N];
    }
    struct Tone
    {
        int32_t curve;
        float exposure, white;
    };
    const Tone tones[] = {{KAJO_TONE_CLAMP, 0.0f, 0.0f}, {KAJO_TONE_REINHARD, 2.0f, 4.0f}, {KAJO_TONE_ACES, -1.0f, 0.0f}};
    for (uint32_t format = 0; format < 4; format++)
        for (uint32_t transfer = 0; transfer < 4; transfer++)
            for (uint32_t flags = 0; flags < 4; flags++) {
                KajoEncodeParams p{};
                p.format = format;
                p.transfer = transfer;
                p.flags = flags;
                p.peakNits = 1000.0f;
                p.ditherSeed = 12345;
                if (kajo::encodeRefusal(&p))
                    continue;
                std::vector<float> table;
                if (format != KAJO_ENCODE_RGBA16F && transfer != KAJO_TRANSFER_LINEAR) {
                    table.resize(kajo::kEncodeTableWords);
                    kajo::encodeTable(transfer, p.peakNits, table.data());
                }
                for (const Tone& t : tones) {
                    kajo::EncodeArgs a{};
                    a.format = format;
                    a.transfer = transfer;
                    a.flags = flags;
                    a.curve = t.curve;
                    a.scale = std::exp2(t.exposure);
                    a.white = t.white;
                    a.seed = p.ditherSeed;
                    a.passes = 1.0f;
                    for (uint32_t filter = 0; filter < 4; filter++)
                        if (!run(a, table, mean, N, N, 0.25, 0.5, N - 0.25, N - 0.5, N, N, filter) || !run(a, table, mean, N, N, 0.0, 0.0, N, N, 5, 7, filter) ||
                            !run(a, table, mean, N, N, 0.0, 0.0, N, N, 2 * N + 1, 2 * N + 1, filter))
                            return 1;
                    if (!run(a, table, line, 4096, 1, 0.0, 0.0, 4096.0, 1.0, 64, 1, KAJO_VIEW_LANCZOS3) ||
                        !run(a, table, line, 1, 4096, 0.0, 0.0, 1.0, 4096.0, 1, 64, KAJO_VIEW_LANCZOS3))
                        return 1;
                }
            }
    // what the view refuses never reaches the definition
    kajo::EncodeArgs a{};
    a.passes = 1.0f;
    a.scale = 1.0f;
    if (run(a, {}, line, 4096, 1, 0.0, 0.0, 4096.0, 1.0, 63, 1, KAJO_VIEW_AREA)) // (more than 64 source pixels a pixel)
        return 1;
    std::printf("encode_view_san: %zu words, checksum %016llx: ok\n", words, (unsigned long long)sum);
    return 0;
}
