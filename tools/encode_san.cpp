// encode_san.cpp -- the encode's host code (kajo_amd/csrc/encode_host.h: the bodies of kajo_hip_encode_table and kajo_hip_encode_pixels;
// encode_math.h: the lines encode.cpp compiles for the device) under AddressSanitizer + UBSan on the host: every accepted format x
// transfer x flags under the three curves over edge values -- zeros of both signs, subnormals, 2^-32 and its neighbourhood, 1.0 and its
// neighbours, the half format's boundary, values that overflow, NaN and the infinities. tests/test_encode_cpu.py builds and runs it
// and compares the checksum of the words it prints with the library's over the same inputs.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -Iinclude -Ikajo_amd/csrc tools/encode_san.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "encode_host.h"

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float values[] = {0.0f, -0.0f, 1e-45f, 1e-40f, 1.17549435e-38f, 0x1p-33f, 0x1p-32f, 1e-6f, 0.18f, 0.5f, 0.99999994f, 1.0f,
                            1.0000001f, 3.5f, 65504.0f, 65520.0f, 1e30f, 3.4e38f, -1.0f, -1e-40f, -3.4e38f, nan, inf, -inf};
    std::vector<float> mean;
    for (float r : values)
        for (float b : values) {
            mean.push_back(r);
            mean.push_back(0.25f);
            mean.push_back(b);
        }
    const int64_t n = (int64_t)(mean.size() / 3);
    struct Tone
    {
        int32_t curve;
        float exposure, white;
    };
    const Tone tones[] = {{KAJO_TONE_CLAMP, 0.0f, 0.0f}, {KAJO_TONE_REINHARD, 2.0f, 4.0f}, {KAJO_TONE_ACES, -1.0f, 0.0f}};
    uint64_t sum = 0;
    size_t words = 0, tables = 0;
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
                // (exactly the table's size, on the heap: a read or write past it is the sanitizer's to see)
                std::vector<float> table;
                if (format != KAJO_ENCODE_RGBA16F && transfer != KAJO_TRANSFER_LINEAR) {
                    table.resize(kajo::kEncodeTableWords);
                    kajo::encodeTable(transfer, p.peakNits, table.data());
                    tables++;
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
                    std::vector<unsigned char> out((size_t)n * kajo::encodePixelBytes(format));
                    kajo::encodePixels(a, table.data(), mean.data(), n, 7, 3, 5, out.data());
                    for (int64_t i = 0; i < n; i++) {
                        uint64_t w = 0;
                        std::memcpy(&w, out.data() + (size_t)i * kajo::encodePixelBytes(format), kajo::encodePixelBytes(format));
                        sum = sum * 1099511628211ull + w;
                        words++;
                    }
                }
            }
    // the refusals read nothing they should not, whatever the block holds
    KajoEncodeParams junk;
    std::memset(&junk, 0xFF, sizeof junk);
    if (!kajo::encodeRefusal(&junk) || !kajo::encodeRefusal(nullptr) || kajo::encodeHalf(65504.0f) != 0x7BFFu || kajo::encodeHalf(0x1p-25f) != 0u ||
        kajo::encodeHalf(-0.0f) != 0x8000u)
        return 1;
    std::printf("encode_san: %zu tables, %zu words, checksum %016llx: ok\n", tables, words, (unsigned long long)sum);
    return 0;
}
