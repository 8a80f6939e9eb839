// grade_san.cpp -- the grade's arithmetic (kajo_amd/csrc/grade_math.h, the lines grade.hip compiles for the device) under
// AddressSanitizer + UBSan on the host: every op over edge values -- zeros of both signs, subnormals, the ends of the parameter
// ranges, values that overflow -- alone and through four chained regions. tests/test_grade_cpu.py builds and runs it; it prints a
// checksum of the results' words so that the work cannot be optimised away.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -Iinclude -Ikajo_amd/csrc tools/grade_san.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "grade_math.h"
#include "kajo_hip.h"

int main()
{
    const float values[] = {0.0f, -0.0f, 1e-45f, 1e-40f, 1.17549435e-38f, 1e-6f, 0.18f, 1.0f, 3.5f, 65536.0f, 1e30f, 3.4e38f, -1.0f, -1e-40f, -3.4e38f};
    const float slopes[] = {0.0f, 1e-40f, 1.0f, 65536.0f};
    const float offsets[] = {-65536.0f, -0.0f, 0.0f, 1e-40f, 65536.0f};
    const float powers[] = {0.125f, 1.0f, 2.2f, 8.0f};
    const float saturations[] = {0.0f, 1.0f, 4.0f};
    const float masks[] = {0.0f, 1e-40f, 0.5f, 1.0f};
    std::vector<KajoGradeOp> ops;
    for (float s : slopes)
        for (float o : offsets)
            for (float p : powers)
                for (float sat : saturations) {
                    KajoGradeOp op{};
                    for (int c = 0; c < 3; c++) {
                        op.slope[c] = s;
                        op.offset[c] = o;
                        op.power[c] = c == 1 ? 1.0f : p; // (one channel always skips the power)
                    }
                    op.saturation = sat;
                    ops.push_back(op);
                }
    uint64_t sum = 0;
    size_t n = 0;
    auto fold = [&](const float c[3]) {
        for (int i = 0; i < 3; i++) {
            uint32_t w;
            std::memcpy(&w, &c[i], 4);
            sum = sum * 1099511628211ull + w;
        }
        n++;
    };
    for (const KajoGradeOp& op : ops)
        for (float r : values)
            for (float b : values) {
                const float v[3] = {r, 0.25f, b};
                float t[3];
                kajo::gradeOp(op, v, t);
                fold(t);
            }
    for (size_t i = 0; i + 4 <= ops.size(); i += 3)
        for (float r : values)
            for (float m : masks) {
                float c[3] = {r, 0.5f, 2.0f};
                for (int k = 0; k < 4; k++)
                    kajo::gradeRegion(ops[i + k], k == 3 ? 1.0f : 0.5f, m, c);
                fold(c);
            }
    KajoGradeOp id{};
    for (int c = 0; c < 3; c++)
        id.slope[c] = id.power[c] = 1.0f;
    id.saturation = 1.0f;
    if (!kajo::gradeOpIsDefault(id) || kajo::gradeMask(3, 0.0f) != 0.0f || kajo::gradeMask(8, 16.0f) != 0.5f || kajo::gradeFinite(1.0f / 0.0f * 0.0f + __builtin_inff()))
        return 1;
    std::printf("grade_san: %zu results, checksum %016llx: ok\n", n, (unsigned long long)sum);
    return 0;
}
