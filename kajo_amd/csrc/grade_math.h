// grade_math.h -- the arithmetic of the grade stage (include/kajo_hip.h "The grade"), host and device: one ASC CDL op on a pixel's mean
// and the blend of a region's result by its matte. grade.hip's kernels and capi.cpp's kajo_hip_grade_pixels are compiled from these
// same lines, as view.hip's numbers come from view_weights.h: what a test reads from the host is what the device computes. float32 IEEE,
// no contraction (the pragma below on the host; -ffp-contract=off for the device), in the order written; the one transcendental is
// kajo_powf (include/kajo_strictmath.h), the same bits on x86-64 and gfx950. Pure functions, no state.
#pragma once

#include <stdint.h>

#include "kajo_strictmath.h"

#if defined(__HIPCC__)
#define KGM_FN __host__ __device__ static inline
#else
#define KGM_FN static inline
#endif

namespace kajo
{

// max(t, 0) as the stage means it: 0 for a NaN (fmaxf's choice) and +0 for -0, which fmaxf leaves to the implementation
KGM_FN float gradeMax0(float t)
{
    return t > 0.0f ? t : 0.0f;
}

// the sum of the selected slots' counts over the samples: kajo_hip_matte_mask's words (matte.hip)
KGM_FN float gradeMask(uint32_t sum, float samples)
{
    return samples > 0.0f ? (float)sum / samples : 0.0f;
}

// One op on v (r, g, b), in ASC CDL order: slope, offset, power, then saturation. Op: KajoGradeOp, or anything with its four fields.
template <class Op>
KGM_FN void gradeOp(const Op& op, const float v[3], float t[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int c = 0; c < 3; c++) {
        t[c] = gradeMax0(v[c] * op.slope[c] + op.offset[c]);
        if (op.power[c] != 1.0f)
            t[c] = kajo_powf(t[c], op.power[c]);
    }
    if (op.saturation != 1.0f) {
        const float l = (0.2126f * t[0] + 0.7152f * t[1]) + 0.0722f * t[2];
        for (int c = 0; c < 3; c++)
            t[c] = l + op.saturation * (t[c] - l);
    }
}

// c = c + a (op(c) - c), a = amount * mask: a == 0 adds +-0, the pixel keeps its bits
template <class Op>
KGM_FN void gradeRegion(const Op& op, float amount, float mask, float c[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float t[3];
    gradeOp(op, c, t);
    const float a = amount * mask;
    for (int i = 0; i < 3; i++)
        c[i] = c[i] + a * (t[i] - c[i]);
}

// the op at its defaults: with no region the stage is then the identity and does no work
template <class Op>
KGM_FN bool gradeOpIsDefault(const Op& op)
{
    bool same = op.saturation == 1.0f;
    for (int c = 0; c < 3; c++)
        same = same && op.slope[c] == 1.0f && op.offset[c] == 0.0f && op.power[c] == 1.0f;
    return same;
}

KGM_FN bool gradeFinite(float x)
{
    return (ksm_bits32(x) & 0x7f800000u) != 0x7f800000u;
}

} // namespace kajo
