// view_weights.h -- the host half of the view stage (include/kajo_hip.h "The view"): the weight rows of one axis and the two transfer
// tables, in binary64, rounded to float32 last. Pure functions of their arguments: no device, no handle, no global state. present.cpp's
// kajo_hip_view_weights / kajo_hip_view_tables and the stage's launches go through them, so what a test reads is what the kernels read.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "kajo_hip.h"

namespace kajo
{

struct ViewAxis
{
    int32_t stride = 0;         // the largest count
    int32_t lo = 0, hi = 0;     // the source pixels any row reads: lo .. hi - 1
    std::vector<int32_t> first; // [outN]
    std::vector<int32_t> count; // [outN]
    std::vector<float> weights; // [outN][stride], zeros behind a row's count
};

inline bool viewAxisValid(int32_t srcN, double a0, double a1, int32_t outN, uint32_t filter)
{
    if (srcN < 1 || outN < 1 || outN > KAJO_VIEW_MAX_OUT || filter > KAJO_VIEW_LANCZOS3)
        return false;
    if (!(std::isfinite(a0) && std::isfinite(a1) && 0.0 <= a0 && a0 < a1 && a1 <= (double)srcN))
        return false;
    return (a1 - a0) / outN <= (double)KAJO_VIEW_MAX_SCALE;
}

inline double viewSinc(double t)
{
    if (t == 0.0)
        return 1.0;
    if (t == std::floor(t))
        return 0.0; // (exactly: sin(pi t) is not 0 in binary64)
    const double a = M_PI * t;
    return std::sin(a) / a;
}

inline double viewFilter(uint32_t filter, double t)
{
    const double a = std::fabs(t);
    if (filter == KAJO_VIEW_TRIANGLE)
        return a < 1.0 ? 1.0 - a : 0.0;
    return a < 3.0 ? viewSinc(t) * viewSinc(t / 3.0) : 0.0;
}

// The rows of one axis; the arguments are viewAxisValid. false (nothing usable in *out) if a row came out longer than KAJO_VIEW_MAX_TAPS,
// which the header argues cannot happen: the caller refuses rather than resample with a row that is not the definition's
inline bool viewAxis(int32_t srcN, double a0, double a1, int32_t outN, uint32_t filter, ViewAxis* out)
{
    const double s = (a1 - a0) / outN, S = s > 1.0 ? s : 1.0;
    const double support = filter == KAJO_VIEW_TRIANGLE ? 1.0 : 3.0;
    auto inside = [srcN](double j) { return (int32_t)(j < 0.0 ? 0.0 : j > srcN - 1.0 ? srcN - 1.0 : j); };
    std::vector<std::vector<float>> rows((size_t)outN);
    out->first.assign((size_t)outN, 0);
    out->count.assign((size_t)outN, 0);
    std::vector<double> w;
    int32_t stride = 1, lo = srcN, hi = 0;
    for (int32_t i = 0; i < outN; i++) {
        const double u = a0 + (i + 0.5) * s;
        const int32_t nearest = inside(std::floor(u));
        int32_t j0 = nearest, j1 = nearest;
        w.clear();
        if (filter == KAJO_VIEW_AREA) {
            const double a = a0 + i * s, b = a0 + (i + 1) * s;
            j0 = inside(std::floor(a));
            j1 = inside(std::ceil(b) - 1.0);
            for (int32_t j = j0; j <= j1; j++) {
                const double l = a > j ? a : (double)j, r = b < j + 1.0 ? b : j + 1.0;
                w.push_back(r > l ? r - l : 0.0);
            }
        } else if (filter != KAJO_VIEW_NEAREST) {
            j0 = inside(std::ceil(u - support * S - 0.5));
            j1 = inside(std::floor(u + support * S - 0.5));
            for (int32_t j = j0; j <= j1; j++)
                w.push_back(viewFilter(filter, (j + 0.5 - u) / S));
        }
        double sum = 0.0;
        for (double x : w)
            sum += x;
        std::vector<float>& row = rows[(size_t)i];
        if (sum > 0.0)
            for (double x : w)
                row.push_back((float)(x / sum));
        // trim the float32 zeros at both ends
        size_t b = 0, e = row.size();
        while (e > b && row[e - 1] == 0.0f)
            e--;
        while (b < e && row[b] == 0.0f)
            b++;
        if ((int32_t)(e - b) > KAJO_VIEW_MAX_TAPS)
            return false;
        if (b == e) {
            // (NEAREST, and what must never be nothing)
            row.assign(1, 1.0f);
            j0 = nearest;
            b = 0;
            e = 1;
        }
        row.erase(row.begin() + (std::ptrdiff_t)e, row.end());
        row.erase(row.begin(), row.begin() + (std::ptrdiff_t)b);
        out->first[(size_t)i] = j0 + (int32_t)b;
        out->count[(size_t)i] = (int32_t)row.size();
        stride = stride > (int32_t)row.size() ? stride : (int32_t)row.size();
        lo = lo < out->first[(size_t)i] ? lo : out->first[(size_t)i];
        hi = hi > out->first[(size_t)i] + out->count[(size_t)i] ? hi : out->first[(size_t)i] + out->count[(size_t)i];
    }
    out->stride = stride;
    out->lo = lo;
    out->hi = hi;
    out->weights.assign((size_t)outN * stride, 0.0f);
    for (int32_t i = 0; i < outN; i++)
        for (size_t k = 0; k < rows[(size_t)i].size(); k++)
            out->weights[(size_t)i * stride + k] = rows[(size_t)i][k];
    return true;
}

inline void viewTables(float lin[256], float thresholds[255])
{
    for (int c = 0; c < 256; c++) {
        if (lin)
            lin[c] = (float)std::pow(c / 255.0, 2.2);
        if (thresholds && c >= 1)
            thresholds[c - 1] = (float)std::pow((c - 0.5) / 255.0, 2.2);
    }
}

} // namespace kajo
