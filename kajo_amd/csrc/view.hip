// view.hip -- the view: crop, zoom and supersampled output behind the tone curves (kajo_hip_view_argb8, kajo_hip_present_view_*; the
// definition is in include/kajo_hip.h). Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, in every numerics build alike: ARGB8
// in, ARGB8 out, so nothing here depends on FAST / EXACT / STRICT at all.
//
// The weight rows and the two transfer tables come from the host (view_weights.h); the device multiplies and adds in the definition's
// order. Two kernels on the caller's stream, workgroups of 64x4 lanes:
//   rows     one lane per (output column i, source row y): T[y][i] = sum over the column's taps of wx * lin[src[y][j]], float4 (.w = 0),
//            row-major outW x rows, only the source rows the vertical pass reads
//   columns  one lane per output pixel: v = sum over the row's taps of wy * T, then encode and one dword store
// Layouts. wx is TAP-MAJOR on the device, wxT[k * outW + i]: the 64 lanes of a wave are 64 neighbouring columns, so a tap's weights are
// one coalesced 256-byte load. While the axis's longest row has at most kViewLdsTaps = 16 taps (every AREA ratio up to 15, TRIANGLE up
// to 8, LANCZOS3 up to 2.6) the workgroup stages its 64 columns' rows in LDS as sw[k][column] -- lane l reads bank l % 32, no conflict --
// and its four waves share them; above that limit each wave reads them from global memory as it goes. wy is row-major: a wave of
// `columns` is one output row, so its weights are at wave-uniform addresses (readfirstlane makes that visible to the compiler) and go
// through the scalar cache. lin (256 floats) and the thresholds (255 + one pad) are staged in LDS, one dword per byte value: a lookup
// by byte value is a gather, its cost the number of DISTINCT values that fall on one of the 32 banks within a half wave (equal values
// broadcast). Neighbouring pixels of an image are mostly a few codes apart, which land on neighbouring banks; random words cost about
// three passes per lookup. Replicating the table per bank would take 32 KiB and 32 stores per lane to stage and was not built.
// No atomics, no cross-lane operation, no order between workgroups.
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace
{

constexpr int kViewLdsTaps = 16;

// the number of thresholds <= v: eight selects over the sorted table t[0 .. 254] (+ one pad word that is never read)
__device__ inline uint32_t viewEncode(const float* t, float v)
{
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1)
        pos += (t[pos + step - 1] <= v) ? step : 0u;
    return pos;
}

} // namespace

extern "C" __global__ __launch_bounds__(256) void kajo_view_rows(const uint32_t* __restrict__ src, int W, const float* __restrict__ linTable,
                                                      const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                      const float* __restrict__ wxT, int stride, int outW, int row0, int rows,
                                                      int blocksX, float4* __restrict__ T)
{
    __shared__ float lin[256];
    __shared__ float sw[kViewLdsTaps][64];
    const int tx = threadIdx.x, ty = threadIdx.y;
    // (a one-dimensional grid: a tall source has more groups of four rows than a grid's y extent holds)
    const int bx = blockIdx.x % blocksX, by = blockIdx.x / blocksX;
    const int i = bx * 64 + tx, r = by * 4 + ty;
    lin[ty * 64 + tx] = linTable[ty * 64 + tx];
    const bool staged = stride <= kViewLdsTaps;
    if (staged && i < outW)
        for (int k = ty; k < stride; k += 4)
            sw[k][tx] = wxT[(size_t)k * outW + i];
    __syncthreads();
    if (i >= outW || r >= rows)
        return;
    const int f = first[i], n = count[i];
    const uint32_t* line = src + (size_t)(row0 + r) * W + f;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    if (staged) {
        for (int k = 0; k < n; k++) {
            const uint32_t p = line[k];
            const float w = sw[k][tx];
            ar = ar + w * lin[(p >> 16) & 255u];
            ag = ag + w * lin[(p >> 8) & 255u];
            ab = ab + w * lin[p & 255u];
        }
    } else {
        const float* wcol = wxT + i;
        for (int k = 0; k < n; k++) {
            const uint32_t p = line[k];
            const float w = wcol[(size_t)k * outW];
            ar = ar + w * lin[(p >> 16) & 255u];
            ag = ag + w * lin[(p >> 8) & 255u];
            ab = ab + w * lin[p & 255u];
        }
    }
    T[(size_t)r * outW + i] = make_float4(ar, ag, ab, 0.0f);
}

extern "C" __global__ __launch_bounds__(256) void kajo_view_columns(const float4* __restrict__ T, const float* __restrict__ thresholds,
                                                         const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                         const float* __restrict__ wy, int stride, int outW, int outH, int row0,
                                                         uint32_t* __restrict__ dst)
{
    __shared__ float thr[256];
    const int tx = threadIdx.x, ty = threadIdx.y;
    thr[ty * 64 + tx] = thresholds[ty * 64 + tx]; // (256 words: the table is padded by one)
    __syncthreads();
    const int i = blockIdx.x * 64 + tx;
    const int o = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + ty); // (a wave is one row of the 64x4 workgroup)
    if (i >= outW || o >= outH)
        return;
    const int f = first[o], n = count[o];
    const float* w = wy + (size_t)o * stride;
    const float4* column = T + (size_t)(f - row0) * outW + i;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    for (int k = 0; k < n; k++) {
        const float4 t = column[(size_t)k * outW];
        const float wk = w[k];
        ar = ar + wk * t.x;
        ag = ag + wk * t.y;
        ab = ab + wk * t.z;
    }
    dst[(size_t)o * outW + i] = 0xff000000u | (viewEncode(thr, ar) << 16) | (viewEncode(thr, ag) << 8) | viewEncode(thr, ab);
}

// The launch limit of the LDS form of `rows` (what a budget test and the notes quote)
extern "C" int kajo_view_lds_taps(void)
{
    return kViewLdsTaps;
}

// Both passes on `stream`: src (W x H words) -> dst (outW x outH words) through T (float4 [outW * rows]). tables = lin[256] then the
// thresholds[256] (255 + one pad); firstX / countX [outW], wxT [strideX][outW]; firstY / countY [outH], wy [outH][strideY]; row0 .. row0 +
// rows - 1 = the source rows any output row reads. Every tap the rows name lies inside the image (the caller built them with
// view_weights.h, which drops the taps outside).
extern "C" int kajo_view_launch(const void* src, int W, const void* tables, const void* firstX, const void* countX, const void* wxT, int strideX,
                                const void* firstY, const void* countY, const void* wy, int strideY, int outW, int outH, int row0, int rows,
                                void* T, void* dst, void* stream)
{
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 block(64, 4);
    const float* tab = static_cast<const float*>(tables);
    const int blocksX = (outW + 63) / 64;
    const long long rowBlocks = (long long)blocksX * ((rows + 3) / 4);
    if (rowBlocks > 0x7fffffffll)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kajo_view_rows, dim3((unsigned)rowBlocks), block, 0, st, static_cast<const uint32_t*>(src), W, tab,
                       static_cast<const int32_t*>(firstX), static_cast<const int32_t*>(countX), static_cast<const float*>(wxT), strideX, outW,
                       row0, rows, blocksX, static_cast<float4*>(T));
    hipLaunchKernelGGL(kajo_view_columns, dim3((outW + 63) / 64, (outH + 3) / 4), block, 0, st, static_cast<const float4*>(T), tab + 256,
                       static_cast<const int32_t*>(firstY), static_cast<const int32_t*>(countY), static_cast<const float*>(wy), strideY, outW,
                       outH, row0, static_cast<uint32_t*>(dst));
    return (int)hipGetLastError();
}
