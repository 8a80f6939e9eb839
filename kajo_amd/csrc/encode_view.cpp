// encode_view.cpp -- the float view: crop, zoom and supersampled output between the tone curve and the transfer of the encode
// (kajo_hip_encode_view, kajo_hip_encode_view_present and its gathered twin; the definition is in include/kajo_hip.h "The float view").
// HIP source in a .cpp file, as encode.cpp. Build: hipcc -x hip --offload-arch=gfx950 -O3 -ffp-contract=off, once, in every numerics build
// alike: the arithmetic is encode_math.h's, the weight rows are the view's own (view_weights.h, tap-major on the device as view.hip reads
// them), so only the stage's input depends on FAST / EXACT / STRICT. The device evaluates no pow, exp or log.
//
// Two kernels on the caller's stream, workgroups of 256 lanes = 64 x 4:
//   kajo_encode_view_rows     the front (mean, exposure, curve: encodeFront) and the horizontal pass. A workgroup is 64 output columns by
//            4 source rows, over only the source rows the vertical pass reads. It finds its columns' source span [min first, max(first +
//            count)) (one LDS word pair per column, every lane reads all 64: broadcasts), then walks the span in ASCENDING chunks of
//            kChunk = 256 source pixels of its 4 rows: the 256 lanes evaluate the front ONCE per source pixel of the chunk (tile buffers
//            through TileMap, or a row-major frame: one global_load_dwordx4, neighbouring lanes neighbouring pixels) into LDS as separate
//            r, g, b planes [4][kChunk]; then lane (column i, row y) adds the taps of its row that fall in the chunk, in increasing j.
//            Ascending chunks with the accumulators kept in registers are the definition's order of the sum; staging keeps Lanczos's
//            12-odd taps from evaluating ACES's or Reinhard's division 12 times. A plane is read at word first[i] + k - chunk: the 64
//            lanes of a wave (one row) read words `scale` apart: a 2-way bank conflict at minification 2, more at larger integer scales,
//            none at magnification; separate planes keep that stride at one word a pixel and not three.
//            T[y][i] = float4 (.w = 0), row-major outW x rows.
//   kajo_encode_view_columns  the vertical pass, the clamp, the back (transfer, dither, quantise or half: encodeBack) and the store. One
//            lane per output pixel, a wave is one output row: first, count and the weights are at wave-uniform addresses (readfirstlane
//            makes that visible to the compiler) and go through the scalar cache; a tap's T is one coalesced 1 KiB load a wave. The
//            transfer's table (32776 bytes) is staged in LDS once per workgroup, with a grid-stride over 64x4 blocks of the OUTPUT as
//            kajo_encode has over the frame; LINEAR and the half format stage none. A pixel takes one global_store_dword or, for the
//            8-byte formats, one global_store_dwordx2. The dither runs over output coordinates.
// No atomics, no division by anything but the pass count, no order between workgroups: a word depends on the inputs through image
// coordinates only, so the image is the same for any number of tile owners. LDS: rows 12800 bytes, columns 32776 bytes.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "encode_math.h"
#include "render_args.h"

namespace
{

constexpr unsigned kMaxGroups = 1024; // of `columns`: four workgroups for each of 256 compute units, as kajo_encode
constexpr int kChunk = 256;           // source pixels of a row staged at a time: 3 planes x 4 rows x 256 floats = 12 KiB

__device__ inline float4 sourcePixel(const float4* src, const TileMap& map, int fromTiles, int x, int y)
{
    if (fromTiles) {
        int owner;
        uint32_t slot;
        kajoTileSlot(map, x, y, &owner, &slot);
        return src[(size_t)owner * map.slotsPerOwner + slot];
    }
    return src[(size_t)y * map.W + x];
}

} // namespace

extern "C" __global__ void __launch_bounds__(256) kajo_encode_view_rows(const float4* __restrict__ src, TileMap map, int fromTiles, kajo::EncodeArgs a,
                                                                         const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                                         const float* __restrict__ wxT, int outW, int row0, int rows, int blocksX,
                                                                         float4* __restrict__ T)
{
    __shared__ float plane[3][4][kChunk];
    __shared__ int32_t sFirst[64], sEnd[64];
    const int tid = (int)threadIdx.x, tx = tid & 63, ty = tid >> 6;
    // (a one-dimensional grid: a tall source has more groups of four rows than a grid's y extent holds)
    const int bx = (int)(blockIdx.x % (unsigned)blocksX), by = (int)(blockIdx.x / (unsigned)blocksX);
    const int i = bx * 64 + tx, r = by * 4 + ty;
    const bool column = i < outW;
    const int f = column ? first[i] : 0, n = column ? count[i] : 0;
    if (ty == 0) {
        // (a column past the image's edge repeats the last one's span: it widens nothing)
        const int last = outW - 1;
        sFirst[tx] = column ? f : first[last];
        sEnd[tx] = column ? f + n : first[last] + count[last];
    }
    __syncthreads();
    int lo = sFirst[0], hi = sEnd[0];
    for (int k = 1; k < 64; k++) {
        lo = min(lo, sFirst[k]);
        hi = max(hi, sEnd[k]);
    }
    const bool live = column && r < rows;
    const float* wcol = wxT + i;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    for (int c0 = lo; c0 < hi; c0 += kChunk) {
        const int width = min(kChunk, hi - c0);
        // the front, once per source pixel of the chunk: lane t takes pixels t, t + 256, ... of the 4 x width block, row by row
        for (int p = tid; p < 4 * kChunk; p += 256) {
            const int py = p / kChunk, px = p % kChunk;
            const int sr = by * 4 + py;
            if (px < width && sr < rows) {
                const float4 F = sourcePixel(src, map, fromTiles, c0 + px, row0 + sr);
                float L[3];
                kajo::encodeFront(a, F.x, F.y, F.z, L);
                plane[0][py][px] = L[0];
                plane[1][py][px] = L[1];
                plane[2][py][px] = L[2];
            }
        }
        __syncthreads();
        if (live) {
            const int j0 = max(f, c0), j1 = min(f + n, c0 + width);
            for (int j = j0; j < j1; j++) {
                const float w = wcol[(size_t)(j - f) * outW];
                ar = ar + w * plane[0][ty][j - c0];
                ag = ag + w * plane[1][ty][j - c0];
                ab = ab + w * plane[2][ty][j - c0];
            }
        }
        __syncthreads();
    }
    if (live)
        T[(size_t)r * outW + i] = make_float4(ar, ag, ab, 0.0f);
}

extern "C" __global__ void __launch_bounds__(256) kajo_encode_view_columns(const float4* __restrict__ T, kajo::EncodeArgs a,
                                                                            const float2* __restrict__ table, const int32_t* __restrict__ first,
                                                                            const int32_t* __restrict__ count, const float* __restrict__ wy, int stride,
                                                                            int outW, int outH, int row0, void* __restrict__ dst)
{
    __shared__ float2 sTable[kajo::kEncodeTableWords / 2];
    const bool tabled = a.format != kajo::kEncodeRgba16f && a.transfer != kajo::kEncodeLinear;
    if (tabled) {
        for (int k = threadIdx.x; k < kajo::kEncodeTableWords / 2; k += 256)
            sTable[k] = table[k];
        __syncthreads();
    }
    const float* table32 = reinterpret_cast<const float*>(sTable);
    const bool wide = a.format == kajo::kEncodeRgba16 || a.format == kajo::kEncodeRgba16f;
    const unsigned nbx = (unsigned)(outW + 63) / 64, nby = (unsigned)(outH + 3) / 4;
    for (unsigned b = blockIdx.x; b < nbx * nby; b += gridDim.x) {
        const int i = (int)(b % nbx) * 64 + (int)(threadIdx.x & 63);
        const int o = __builtin_amdgcn_readfirstlane((int)(b / nbx) * 4 + (int)(threadIdx.x >> 6)); // (a wave is one output row)
        if (i >= outW || o >= outH)
            continue;
        const int f = first[o], n = count[o];
        const float* w = wy + (size_t)o * stride;
        const float4* col = T + (size_t)(f - row0) * outW + i;
        float ar = 0.0f, ag = 0.0f, ab = 0.0f;
        for (int k = 0; k < n; k++) {
            const float4 t = col[(size_t)k * outW];
            const float wk = w[k];
            ar = ar + wk * t.x;
            ag = ag + wk * t.y;
            ab = ab + wk * t.z;
        }
        const float q[3] = {kajo::encodeViewClamp(a, ar), kajo::encodeViewClamp(a, ag), kajo::encodeViewClamp(a, ab)};
        const uint64_t word = kajo::encodeBack(a, table32, q, (uint32_t)i, (uint32_t)o);
        const size_t at = (size_t)o * outW + i;
        if (wide)
            static_cast<uint2*>(dst)[at] = make_uint2((uint32_t)word, (uint32_t)(word >> 32));
        else
            static_cast<uint32_t*>(dst)[at] = (uint32_t)word;
    }
}

// source pixels of a row that `rows` stages at a time (what a budget test and the notes quote)
extern "C" int kajo_encode_view_chunk(void)
{
    return kChunk;
}

// Both passes on `stream`: src (tile buffers, or with fromTiles 0 a row-major frame) -> dst (outW * outH words of 4 or 8 bytes, row-major)
// through T (float4 [outW * rows]). firstX / countX [outW], wxT [strideX][outW]; firstY / countY [outH], wy [outH][strideY]; row0 .. row0 +
// rows - 1 = the source rows any output row reads. Every tap the rows name lies inside the frame (the caller built them with
// view_weights.h, which drops the taps outside). table: as kajo_encode_launch's.
extern "C" int kajo_encode_view_launch(const void* src, const TileMap* map, int fromTiles, const kajo::EncodeArgs* a, const void* table,
                                       const void* firstX, const void* countX, const void* wxT, const void* firstY, const void* countY,
                                       const void* wy, int strideY, int outW, int outH, int row0, int rows, void* T, void* dst, void* stream)
{
    const bool tabled = a->format != kajo::kEncodeRgba16f && a->transfer != kajo::kEncodeLinear;
    if (map->W < 1 || map->H < 1 || outW < 1 || outH < 1 || row0 < 0 || rows < 1 || row0 + rows > map->H || !src || !dst || !T ||
        (tabled && !table) || a->format > kajo::kEncodeRgba16f || a->transfer > kajo::kEncodeLinear)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int blocksX = (outW + 63) / 64;
    const long long rowBlocks = (long long)blocksX * ((rows + 3) / 4);
    if (rowBlocks > 0x7fffffffll)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kajo_encode_view_rows, dim3((unsigned)rowBlocks), dim3(256), 0, st, static_cast<const float4*>(src), *map, fromTiles, *a,
                       static_cast<const int32_t*>(firstX), static_cast<const int32_t*>(countX), static_cast<const float*>(wxT), outW, row0, rows,
                       blocksX, static_cast<float4*>(T));
    const unsigned blocks = (unsigned)blocksX * (unsigned)((outH + 3) / 4);
    hipLaunchKernelGGL(kajo_encode_view_columns, dim3(blocks < kMaxGroups ? blocks : kMaxGroups), dim3(256), 0, st, static_cast<const float4*>(T), *a,
                       static_cast<const float2*>(table), static_cast<const int32_t*>(firstY), static_cast<const int32_t*>(countY),
                       static_cast<const float*>(wy), strideY, outW, outH, row0, dst);
    return (int)hipGetLastError();
}
