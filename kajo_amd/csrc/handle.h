// handle.h -- what the two halves of libkajo_hip.so's C ABI share: the KajoHip handle and its device buffers, the kernels' launchers and
// one numerics build's set of them, the error text of kajo_hip_last_error, and the preamble of every image output (the device bound,
// something rendered, the image to read). capi.cpp: create (its steps), the list of what accumulates, render (its steps), compose, the
// readers, noise, adaptive sampling, the known-answer entry points, the counters. present.cpp: the display stages and their chain.
// launch_plan.h: create's refusals, the frame plan (the handle's base), the LDS plan, the cut of the passes and the launch shape, without
// HIP. Private to those two files; inline functions, no symbols.
#ifndef KAJO_HANDLE_H
#define KAJO_HANDLE_H

#include "kajo_hip.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "render_args.h"
#include "stage.h"
#include "launch_order.h"
#include "launch_plan.h"
#include "view_weights.h"
#include "grade_math.h"
#include "adapt_math.h"
#include "checkpoint_host.h"

// launchers defined next to their kernels (kernel_fast.hip, kernel_strict.hip, kernel_exact.hip, aux_kernels.hip)
extern "C" {
int kajo_render_exact_launch(const RenderArgs*, int coldInLds, unsigned grid, unsigned block, size_t lds, void* stream);
int kajo_render_exact_split_launch(const RenderArgs*, unsigned grid, unsigned block, size_t lds, void* stream);
int kajo_render_exact_set_lds(int coldInLds, size_t lds);
int kajo_kat_shade_exact_launch(const RenderArgs*, unsigned grid, size_t lds, void* stream);
int kajo_render_fast_launch(const RenderArgs*, int coldInLds, unsigned grid, unsigned block, size_t lds, void* stream);
int kajo_render_strict_launch(const RenderArgs*, int coldInLds, unsigned grid, unsigned block, size_t lds, void* stream);
int kajo_render_fast_split_launch(const RenderArgs*, unsigned grid, unsigned block, size_t lds, void* stream);
int kajo_render_strict_split_launch(const RenderArgs*, unsigned grid, unsigned block, size_t lds, void* stream);
int kajo_render_fast_set_lds(int coldInLds, size_t lds);
int kajo_render_strict_set_lds(int coldInLds, size_t lds);
int kajo_resolve_fast_launch(const void* frame, int count, float passes, void* dst, void* stream);
int kajo_resolve_strict_launch(const void* frame, int count, float passes, void* dst, void* stream);
int kajo_resolve_tiles_fast_launch(const void* gathered, const TileMap* map, float passes, void* dst, void* stream);
int kajo_resolve_tiles_strict_launch(const void* gathered, const TileMap* map, float passes, void* dst, void* stream);
int kajo_compose_launch(const void* gathered, const TileMap* map, void* frame, void* stream);
int kajo_fold_parts_launch(void* tiles, const void* side, uint32_t sideStride, const uint32_t* blocks, unsigned count, unsigned threads, int parts, void* stream);
int kajo_kat_shade_fast_launch(const RenderArgs*, unsigned grid, size_t lds, void* stream);
int kajo_kat_shade_strict_launch(const RenderArgs*, unsigned grid, size_t lds, void* stream);
int kajo_kat_trace_fast_launch(const KatTraceArgs*, unsigned grid, size_t lds, void* stream);
int kajo_kat_trace_strict_launch(const KatTraceArgs*, unsigned grid, size_t lds, void* stream);
int kajo_kat_math_launch(int fn, int n, const void* x, const void* y, void* out, void* stream);
int kajo_kat_math_sweep_launch(int fn, float y, void* partial, void* stream); // 512 * 64 workgroups, a pair of 64-bit words each
int kajo_aov_fast_launch(const AovArgs*, int instance, unsigned grid, size_t lds, void* stream);
int kajo_aov_strict_launch(const AovArgs*, int instance, unsigned grid, size_t lds, void* stream);
int kajo_aov_fast_set_lds(int instance, size_t lds);
int kajo_aov_strict_set_lds(int instance, size_t lds);
int kajo_denoise_launch(const void* src, const TileMap* map, int fromTiles, const void* albedoHits, const void* normalDepth, float passes,
                        float samples, int iterations, int demodulate, float sigmaLuminance, float sigmaNormal, float sigmaDepth, void* scratch, void** result,
                        void* stream);
int kajo_denoise_guided_launch(const void* src, const TileMap* map, int fromTiles, const void* albedoHits, const void* normalDepth, float passes,
                               float samples, int iterations, int demodulate, float sigmaLuminance, float sigmaNormal, float sigmaDepth,
                               const void* records, const void* mean, const void* stdError, void* scratch, void** result, void* stream);
int kajo_glare_plan(int W, int H, int levels, size_t* pixels);
int kajo_glare_launch(const void* src, const TileMap* map, int fromTiles, float passes, int n, float strength, float threshold, void* scratch,
                      void* out, void* stream);
int kajo_despeckle_groups(int W, int H);
int kajo_despeckle_launch(const void* src, const TileMap* map, int fromTiles, float passes, float factor, int rank, float floorL, void* clamped,
                          void* out, int toTiles, void* partials, void* counts, void* stream);
int kajo_meter_groups(int W, int H);
int kajo_meter_launch(const void* src, const TileMap* map, int fromTiles, float passes, void* partials, void* result, void* stream);
size_t kajo_local_plane(int W, int H);
int kajo_local_launch(const void* src, const TileMap* map, int fromTiles, float passes, int iterations, float compression, float detail,
                      float sigmaRange, float pivot, void* planes, void* out, void* stream);
size_t kajo_lens_plane(int W, int H);
int kajo_lens_coc_launch(const TileMap* map, const void* albedoHits, const void* normalDepth, float aperture, float focusDistance, int maxRadius,
                         void* scratch, void* stream);
int kajo_lens_launch(const void* src, const TileMap* map, int fromTiles, float passes, const void* albedoHits, const void* normalDepth,
                     float aperture, float focusDistance, int maxRadius, void* scratch, void* out, void* stream);
int kajo_view_launch(const void* src, int W, const void* tables, const void* firstX, const void* countX, const void* wxT, int strideX,
                     const void* firstY, const void* countY, const void* wy, int strideY, int outW, int outH, int row0, int rows, void* T, void* dst,
                     void* stream);
size_t kajo_grade_block_bytes(void);
int kajo_grade_launch(const void* src, const TileMap* map, int fromTiles, float passes, const void* block, int nRegions, const void* ids,
                      const void* counts, unsigned words, unsigned nObjects, float samples, void* out, void* stream);
int kajo_compose_aov_launch(const void* gatheredAov, const void* gatheredMatte, const TileMap* map, void* aov, void* matte, void* stream);
int kajo_matte_rank_launch(const void* ids, const void* counts, int W, int H, void* rankedIds, void* rankedCounts, void* stream);
int kajo_matte_mask_launch(const void* ids, const void* counts, int W, int H, const void* selected, unsigned nObjects, float samples, void* mask,
                           void* dominant, void* stream);
int kajo_tone_fast_launch(const void* src, const TileMap* map, int fromTiles, float passes, const ToneArgs* t, void* scratch, void* dst, void* stream);
int kajo_tone_strict_launch(const void* src, const TileMap* map, int fromTiles, float passes, const ToneArgs* t, void* scratch, void* dst, void* stream);
// checkpoint_kernels.cpp: a plane between the handle's layout and canonical order (parts arrays of elems pieces of vecs 16-byte vectors), its digest
int kajo_ckpt_pack_launch(const void* src, const KajoCkptGeom* g, const void* prefix, uint32_t pixels, uint32_t parts, uint32_t vecs, uint32_t elems,
                          int tiled, void* staged, void* stream);
int kajo_ckpt_unpack_launch(const void* staged, const KajoCkptGeom* g, const void* prefix, uint32_t parts, uint32_t vecs, uint32_t elems, int tiled,
                            void* dst, void* stream);
unsigned kajo_ckpt_digest_groups(uint32_t pixels);
int kajo_ckpt_digest_launch(const void* staged, const KajoCkptGeom* g, const void* prefix, uint32_t pixels, uint32_t vecs, void* partials, void* out,
                            void* stream);
}

static_assert(KAJO_TONE_CLAMP == KAJO_TONE_CURVE_CLAMP && KAJO_TONE_REINHARD == KAJO_TONE_CURVE_REINHARD && KAJO_TONE_ACES == KAJO_TONE_CURVE_ACES,
              "tonemap.inc.hip numbers the curves as include/kajo_hip.h does");

// One numerics build's launchers
struct KernelSet
{
    int (*render)(const RenderArgs*, int coldInLds, unsigned grid, unsigned block, size_t lds, void* stream);
    int (*split)(const RenderArgs*, unsigned grid, unsigned block, size_t lds, void* stream);
    int (*setLds)(int coldInLds, size_t lds);
    int (*resolve)(const void* frame, int count, float passes, void* dst, void* stream);
    int (*resolveTiles)(const void* gathered, const TileMap* map, float passes, void* dst, void* stream);
    int (*tone)(const void* src, const TileMap* map, int fromTiles, float passes, const ToneArgs* t, void* scratch, void* dst, void* stream);
    int (*aov)(const AovArgs*, int instance, unsigned grid, size_t lds, void* stream);
    int (*aovSetLds)(int instance, size_t lds);
    int (*katTrace)(const KatTraceArgs*, unsigned grid, size_t lds, void* stream);
    int (*katShade)(const RenderArgs*, unsigned grid, size_t lds, void* stream);
    const char* aovNames[KAJO_AOV_INSTANCES]; // kajo_hip_aov_kernel: the five scene classes, with _spec, with _matte, with both
};

// the three builds' sets (capi.cpp; kajo_hip_create picks one)
extern const KernelSet kFastKernels, kStrictKernels, kExactKernels;

// the text of kajo_hip_last_error: one per thread, defined in capi.cpp
extern thread_local std::string g_error;

inline int fail(int code, const std::string& what)
{
    g_error = what;
    return code;
}

inline int failHip(hipError_t e, const char* what)
{
    return fail(KAJO_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            return failHip(e_, #expr);                                                                                 \
    } while (0)

// A device allocation, freed with its owner (KajoHip's members: by destroy(), with the handle's device current)
struct DeviceBuffer
{
    void* p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p) { o.p = nullptr; }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { reset(); }
    void reset()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(size_t bytes)
    {
        reset();
        return hipMalloc(&p, bytes ? bytes : 1);
    }
    // allocated on first need, kept after
    hipError_t ensure(size_t bytes) { return p ? hipSuccess : alloc(bytes); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    explicit operator bool() const { return p != nullptr; }
};

// (KajoFramePlan, launch_plan.h: the tile map and the owner's share of it, the launch grid, what every launch has in common)
struct KajoHip : KajoFramePlan
{
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    int W = 0, H = 0;
    KajoParams params{};
    Numerics numerics = Numerics::Fast;
    const KernelSet* k = &kFastKernels; // the launchers of that build
    kajo::StagedScene staged;
    DSceneView view{};
    std::vector<DeviceBuffer> sceneBuffers;
    KajoLdsPlan lds; // launch_plan.h
    DeviceBuffer tiles; // float4[slotsPerOwner]
    DeviceBuffer frame; // float4[W*H], lazily
    DeviceBuffer argb;  // uint32[W*H], lazily
    bool frameValid = false;
    DeviceBuffer counters; // unsigned long long [32]: [4] work counters, then the block profile of diagnostic builds
    // launch-order feedback (render_args.h): per-wave loop trips of the last launch, block order for the next
    DeviceBuffer waveTrips;  // uint32 [grid * wavesPerBlock]
    DeviceBuffer blockOrder; // uint32 [grid]
    bool orderValid = false, tripsPending = false;
    // launch tail (updateBlockOrder / partTheTail): the cost-sorted order on the host, how many of its last (cheapest) blocks are rendered in
    // parts, those blocks, and per number of parts G = 2 .. 8 the order with each of them expanded into G workgroups (built on first use)
    std::vector<uint32_t> hostOrder;
    DeviceBuffer partedOrder[kMaxParts + 1]; // uint32 [gridBlocks + (G - 1) * nParted]
    DeviceBuffer partedBlocks;               // uint32 [nParted]
    unsigned nParted = 0;
    DeviceBuffer side;         // float4 [kMaxParts - 1][nParted * block threads]: the later parts' group sums of one launch
    // FAST / EXACT, small scenes (render_args.h): a launch that ends inside a group of four passes leaves the group so far and the total of
    // the complete groups here
    DeviceBuffer carry;          // float4 [2][slotsPerOwner], on first need
    bool carryValid = false;     // ... and they are those of passesDone
    int waveSlots = 0;           // waves the chip holds at once with this handle's kernel (updateBlockOrder)
    unsigned lastTailGroups = 0; // KajoCounters.tailGroups
    int passesDone = 0;
    // what every launch's arguments have in common, filled at create (kajo_hip_render sets the passes, the order and the carry)
    RenderArgs renderArgs{};
    AovArgs aovArgs{};
    unsigned aovGrid = 0; // workgroups of an AOV launch: four 8x8 pixel blocks each
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending; // kernel timing
    std::vector<hipEvent_t> eventPool;
    double kernelMs = 0.0;
    uint64_t launches = 0;
    // first-hit AOVs (KAJO_FLAG_AOV; aov.inc.hip): float4 [2][W * H], albedo + hits then normal + depth, row-major; the passes summed into them
    DeviceBuffer aov;
    int aovInstance = KAJO_AOV_SMALL; // render_args.h KajoAovInstance: the scene class, as the render kernel is chosen
    size_t aovLds = 0;                // the instance's scene copy
    long long aovPasses = 0;
    // object-coverage mattes (KAJO_FLAG_AOV_MATTE; aov.inc.hip MATTE): uint4 [W * H][2] ids, then uint4 [W * H][2] counts, row-major; a slot with
    // count 0 is empty. Filled over the AOVs' samples (aovPasses counts them too)
    DeviceBuffer matte;
    // tiled AOVs (KAJO_FLAG_AOV_TILED): the sums and tables of the handle's OWN tiles in the accumulation's tile layout -- float4 [2][slotsPerOwner]
    // and uint4 [2][slotsPerOwner][2] -- are what the AOV kernel adds to; `aov` and `matte` above are then the composed whole frame, allocated
    // by the first kajo_hip_compose_aov and valid (aovComposed, matteComposed) until the next render or reset
    bool aovTiled = false;
    DeviceBuffer aovTiles, matteTiles;
    bool aovComposed = false, matteComposed = false;
    // the matte readers' scratch (matte.hip; kajo_hip_read_matte, kajo_hip_matte_mask), on the first call: the ranked tables int32 [W * H][8]
    // + uint32 [W * H][8], the mask and the dominant id float [2][W * H], the bitset of selected ids
    DeviceBuffer matteScratch;
    // the denoiser's scratch (denoise.hip; kajo_hip_denoise), on its first call: float4 [3][W * H] (guide, two colour frames) + uint32 [W * H]
    DeviceBuffer denoise;
    // the noise-guided denoiser's uploaded planes (denoise_guided.cpp; kajo_hip_denoise_guide_planes), on the first upload: float [2][W * H],
    // m then se of the whole frame; guideStamp: the pass count they were uploaded at, -1 = none
    DeviceBuffer guidePlanes;
    int guideStamp = -1;
    // tone mapping (tonemap.inc.hip; kajo_hip_tonemap_*), on its first call: the scale word + the logavg partials (toneLaunch)
    DeviceBuffer tone;
    // glare (glare.hip; kajo_hip_glare, kajo_hip_display_*), on its first call: the pyramid of kajo_glare_plan at the most levels, then
    // the output frame float4 [W * H]
    DeviceBuffer glare;
    // despeckle (despeckle.hip; kajo_hip_despeckle, kajo_hip_present_*), on its first call: the two counts (int64 [2]), the workgroups'
    // partial counts (despeckleImage), the clamped frame float4 [W * H] and the output frame float4 [max(W * H, slotsPerOwner)]
    DeviceBuffer despeckle;
    bool despeckled = false; // the counts are those of a despeckle (kajo_hip_despeckle_counts)
    // metering (meter.hip; kajo_hip_meter, kajo_hip_present_metered_*), on its first call: the result (the 514 bins and the count of pixels
    // that do not count, uint32 [kMeterRow], padded to 16 bytes), then the workgroups' partial histograms (meterImage)
    DeviceBuffer meter;
    // local tone mapping (local.hip; kajo_hip_local, kajo_hip_present_local_*), on its first call: three float planes of kajo_local_plane
    // (log2 luminance, the two of the ping-pong), then the output frame float4 [W * H]
    DeviceBuffer local;
    bool localRun = false; // localPivot is that of a run of the stage (kajo_hip_local_pivot)
    float localPivot = 0.0f;
    // depth of field (lens.hip; kajo_hip_lens, kajo_hip_lens_coc, kajo_hip_present_lens_argb8), on its first call: two float planes of
    // kajo_lens_plane (r, z), the tap records float4 [W * H], then the output frame float4 [W * H]
    DeviceBuffer lens;
    // the view (view.hip; kajo_hip_view_argb8, kajo_hip_present_view_*), on its first call and grown when a larger view asks: the tables
    // and the weight rows of both axes in one block (viewImage's layout), uploaded from the pinned block `viewStaging` only when the
    // parameters differ from `viewLast`; the intermediate T; an ARGB8 frame W x H for the chain's image; one outW x outH for the output
    DeviceBuffer viewRows, viewMid, viewIn, viewOut;
    size_t viewRowsBytes = 0, viewMidBytes = 0, viewOutBytes = 0, viewStagingBytes = 0;
    void* viewStaging = nullptr;
    hipEvent_t viewUploaded = nullptr; // the last upload has left viewStaging
    bool viewPlanned = false;
    KajoViewParams viewLast{};
    struct
    {
        size_t firstX, countX, wx, firstY, countY, wy; // byte offsets into viewRows (the tables are at 0)
        int strideX, strideY, row0, rows;
    } viewPlan{};
    // the grade (grade.hip; kajo_hip_grade, kajo_hip_present_grade_*), on its first call: the output frame float4 [W * H]; the parameter
    // block (five ops and the regions' amounts) with the regions' id bitsets behind it, uploaded from the pinned block `gradeStaging`
    // only when the parameters differ from `gradeLast`
    DeviceBuffer grade, gradeBlock;
    void* gradeStaging = nullptr;
    hipEvent_t gradeUploaded = nullptr; // the last upload has left gradeStaging
    bool gradePlanned = false;
    KajoGradeParams gradeLast{};
    // the encode (encode.cpp; kajo_hip_encode, kajo_hip_encode_present and its gathered twin), on its first call: the image for the host
    // (grown when a wider format asks); the transfer's table, uploaded from the pinned block `encodeStaging` only when the transfer or
    // the peak luminance differ from the last upload's
    DeviceBuffer encodeOut, encodeTable;
    size_t encodeOutBytes = 0;
    void* encodeStaging = nullptr;
    hipEvent_t encodeUploaded = nullptr; // the last upload has left encodeStaging
    bool encodePlanned = false;
    uint32_t encodeTransfer = 0;
    float encodePeak = 0.0f;
    // the noise estimate (the handle's `noise`; noise.hip), at create: the baseline float4 [slotsPerOwner] and the moment records
    // KajoNoiseMoments [slotsPerOwner] of the handle's own tile buffer; noiseRebase: the baseline is to be taken from the buffer at the next
    // batch boundary, whose batch does not count (kajo_hip_set_pass_count). noiseOut, on the first kajo_hip_noise: four planes of W * H
    // words (m, se, rel, n), then the histogram; noiseStaged, on the first kajo_hip_noise of an owner of part of the frame: the planes as
    // the device wrote them, on the host, of which the owner's pixels are copied out
    bool noise = false, noiseRebase = false;
    DeviceBuffer noiseBase, noiseMoments, noiseOut;
    std::vector<uint32_t> noiseStaged;
    // adaptive sampling (KAJO_FLAG_ADAPTIVE; adapt_kernels.cpp), at create: a state word per unit (launch block) on the device and, pinned, on
    // the host; the in-image pixels of every unit. adaptSet: kajo_hip_set_adaptive has given the rule. Once a unit has retired
    // (adaptRetired > 0) the launches take their order from adaptUnits (the handle's order without the retired units) or, the SPLIT
    // kernels, adaptBlocks (their pixel blocks); adaptOut, on the first kajo_hip_adapt_passes: the plane
    bool adaptive = false, adaptSet = false;
    KajoAdaptParams adaptParams{};
    DeviceBuffer adaptStateDev, adaptUnits, adaptBlocks, adaptOut;
    uint32_t* adaptStateHost = nullptr; // [gridBlocks], pinned
    std::vector<uint32_t> adaptUnitPixels, adaptStaged;
    unsigned adaptRetired = 0;
    long long adaptPixels = 0, adaptActivePixels = 0, adaptPaths = 0;
    int adaptLastDecision = 0;
    // checkpoints (checkpoint.cpp; kajo_hip_checkpoint_*, kajo_hip_digest): the hash of the scene create() was given; on the first call the
    // staging buffer of one plane in canonical order, sized for the widest the handle can keep and reused plane by plane, the owner's
    // prefix table (checkpoint_math.h) and the digests with the workgroups' partial sums behind them
    uint64_t sceneHash = 0;
    DeviceBuffer ckptStaging, ckptPrefix, ckptSums;
    std::vector<uint32_t> ckptPrefixHost; // [tilesY + 1]; its last word: the owner's pixels
    int toneScaleState = 0; // the s of the most recent tone mapping: 0 none yet, 1 toneScale, 2 the scale word (auto exposure)
    float toneScale = 1.0f;
};

inline int bind(KajoHip* h)
{
    HIP_TRY(hipSetDevice(h->device));
    return KAJO_OK;
}

// whole frame from this handle's own tiles (single-owner case)
inline int composeOwn(KajoHip* h)
{
    if (h->frameValid)
        return KAJO_OK;
    if (h->map.tileCount != 1)
        return fail(KAJO_E_STATE, "whole-frame output needs kajo_hip_compose() when tileCount > 1");
    HIP_TRY(h->frame.ensure((size_t)h->W * h->H * 16));
    HIP_TRY((hipError_t)kajo_compose_launch(h->tiles.p, &h->map, h->frame.p, h->stream));
    h->frameValid = true;
    return KAJO_OK;
}

// camera samples summed into the AOVs
inline long long aovSamples(const KajoHip* h)
{
    const long long n = samplesPerAxis(h->params);
    return n * n * h->aovPasses;
}

// words of the bitset of selected object ids kajo_hip_matte_mask uploads: one bit per id 0 .. nPlanes + nSpheres
inline size_t matteBitsetWords(const KajoHip* h)
{
    return ((size_t)h->staged.nPlanes + h->staged.nSpheres + 1 + 31) / 32;
}

// The whole-frame AOV sums are at hand: the refusals of their readers, `unflagged` for a handle without the AOV flag. A tiled handle
// (KAJO_FLAG_AOV_TILED) has them from kajo_hip_compose_aov until the next render or reset.
inline int aovReady(const KajoHip* h, const char* unflagged)
{
    if (!(h->params.flags & KAJO_FLAG_AOV))
        return fail(KAJO_E_STATE, unflagged);
    if (h->aovTiled && !h->aovComposed)
        return fail(KAJO_E_STATE, "a handle with tiled AOVs has the whole-frame AOVs only after kajo_hip_compose_aov() of the passes rendered so far");
    return KAJO_OK;
}

// ... and the whole-frame coverage tables
inline int matteReady(const KajoHip* h)
{
    if (!(h->params.flags & KAJO_FLAG_AOV_MATTE))
        return fail(KAJO_E_STATE, "the handle was created without the matte flag: no coverage tables to read");
    if (h->aovTiled && !h->matteComposed)
        return fail(KAJO_E_STATE, "a handle with tiled AOVs has the whole-frame coverage tables only after kajo_hip_compose_aov() with the matte tile buffers");
    return KAJO_OK;
}

// An image to resolve or tone-map: a tile buffer through h->map's geometry, or the row-major frame
struct Image
{
    const void* src;
    bool fromTiles;
};

// The preamble of the image outputs, after the caller's null checks, in the order of its refusals: the device bound, something rendered,
// and the image -- with `fromGathered` the caller's gathered tile buffers (null: this handle's own, which must be the whole frame); otherwise
// this handle's own tiles while it is the frame's one owner and no composed frame is at hand (the frame is composed when somebody asks for
// the float radiance), else the composed frame.
inline int imageOf(KajoHip* h, bool fromGathered, const void* gathered, Image* img)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (h->passesDone < 1)
        return fail(KAJO_E_STATE, "nothing rendered yet");
    if (fromGathered || (!h->frameValid && h->map.tileCount == 1)) {
        if (!gathered) {
            if (h->map.tileCount != 1)
                return fail(KAJO_E_STATE, "a handle that owns part of the frame needs the gathered tile buffers");
            gathered = h->tiles.p;
        }
        *img = Image{gathered, true};
        return KAJO_OK;
    }
    if ((rc = composeOwn(h)))
        return rc;
    *img = Image{h->frame.p, false};
    return KAJO_OK;
}

// Enqueue the display transform of the reference (the mean, clamp, 1/2.2) of an image into dst (device, ARGB8)
inline int resolve(KajoHip* h, Image img, void* dst)
{
    hipError_t le = (hipError_t)(img.fromTiles ? h->k->resolveTiles(img.src, &h->map, (float)h->passesDone, dst, h->stream)
                                               : h->k->resolve(img.src, h->W * h->H, (float)h->passesDone, dst, h->stream));
    if (le != hipSuccess)
        return failHip(le, "resolve kernel launch");
    return KAJO_OK;
}

// The bins of the meter's histogram, which the noise map's shares (include/kajo_hip.h): the float with the bits (b - 1 + base) << 19 is
// the lower edge of inner bin b, b = 1 .. 513
inline double meterEdge(int b)
{
    const uint32_t bits = (uint32_t)(b - 1 + ((127 - 16) << 4)) << 19;
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return (double)f;
}

inline double meterCentre(int b)
{
    return b >= KAJO_METER_BINS - 1 ? meterEdge(KAJO_METER_BINS - 1) : 0.5 * (meterEdge(b) + meterEdge(b + 1));
}

inline hipError_t growBuffer(DeviceBuffer& b, size_t* have, size_t want)
{
    if (b && *have >= want)
        return hipSuccess;
    *have = 0;
    hipError_t e = b.alloc(want); // (hipFree of the smaller one waits for the device: nothing in flight reads it after)
    if (e == hipSuccess)
        *have = want;
    return e;
}

#endif
