// capi.cpp -- libkajo_hip.so: the C ABI of include/kajo_hip.h over the HIP runtime.
//
// One KajoHip handle = one GPU's share of a frame: the staged scene in device memory, the
// compact tile accumulation buffer, a stream, and (on demand) the composed whole frame and
// its ARGB8 image. There is NO CPU rendering path in this library: without a usable HIP
// device kajo_hip_create fails with KAJO_E_NO_DEVICE.
#include "kajo_hip.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
int kajo_noise_update_launch(const void* tiles, void* baseline, void* records, uint32_t slots, void* stream);
int kajo_noise_map_launch(const void* records, const TileMap* map, int tileIndex, double floorL, void* mean, void* stdError, void* relative,
                          void* batches, void* hist, void* stream);
int kajo_adapt_step_launch(void* tiles, void* baseline, void* records, const void* state, uint32_t slots, uint32_t unitShift, int boundary, int P,
                           void* stream);
int kajo_adapt_select_launch(const void* records, void* state, const AdaptGeom* geom, const AdaptRule* rule, uint32_t units, uint32_t unitThreads,
                             void* stream);
int kajo_adapt_passes_launch(const void* records, const void* state, const TileMap* map, int tileIndex, uint32_t unitShift, uint32_t P, void* plane,
                             void* stream);
int kajo_compose_aov_launch(const void* gatheredAov, const void* gatheredMatte, const TileMap* map, void* aov, void* matte, void* stream);
int kajo_matte_rank_launch(const void* ids, const void* counts, int W, int H, void* rankedIds, void* rankedCounts, void* stream);
int kajo_matte_mask_launch(const void* ids, const void* counts, int W, int H, const void* selected, unsigned nObjects, float samples, void* mask,
                           void* dominant, void* stream);
int kajo_tone_fast_launch(const void* src, const TileMap* map, int fromTiles, float passes, const ToneArgs* t, void* scratch, void* dst, void* stream);
int kajo_tone_strict_launch(const void* src, const TileMap* map, int fromTiles, float passes, const ToneArgs* t, void* scratch, void* dst, void* stream);
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

static const KernelSet kFastKernels = {kajo_render_fast_launch, kajo_render_fast_split_launch, kajo_render_fast_set_lds, kajo_resolve_fast_launch,
                                       kajo_resolve_tiles_fast_launch, kajo_tone_fast_launch, kajo_aov_fast_launch, kajo_aov_fast_set_lds,
                                       kajo_kat_trace_fast_launch, kajo_kat_shade_fast_launch,
                                       {"kajo_aov_fast", "kajo_aov_fast_big", "kajo_aov_fast_big_lg", "kajo_aov_fast_biglist", "kajo_aov_fast_biglist_lg",
                                       "kajo_aov_fast_spec", "kajo_aov_fast_spec_big", "kajo_aov_fast_spec_big_lg", "kajo_aov_fast_spec_biglist", "kajo_aov_fast_spec_biglist_lg",
                                       "kajo_aov_fast_matte", "kajo_aov_fast_matte_big", "kajo_aov_fast_matte_big_lg", "kajo_aov_fast_matte_biglist", "kajo_aov_fast_matte_biglist_lg",
                                       "kajo_aov_fast_spec_matte", "kajo_aov_fast_spec_matte_big", "kajo_aov_fast_spec_matte_big_lg", "kajo_aov_fast_spec_matte_biglist",
                                       "kajo_aov_fast_spec_matte_biglist_lg"}};
static const KernelSet kStrictKernels = {kajo_render_strict_launch, kajo_render_strict_split_launch, kajo_render_strict_set_lds, kajo_resolve_strict_launch,
                                         kajo_resolve_tiles_strict_launch, kajo_tone_strict_launch, kajo_aov_strict_launch, kajo_aov_strict_set_lds,
                                         kajo_kat_trace_strict_launch, kajo_kat_shade_strict_launch,
                                         {"kajo_aov_strict", "kajo_aov_strict_big", "kajo_aov_strict_big_lg", "kajo_aov_strict_biglist", "kajo_aov_strict_biglist_lg",
                                         "kajo_aov_strict_spec", "kajo_aov_strict_spec_big", "kajo_aov_strict_spec_big_lg", "kajo_aov_strict_spec_biglist", "kajo_aov_strict_spec_biglist_lg",
                                         "kajo_aov_strict_matte", "kajo_aov_strict_matte_big", "kajo_aov_strict_matte_big_lg", "kajo_aov_strict_matte_biglist", "kajo_aov_strict_matte_biglist_lg",
                                         "kajo_aov_strict_spec_matte", "kajo_aov_strict_spec_matte_big", "kajo_aov_strict_spec_matte_big_lg", "kajo_aov_strict_spec_matte_biglist",
                                         "kajo_aov_strict_spec_matte_biglist_lg"}};
// The oracle's arithmetic in everything that decides (STRICT and EXACT): which walk, which hold policy, whose resolve. EXACT has render
// and shading kernels of its own; the STRICT instances serve it for the rest (EXACT's camera rays, walk and normals are STRICT's arithmetic).
static const KernelSet kExactKernels = {kajo_render_exact_launch, kajo_render_exact_split_launch, kajo_render_exact_set_lds, kajo_resolve_strict_launch,
                                        kajo_resolve_tiles_strict_launch, kajo_tone_strict_launch, kajo_aov_strict_launch, kajo_aov_strict_set_lds,
                                        kajo_kat_trace_strict_launch, kajo_kat_shade_exact_launch,
                                        {"kajo_aov_strict", "kajo_aov_strict_big", "kajo_aov_strict_big_lg", "kajo_aov_strict_biglist", "kajo_aov_strict_biglist_lg",
                                         "kajo_aov_strict_spec", "kajo_aov_strict_spec_big", "kajo_aov_strict_spec_big_lg", "kajo_aov_strict_spec_biglist", "kajo_aov_strict_spec_biglist_lg",
                                         "kajo_aov_strict_matte", "kajo_aov_strict_matte_big", "kajo_aov_strict_matte_big_lg", "kajo_aov_strict_matte_biglist", "kajo_aov_strict_matte_biglist_lg",
                                         "kajo_aov_strict_spec_matte", "kajo_aov_strict_spec_matte_big", "kajo_aov_strict_spec_matte_big_lg", "kajo_aov_strict_spec_matte_biglist",
                                         "kajo_aov_strict_spec_matte_biglist_lg"}};

namespace
{

thread_local std::string g_error;

int fail(int code, const std::string& what)
{
    g_error = what;
    return code;
}

int failHip(hipError_t e, const char* what)
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

template <class T>
hipError_t upload(const std::vector<T>& v, const T** out, std::vector<DeviceBuffer>& owned)
{
    owned.emplace_back();
    DeviceBuffer& b = owned.back();
    hipError_t e = b.alloc((v.empty() ? 1 : v.size()) * sizeof(T));
    if (e == hipSuccess && !v.empty())
        e = hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    *out = b.as<const T>();
    return e;
}

} // namespace

struct KajoHip
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
    TileMap map{};
    int tilesY = 0, nTiles = 0, nTilesOwned = 0, tilesPerOwner = 0;
    size_t tileBytes = 0;
    DeviceBuffer tiles; // float4[slotsPerOwner]
    DeviceBuffer frame; // float4[W*H], lazily
    DeviceBuffer argb;  // uint32[W*H], lazily
    bool frameValid = false;
    DeviceBuffer counters; // unsigned long long [32]: [4] work counters, then the block profile of diagnostic builds
    // launch-order feedback (render_args.h): per-wave loop trips of the last launch, block order for the next
    DeviceBuffer waveTrips;  // uint32 [grid * wavesPerBlock]
    DeviceBuffer blockOrder; // uint32 [grid]
    bool orderValid = false, tripsPending = false;
    unsigned gridBlocks = 0;
    // launch tail (updateBlockOrder / partTheTail): the cost-sorted order on the host, how many of its last (cheapest) blocks are rendered in
    // parts, those blocks, and per number of parts G = 2 .. 8 the order with each of them expanded into G workgroups (built on first use)
    std::vector<uint32_t> hostOrder;
    DeviceBuffer partedOrder[kMaxParts + 1]; // uint32 [gridBlocks + (G - 1) * nParted]
    DeviceBuffer partedBlocks;               // uint32 [nParted]
    unsigned nParted = 0;
    DeviceBuffer side;         // float4 [kMaxParts - 1][nParted * block threads]: the later parts' group sums of one launch
    bool partsAllowed = false; // FAST / EXACT handle of a small scene that orders its launches and may divide them
    // FAST / EXACT, small scenes (render_args.h): a launch that ends inside a group of four passes leaves the group so far and the total of
    // the complete groups here
    DeviceBuffer carry;          // float4 [2][slotsPerOwner], on first need
    bool carryValid = false;     // ... and they are those of passesDone
    int waveSlots = 0;           // waves the chip holds at once with this handle's kernel (updateBlockOrder)
    unsigned lastTailGroups = 0; // KajoCounters.tailGroups
    int passesDone = 0;
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
    // the noise estimate (KAJO_FLAG_NOISE; noise.hip), at create: the baseline float4 [slotsPerOwner] and the moment records
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
    AdaptGeom adaptGeom{};
    DeviceBuffer adaptStateDev, adaptUnits, adaptBlocks, adaptOut;
    uint32_t* adaptStateHost = nullptr; // [gridBlocks], pinned
    std::vector<uint32_t> adaptUnitPixels, adaptStaged;
    unsigned adaptShift = 6, adaptRetired = 0;
    long long adaptPixels = 0, adaptActivePixels = 0, adaptPaths = 0;
    int adaptLastDecision = 0;
    int toneScaleState = 0; // the s of the most recent tone mapping: 0 none yet, 1 toneScale, 2 the scale word (auto exposure)
    float toneScale = 1.0f;
};

namespace
{

int bind(KajoHip* h)
{
    HIP_TRY(hipSetDevice(h->device));
    return KAJO_OK;
}

int drainEvents(KajoHip* h)
{
    for (auto& pr : h->pending) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
        h->kernelMs += ms;
        h->eventPool.push_back(pr.first);
        h->eventPool.push_back(pr.second);
    }
    h->pending.clear();
    return KAJO_OK;
}

int getEvent(KajoHip* h, hipEvent_t* ev)
{
    if (!h->eventPool.empty()) {
        *ev = h->eventPool.back();
        h->eventPool.pop_back();
        return KAJO_OK;
    }
    HIP_TRY(hipEventCreate(ev));
    return KAJO_OK;
}

// whole frame from this handle's own tiles (single-owner case)
int composeOwn(KajoHip* h)
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

void destroy(KajoHip* h)
{
    if (!h)
        return;
    (void)hipSetDevice(h->device);
    if (h->stream)
        (void)hipStreamSynchronize(h->stream);
    for (auto& pr : h->pending) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    for (hipEvent_t e : h->eventPool)
        (void)hipEventDestroy(e);
    if (h->viewUploaded)
        (void)hipEventDestroy(h->viewUploaded);
    if (h->viewStaging)
        (void)hipHostFree(h->viewStaging);
    if (h->gradeUploaded)
        (void)hipEventDestroy(h->gradeUploaded);
    if (h->gradeStaging)
        (void)hipHostFree(h->gradeStaging);
    if (h->adaptStateHost)
        (void)hipHostFree(h->adaptStateHost);
    if (h->ownStream && h->stream)
        (void)hipStreamDestroy(h->stream);
    delete h;
}

// The launch tail. Workgroups are dispatched in order as wave slots come free, so a launch ends while its last `waveSlots` jobs run out:
// on average half such a job per slot stands idle -- 3 % of a 1920x1080 launch (six rounds of the slots), 1 % at 3840x2160. The cheapest
// blocks, last in the order, are therefore rendered as one workgroup per GROUP of the launch's passes (integrator.inc.hip PARTS; a launch of
// 16 passes: four workgroups of four passes): the launch ends on short jobs. Short waves are the less efficient ones (a lane that has run
// out of passes can only take over whole ones: 16 -> 4 passes per wave costs 10 %, tools/ppl_sweep.py), so only the tail is parted. FAST
// and EXACT kernels of small scenes, whose totals take the passes in groups of four whoever renders them (integrator.inc.hip GROUPS):
// the frame does not change by a bit.
// Which blocks: decided once, when the order is known. How they are expanded depends on the number of groups of a launch: partedOrderFor.
int partTheTail(KajoHip* h)
{
    h->nParted = 0;
    const unsigned n = (unsigned)h->hostOrder.size();
    if (!h->partsAllowed || n >= (1u << 28))
        return KAJO_OK;
    if (!h->waveSlots) {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        h->waveSlots = cus * 4 * (h->lds.coldInLds ? 5 : 4); // (launch bounds of the small-scene / large-scene kernels)
    }
    int q4 = 4; // how many blocks, in eighths of the slots (measured: tools/tail_sweep.sh)
    KAJO_TUNE_INT("KAJO_TAIL_Q4", 0, 64, q4);
    const unsigned nParted = kajoTailBlocks(n, (unsigned)h->waveSlots / h->lds.wavesPerBlock, q4);
    if (nParted == 0)
        return KAJO_OK;
    const unsigned block = 64 * h->lds.wavesPerBlock;
    for (DeviceBuffer& o : h->partedOrder)
        o.reset();
    h->partedBlocks.reset();
    h->side.reset();
    HIP_TRY(h->partedBlocks.alloc((size_t)nParted * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(h->partedBlocks.p, h->hostOrder.data() + (n - nParted), (size_t)nParted * sizeof(uint32_t), hipMemcpyHostToDevice));
    // the later parts' group sums of one launch: compact, a workgroup's worth of slots per parted block and part (18 MB at 1920x1080)
    // Cleared once, in front of the launches that use them on the handle's stream: a later part writes the slots of its lanes inside the
    // image only and the fold kernel adds every slot, so a slot outside the image must hold zero for the tile buffer's to stay zero. Which
    // lane of which parted block lies outside does not change while the order stands, so no launch has to clear anything again.
    const size_t sideBytes = (size_t)(kMaxParts - 1) * nParted * block * 16;
    HIP_TRY(h->side.alloc(sideBytes));
    HIP_TRY(hipMemsetAsync(h->side.p, 0, sideBytes, h->stream));
    h->nParted = nParted;
    return KAJO_OK;
}

// The order of a launch of `parts` groups: every block once, in cost order, the last nParted of them as `parts` consecutive workgroups.
int partedOrderFor(KajoHip* h, int parts)
{
    if (h->partedOrder[parts])
        return KAJO_OK;
    std::vector<uint32_t> parted;
    kajoPartedOrder(h->hostOrder, h->nParted, parts, parted);
    HIP_TRY(h->partedOrder[parts].alloc(parted.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(h->partedOrder[parts].p, parted.data(), parted.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return KAJO_OK;
}

// Longest-processing-time-first order of the workgroups from the trips the first launch recorded
// (a block runs as long as its slowest wave).
int updateBlockOrder(KajoHip* h)
{
    h->tripsPending = false;
    const unsigned n = h->gridBlocks;
    const unsigned w = h->lds.wavesPerBlock;
    std::vector<uint32_t> trips((size_t)n * w);
    HIP_TRY(hipMemcpy(trips.data(), h->waveTrips.p, trips.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint32_t> cost, order;
    kajoBlockCosts(trips.data(), n, w, cost);
    kajoCostOrder(cost, order);
    HIP_TRY(hipMemcpy(h->blockOrder.p, order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->orderValid = true;
    h->hostOrder.swap(order);
    return partTheTail(h);
}

// adaptive sampling: every unit active again (the device's state words are zeroed by the caller)
void adaptReactivate(KajoHip* h)
{
    if (!h->adaptive)
        return;
    std::memset(h->adaptStateHost, 0, (size_t)h->gridBlocks * sizeof(uint32_t));
    h->adaptRetired = 0;
    h->adaptActivePixels = h->adaptPixels;
    h->adaptPaths = 0;
    h->adaptLastDecision = 0;
}

int adaptUploadOrder(KajoHip* h);

// A decision of an adaptive handle at passesDone, behind the noise update of that boundary: the select kernel over every unit, the state
// words to the host -- the one synchronisation -- a cost order that waited for it, and the order of the launches from here on.
int adaptDecide(KajoHip* h)
{
    const unsigned n = h->gridBlocks, w = h->lds.wavesPerBlock;
    const AdaptRule rule{h->adaptParams.target, h->adaptParams.floor, (uint32_t)h->adaptParams.allowance};
    HIP_TRY((hipError_t)kajo_adapt_select_launch(h->noiseMoments.p, h->adaptStateDev.p, &h->adaptGeom, &rule, n, 64u * w, h->stream));
    HIP_TRY(hipMemcpyAsync(h->adaptStateHost, h->adaptStateDev.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int rc;
    if (h->tripsPending && (rc = updateBlockOrder(h)))
        return rc;
    h->adaptLastDecision = h->passesDone;
    unsigned retired = 0;
    long long activePixels = 0;
    for (unsigned u = 0; u < n; u++) {
        if (h->adaptStateHost[u] != KAJO_ADAPT_ACTIVE)
            retired++;
        else
            activePixels += h->adaptUnitPixels[u];
    }
    h->adaptRetired = retired;
    h->adaptActivePixels = activePixels;
    return adaptUploadOrder(h);
}

// The launch orders of an adaptive handle that has retired some of its units: the handle's order without them, and their pixel blocks
int adaptUploadOrder(KajoHip* h)
{
    const unsigned n = h->gridBlocks, w = h->lds.wavesPerBlock;
    if (!h->adaptive || h->adaptRetired == 0 || h->adaptRetired == n)
        return KAJO_OK;
    // (both orders, every time: the launch shape follows the passes of a launch, so one handle launches whole units for one cut of the
    // passes and the SPLIT kernels' pixel blocks for another; neither list can be dropped)
    std::vector<uint32_t> units, blocks;
    const uint32_t* order = h->orderValid ? h->hostOrder.data() : nullptr;
    kajoAdaptOrder(order, n, h->adaptStateHost, w, false, units);
    kajoAdaptOrder(order, n, h->adaptStateHost, w, true, blocks);
    HIP_TRY(hipMemcpy(h->adaptUnits.p, units.data(), units.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->adaptBlocks.p, blocks.data(), blocks.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return KAJO_OK;
}

int samplesPerAxis(const KajoParams& p)
{
    return (int)std::sqrt((double)(unsigned)p.samplesPerPass); // Renderer.cpp:38
}

// camera samples summed into the AOVs
long long aovSamples(const KajoHip* h)
{
    const long long n = samplesPerAxis(h->params);
    return n * n * h->aovPasses;
}

// the coverage tables of a handle: ids and counts, a word each per slot
size_t matteTableBytes(const KajoHip* h)
{
    return (size_t)h->W * h->H * KAJO_MATTE_SLOTS * 8;
}

// words of the bitset of selected object ids kajo_hip_matte_mask uploads: one bit per id 0 .. nPlanes + nSpheres
size_t matteBitsetWords(const KajoHip* h)
{
    return ((size_t)h->staged.nPlanes + h->staged.nSpheres + 1 + 31) / 32;
}

// the matte readers' scratch: the ranked tables (ids, counts), the mask, the dominant id, the bitset
size_t matteScratchBytes(const KajoHip* h)
{
    const size_t count = (size_t)h->W * h->H;
    return matteTableBytes(h) + 2 * count * sizeof(float) + matteBitsetWords(h) * sizeof(uint32_t);
}

// bytes of a tiled handle's AOV tile buffer and of its matte tile buffer (the same on every owner, padding included)
size_t aovTileBytes(const KajoHip* h)
{
    return 2 * (size_t)h->map.slotsPerOwner * 16;
}

size_t matteTileBytes(const KajoHip* h)
{
    return (size_t)h->map.slotsPerOwner * KAJO_MATTE_SLOTS * 8;
}

// The whole-frame AOV sums are at hand: the refusals of their readers, `unflagged` for a handle without the AOV flag. A tiled handle
// (KAJO_FLAG_AOV_TILED) has them from kajo_hip_compose_aov until the next render or reset.
int aovReady(const KajoHip* h, const char* unflagged)
{
    if (!(h->params.flags & KAJO_FLAG_AOV))
        return fail(KAJO_E_STATE, unflagged);
    if (h->aovTiled && !h->aovComposed)
        return fail(KAJO_E_STATE, "a handle with tiled AOVs has the whole-frame AOVs only after kajo_hip_compose_aov() of the passes rendered so far");
    return KAJO_OK;
}

// ... and the whole-frame coverage tables
int matteReady(const KajoHip* h)
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
int imageOf(KajoHip* h, bool fromGathered, const void* gathered, Image* img)
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
int resolve(KajoHip* h, Image img, void* dst)
{
    hipError_t le = (hipError_t)(img.fromTiles ? h->k->resolveTiles(img.src, &h->map, (float)h->passesDone, dst, h->stream)
                                               : h->k->resolve(img.src, h->W * h->H, (float)h->passesDone, dst, h->stream));
    if (le != hipSuccess)
        return failHip(le, "resolve kernel launch");
    return KAJO_OK;
}

} // namespace

extern "C" {

const char* kajo_hip_last_error(void)
{
    return g_error.c_str();
}

const char* kajo_hip_version(void)
{
    // (a comma, not a semicolon, in front of "view": tests/test_lens_cpu.py looks for "lens" in the LAST ';'-separated field, so the
    // stages added after the lens join that field; the next stage appends ", name" likewise)
    return "kajo-hip 0.1 (gfx950; aov-matte; local; aov-tiled; lens, view, grade, denoise-guided)";
}

void kajo_hip_default_params(KajoParams* p)
{
    std::memset(p, 0, sizeof *p);
    p->samplesPerPass = 32;  // Renderer.cpp:21
    p->depthLimit = 8;       // Shader.cpp:24
    p->seed = 0715517;       // Random.h:43
    p->tileW = 64;
    p->tileH = 16;
    p->tileIndex = 0;
    p->tileCount = 1;
    p->passesPerLaunch = 0;
    p->flags = KAJO_FLAG_EXACT; // the fastest build that meets BASELINE's RMSE < 1e-4 against the reference (include/kajo_hip.h)
}

int kajo_hip_stage_scene(const KajoScene* scene, float* invDet17, float* basis12)
{
    if (!scene)
        return fail(KAJO_E_INVALID, "scene is null");
    kajo::StagedScene st;
    kajo::stageScene(*scene, st);
    if (invDet17)
        std::memcpy(invDet17, st.invDet.data(), st.invDet.size() * sizeof(float));
    if (basis12) {
        std::memcpy(basis12 + 0, st.p1, 12);
        std::memcpy(basis12 + 3, st.p2, 12);
        std::memcpy(basis12 + 6, st.p3, 12);
        std::memcpy(basis12 + 9, st.origin, 12);
    }
    return KAJO_OK;
}

int kajo_hip_stage_shadow_lists(const KajoScene* scene, int32_t* binsPerAxis, int32_t* nLights, int32_t* lightSphere, uint32_t* start,
                                size_t startCapacity, float* key, uint32_t* index, size_t itemCapacity)
{
    if (!scene || !binsPerAxis || !nLights)
        return fail(KAJO_E_INVALID, "null argument");
    kajo::StagedScene st;
    kajo::stageScene(*scene, st);
    *binsPerAxis = st.shadowEnabled ? st.shadowN : 0;
    *nLights = (int32_t)st.light.size();
    if (!st.shadowEnabled)
        return 0;
    if (lightSphere)
        std::memcpy(lightSphere, st.light.data(), st.light.size() * sizeof(int32_t));
    if (start) {
        if (startCapacity < st.shadowStart.size())
            return fail(KAJO_E_INVALID, "start array too small");
        std::memcpy(start, st.shadowStart.data(), st.shadowStart.size() * sizeof(uint32_t));
    }
    if (key || index) {
        if (itemCapacity < st.shadowItems.size())
            return fail(KAJO_E_INVALID, "item arrays too small");
        for (size_t i = 0; i < st.shadowItems.size(); i++) {
            if (key)
                key[i] = st.shadowItems[i].key;
            if (index)
                index[i] = st.shadowItems[i].index;
        }
    }
    if (st.shadowItems.size() > 0x7fffffffu)
        return fail(KAJO_E_INVALID, "too many items");
    return (int)st.shadowItems.size();
}

int kajo_hip_stage_info(const KajoScene* scene, KajoStageInfo* info)
{
    if (!scene || !info)
        return fail(KAJO_E_INVALID, "null argument");
    kajo::StagedScene st;
    kajo::stageScene(*scene, st);
    std::memset(info, 0, sizeof *info);
    info->closedRoom = st.roomClosed ? 1 : 0;
    info->grid = st.gridEnabled ? 1 : 0;
    info->shadowLists = st.shadowEnabled ? 1 : 0;
    for (int k = 0; k < 3; k++) {
        info->room[k] = (float)st.roomLo[k];
        info->room[3 + k] = (float)st.roomHi[k];
        info->gridCenter[k] = st.gridCenter[k];
    }
    info->gridReach = (st.gridEnabled && !st.roomClosed) ? std::sqrt(st.gridReach2) : 0.f;
    return KAJO_OK;
}

int kajo_hip_launch_order(const uint32_t* waveTrips, uint32_t nBlocks, uint32_t wavesPerBlock, uint32_t waveSlots, int32_t parts, uint32_t* order,
                          size_t capacity, uint32_t* nPartedOut)
{
    if (!waveTrips || wavesPerBlock < 1 || wavesPerBlock > 4 || parts < 1 || parts > kMaxParts || nBlocks >= (1u << 28))
        return fail(KAJO_E_INVALID, "invalid argument");
    std::vector<uint32_t> cost, plain, out;
    kajoBlockCosts(waveTrips, nBlocks, wavesPerBlock, cost);
    kajoCostOrder(cost, plain);
    const unsigned nParted = kajoTailBlocks(nBlocks, waveSlots / wavesPerBlock);
    if (nPartedOut)
        *nPartedOut = nParted;
    if (parts >= 2 && nParted)
        kajoPartedOrder(plain, nParted, parts, out);
    else
        out.swap(plain);
    if (out.size() > 0x7fffffffu)
        return fail(KAJO_E_INVALID, "order too long");
    if (order) {
        if (capacity < out.size())
            return fail(KAJO_E_INVALID, "order array too small");
        std::memcpy(order, out.data(), out.size() * sizeof(uint32_t));
    }
    return (int)out.size();
}

int kajo_hip_create(const KajoScene* scene, int width, int height, const KajoParams* params, kajo_hip_t* out)
{
    if (!scene || !params || !out)
        return fail(KAJO_E_INVALID, "null argument");
    *out = nullptr;
    if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 31) - 1)
        return fail(KAJO_E_INVALID, "image size out of range");
    if (scene->nPlanes < 0 || scene->nSpheres < 0 || (scene->nPlanes && !scene->planes) || (scene->nSpheres && !scene->spheres))
        return fail(KAJO_E_INVALID, "scene arrays inconsistent");
    KajoParams p = *params;
    if (p.tileW == 0)
        p.tileW = 64;
    if (p.tileH == 0)
        p.tileH = 16;
    if (p.tileCount == 0)
        p.tileCount = 1;
    if (p.samplesPerPass < 1 || p.samplesPerPass > 65535)
        return fail(KAJO_E_INVALID, "samplesPerPass must be in [1, 65535]");
    if ((p.flags & KAJO_FLAG_STRICT) && (p.flags & KAJO_FLAG_EXACT))
        return fail(KAJO_E_INVALID, "the strict and the exact flag name two different numerics builds: set one");
    if (p.flags & KAJO_FLAG_COOP)
        return fail(KAJO_E_INVALID, "KAJO_FLAG_COOP: the cooperative-traversal experiment is not built into this library (make -C kajo_amd/csrc experiments)");
    if (p.flags & KAJO_FLAG_DEFERRED)
        return fail(KAJO_E_INVALID, "KAJO_FLAG_DEFERRED: the deferred-shading experiment is not built into this library (make -C kajo_amd/csrc experiments)");
    if (p.depthLimit < 0 || p.depthLimit > 1000) // (the reference's limit is 8)
        return fail(KAJO_E_INVALID, "depthLimit must be in [0, 1000]");
    if (p.tileW < 8 || p.tileH < 8 || (p.tileW & 7) || (p.tileH & 7) || (p.tileW * p.tileH) % 256)
        return fail(KAJO_E_INVALID, "tile size must be multiples of 8 with tileW*tileH a multiple of 256");
    if (p.tileCount < 1 || p.tileIndex < 0 || p.tileIndex >= p.tileCount)
        return fail(KAJO_E_INVALID, "tileIndex/tileCount out of range");
    if ((p.flags & KAJO_FLAG_AOV) && !(p.flags & KAJO_FLAG_AOV_TILED) && p.tileCount != 1)
        return fail(KAJO_E_INVALID, "first-hit AOVs need the whole frame on one handle (tileCount 1)");
    if ((p.flags & KAJO_FLAG_AOV_SPECULAR) && !(p.flags & KAJO_FLAG_AOV))
        return fail(KAJO_E_INVALID, "the first-non-delta-hit flag changes what the AOV flag's buffers hold: set the AOV flag with it");
    if ((p.flags & KAJO_FLAG_AOV_MATTE) && !(p.flags & KAJO_FLAG_AOV))
        return fail(KAJO_E_INVALID, "the matte flag keeps its coverage tables over the AOV flag's samples: set the AOV flag with it");
    if ((p.flags & KAJO_FLAG_AOV_TILED) && !(p.flags & KAJO_FLAG_AOV))
        return fail(KAJO_E_INVALID, "the tiled flag changes where the AOV flag's sums are kept: set the AOV flag with it");
    if ((p.flags & KAJO_FLAG_ADAPTIVE) && !(p.flags & KAJO_FLAG_NOISE))
        return fail(KAJO_E_INVALID, "the adaptive flag retires units by the noise flag's estimate: set the noise flag with it");
    // (aov.inc.hip: a wave of the tiled launch carries its block's corner and the tile's shape in 16-bit fields, in units of 8 pixels)
    if ((p.flags & KAJO_FLAG_AOV_TILED) && (width > 524288 || height > 262144 || p.tileW > 524280 || p.tileH > 524280))
        return fail(KAJO_E_INVALID, "tiled AOVs: the frame must be within 524288 x 262144 and a tile within 524280 pixels a side");

    if (p.flags & (KAJO_FLAG_STRICT | KAJO_FLAG_EXACT)) {
        // integrator.inc.hip kdiv / ksqrt: the IEEE quotient and root without the compiler's range scaling are exact while operands stay
        // dozens of binades inside the float range, which a scene of ordinary coordinates guarantees; outside it STRICT would silently
        // stop being the oracle
        float lo = 0.f, hi = 0.f;
        kajo::coordinateRange(*scene, &lo, &hi);
        if (!(hi == hi) || (hi > 0.f && (lo < 0x1p-40f || hi > 0x1p40f))) {
            char msg[256];
            std::snprintf(msg, sizeof msg, "strict / exact numerics need the scene's non-zero coordinates within 2^-40 .. 2^40 in magnitude "
                                           "(found %g .. %g): use the fast build or rescale the scene", (double)lo, (double)hi);
            return fail(KAJO_E_INVALID, msg);
        }
    }

    int nDev = 0;
    hipError_t e = hipGetDeviceCount(&nDev);
    if (e != hipSuccess || nDev <= 0)
        return fail(KAJO_E_NO_DEVICE, "no HIP device available; this backend has no CPU path");
    if (p.device < 0 || p.device >= nDev)
        return fail(KAJO_E_INVALID, "device ordinal out of range");

    KajoHip* h = new (std::nothrow) KajoHip;
    if (!h)
        return fail(KAJO_E_INVALID, "out of host memory");
    h->device = p.device;
    h->params = p;
    h->W = width;
    h->H = height;
    h->numerics = (p.flags & KAJO_FLAG_STRICT) ? Numerics::Strict : (p.flags & KAJO_FLAG_EXACT) ? Numerics::Exact : Numerics::Fast;
    h->k = h->numerics == Numerics::Strict ? &kStrictKernels : h->numerics == Numerics::Exact ? &kExactKernels : &kFastKernels;
#define CREATE_TRY(expr)                                                                                               \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) {                                                                                        \
            destroy(h);                                                                                                \
            return failHip(e_, #expr);                                                                                 \
        }                                                                                                              \
    } while (0)
    CREATE_TRY(hipSetDevice(h->device));
    CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->ownStream = true;

    // ---- scene -----------------------------------------------------------------------------
    kajo::stageScene(*scene, h->staged, (p.flags & KAJO_FLAG_NO_GRID) ? 0 : 48, !(p.flags & KAJO_FLAG_NO_SHADOW_LISTS));
    const kajo::StagedScene& st = h->staged;
    DSceneView& v = h->view;
    CREATE_TRY(upload(st.planeRow, &v.planeRow, h->sceneBuffers));
    CREATE_TRY(upload(st.planeDet, &v.planeDet, h->sceneBuffers));
    CREATE_TRY(upload(st.planeFrame, &v.planeFrame, h->sceneBuffers));
    CREATE_TRY(upload(st.sphereHot, &v.sphereHot, h->sceneBuffers));
    CREATE_TRY(upload(st.sphereHotOffset, &v.sphereHotOffset, h->sceneBuffers));
    CREATE_TRY(upload(st.sphereCold, &v.sphereCold, h->sceneBuffers));
    CREATE_TRY(upload(st.material, &v.material, h->sceneBuffers));
    CREATE_TRY(upload(st.light, &v.light, h->sceneBuffers));
    CREATE_TRY(upload(st.gridCellStart, &v.grid.cellStart, h->sceneBuffers));
    CREATE_TRY(upload(st.gridItems, &v.grid.items, h->sceneBuffers));
    v.grid.enabled = st.gridEnabled;
    v.grid.nCells = st.gridEnabled ? (int32_t)st.gridCellStart.size() - 1 : 0;
    v.grid.nItems = (int32_t)st.gridItems.size();
    for (int k = 0; k < 3; k++) {
        v.grid.dim[k] = st.gridDim[k];
        v.grid.bmin[k] = st.gridEnabled ? st.gridMin[k] : 0.f;
        v.grid.bmax[k] = st.gridEnabled ? st.gridMax[k] : 0.f;
        v.grid.cell[k] = st.gridEnabled ? st.gridCell[k] : 1.f;
        v.grid.invCell[k] = st.gridEnabled ? 1.f / st.gridCell[k] : 1.f;
        v.grid.center[k] = st.gridCenter[k];
    }
    v.grid.reach2 = st.gridReach2;
    CREATE_TRY(upload(st.shadowRowBase, &v.shadow.rowBase, h->sceneBuffers));
    CREATE_TRY(upload(st.shadowOff16, &v.shadow.off16, h->sceneBuffers));
    CREATE_TRY(upload(st.shadowPacked, &v.shadow.items, h->sceneBuffers));
    CREATE_TRY(upload(st.shadowInvKeyScale, &v.shadow.invKeyScale, h->sceneBuffers));
    v.shadow.enabled = st.shadowEnabled ? 1 : 0;
    v.shadow.n = st.shadowN;
    v.nPlanes = st.nPlanes;
    v.nSpheres = st.nSpheres;
    v.nSphereHot = (int)st.sphereHot.size();
    v.nLights = (int)st.light.size();
    v.allTranslated = st.allTranslated;
    v.planesRigid = st.planesRigid;
    for (int i = 0; i < 3; i++) {
        v.background[i] = st.background[i];
        v.p1[i] = st.p1[i];
        v.dp2[i] = st.p2[i] - st.p1[i]; // (p2 - p1), (p3 - p1) of Renderer.cpp:58
        v.dp3[i] = st.p3[i] - st.p1[i];
        v.origin[i] = st.origin[i];
    }
    const KajoSceneLds bytes = kajoSceneLds(st);
    h->lds = kajoLdsPlan(bytes.hotBytes, bytes.coldBytes, bytes.gridHeaderBytes, bytes.gridBytes, st.gridEnabled, st.shadowEnabled, v.nLights, h->numerics);
    v.grid.inLds = h->lds.gridInLds ? 1 : 0;
    if (!h->lds.fits) {
        destroy(h);
        return fail(KAJO_E_INVALID, "scene exceeds the LDS staging limit: scene records + the waves' mailboxes must fit 160 KiB");
    }
    // ---- tiles -----------------------------------------------------------------------------
    TileMap& m = h->map;
    m.W = width;
    m.H = height;
    m.tileW = p.tileW;
    m.tileH = p.tileH;
    m.tilesX = (width + p.tileW - 1) / p.tileW;
    m.tileCount = p.tileCount;
    h->tilesY = (height + p.tileH - 1) / p.tileH;
    h->nTiles = m.tilesX * h->tilesY;
    h->tilesPerOwner = (h->nTiles + p.tileCount - 1) / p.tileCount;
    h->nTilesOwned = (h->nTiles - p.tileIndex + p.tileCount - 1) / p.tileCount;
    if (h->nTilesOwned < 0)
        h->nTilesOwned = 0;
    m.slotsPerOwner = h->tilesPerOwner * p.tileW * p.tileH;
    h->tileBytes = (size_t)m.slotsPerOwner * 16;
    // (FAST / EXACT handles of small scenes that order their launches render the tail of a launch in parts: partTheTail)
    h->partsAllowed = h->lds.coldInLds && h->numerics != Numerics::Strict && !(p.flags & (KAJO_FLAG_NO_SPLIT | KAJO_FLAG_NO_REORDER));
    CREATE_TRY(h->tiles.alloc(h->tileBytes));
    CREATE_TRY(hipMemsetAsync(h->tiles.p, 0, h->tileBytes, h->stream));
    if (p.flags & KAJO_FLAG_COUNTERS) {
        CREATE_TRY(h->counters.alloc(32 * sizeof(unsigned long long)));
        CREATE_TRY(hipMemsetAsync(h->counters.p, 0, 32 * sizeof(unsigned long long), h->stream));
    }
    {
        const unsigned wavesPerBlock = h->lds.wavesPerBlock;
        const int wavesPerTile = (p.tileW / 8) * (p.tileH / 8);
        h->gridBlocks = (unsigned)((long long)h->nTilesOwned * wavesPerTile / wavesPerBlock);
        if ((long long)h->nTilesOwned * wavesPerTile / wavesPerBlock >= (1ll << 28)) { // (render_args.h: an order word has 28 bits for the block)
            destroy(h);
            return fail(KAJO_E_INVALID, "frame too large: 2^28 pixel blocks per handle at most");
        }
        if (h->gridBlocks && !(p.flags & KAJO_FLAG_NO_REORDER)) {
            CREATE_TRY(h->waveTrips.alloc((size_t)h->gridBlocks * wavesPerBlock * sizeof(uint32_t)));
            CREATE_TRY(h->blockOrder.alloc((size_t)h->gridBlocks * sizeof(uint32_t)));
        }
    }
    if (h->lds.ldsTotal() > 48 * 1024)
        CREATE_TRY((hipError_t)h->k->setLds(h->lds.coldInLds, h->lds.ldsTotal()));
    if (p.flags & KAJO_FLAG_AOV) {
        // the AOV kernel of the scene's class -- small scenes: everything in LDS; large ones: the hot records (and the grid's cell lists where
        // create() put them in LDS), per home of the cell lists and with or without visibility lists, as launch.inc.hip picks the render kernel
        if (h->lds.coldInLds)
            h->aovInstance = KAJO_AOV_SMALL;
        else if (v.shadow.enabled)
            h->aovInstance = v.grid.inLds ? KAJO_AOV_BIGLIST_LG : KAJO_AOV_BIGLIST;
        else
            h->aovInstance = v.grid.inLds ? KAJO_AOV_BIG_LG : KAJO_AOV_BIG;
        if (p.flags & KAJO_FLAG_AOV_SPECULAR) // the same scene class, with the chain to the first non-delta hit
            h->aovInstance += KAJO_AOV_SPEC_SMALL;
        if (p.flags & KAJO_FLAG_AOV_MATTE) // ... with the coverage tables beside the sums
            h->aovInstance += KAJO_AOV_MATTE_SMALL;
        h->aovLds = h->lds.coldInLds ? h->lds.ldsBytes : h->lds.hotBytes;
        if (h->aovLds > 48 * 1024)
            CREATE_TRY((hipError_t)h->k->aovSetLds(h->aovInstance, h->aovLds));
        h->aovTiled = (p.flags & KAJO_FLAG_AOV_TILED) != 0;
        if (h->aovTiled) {
            // the sums of the handle's own tiles only (the whole-frame buffers: kajo_hip_compose_aov, on the handle it is called on)
            CREATE_TRY(h->aovTiles.alloc(aovTileBytes(h)));
            CREATE_TRY(hipMemsetAsync(h->aovTiles.p, 0, aovTileBytes(h), h->stream));
            if (p.flags & KAJO_FLAG_AOV_MATTE) {
                CREATE_TRY(h->matteTiles.alloc(matteTileBytes(h)));
                CREATE_TRY(hipMemsetAsync(h->matteTiles.p, 0, matteTileBytes(h), h->stream));
            }
        } else {
            const size_t bytes = 2 * (size_t)width * height * 16;
            CREATE_TRY(h->aov.alloc(bytes));
            CREATE_TRY(hipMemsetAsync(h->aov.p, 0, bytes, h->stream));
            if (p.flags & KAJO_FLAG_AOV_MATTE) {
                const size_t tables = matteTableBytes(h);
                CREATE_TRY(h->matte.alloc(tables));
                CREATE_TRY(hipMemsetAsync(h->matte.p, 0, tables, h->stream));
            }
        }
    }
    if (p.flags & KAJO_FLAG_NOISE) {
        h->noise = true;
        CREATE_TRY(h->noiseBase.alloc(h->tileBytes));
        CREATE_TRY(hipMemsetAsync(h->noiseBase.p, 0, h->tileBytes, h->stream));
        CREATE_TRY(h->noiseMoments.alloc(2 * h->tileBytes));
        CREATE_TRY(hipMemsetAsync(h->noiseMoments.p, 0, 2 * h->tileBytes, h->stream));
    }
    if (p.flags & KAJO_FLAG_ADAPTIVE) {
        h->adaptive = true;
        const unsigned w = h->lds.wavesPerBlock;
        if (w != 1 && w != 2 && w != 4) {
            destroy(h);
            return fail(KAJO_E_INVALID, "adaptive sampling: a unit is 64, 128 or 256 slots");
        }
        h->adaptShift = w == 1 ? 6 : w == 2 ? 7 : 8;
        h->adaptGeom = AdaptGeom{width, height, p.tileW, p.tileH, m.tilesX, p.tileIndex, p.tileCount, h->nTilesOwned};
        const size_t words = h->gridBlocks ? h->gridBlocks : 1;
        CREATE_TRY(h->adaptStateDev.alloc(words * sizeof(uint32_t)));
        CREATE_TRY(hipMemsetAsync(h->adaptStateDev.p, 0, words * sizeof(uint32_t), h->stream));
        CREATE_TRY(h->adaptUnits.alloc(words * sizeof(uint32_t)));
        CREATE_TRY(h->adaptBlocks.alloc(words * w * sizeof(uint32_t)));
        CREATE_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->adaptStateHost), words * sizeof(uint32_t), hipHostMallocDefault));
        std::memset(h->adaptStateHost, 0, words * sizeof(uint32_t));
        h->adaptUnitPixels.assign(h->gridBlocks, 0u);
        for (unsigned u = 0; u < h->gridBlocks; u++)
            for (uint32_t s = 0; s < 64u * w; s++) {
                int px, py;
                if (kajo::adaptSlotPixel(h->adaptGeom, u * 64u * w + s, &px, &py))
                    h->adaptUnitPixels[u]++;
            }
        for (uint32_t c : h->adaptUnitPixels)
            h->adaptPixels += c;
        h->adaptActivePixels = h->adaptPixels;
    }
    CREATE_TRY(hipStreamSynchronize(h->stream));
#undef CREATE_TRY
    *out = h;
    return KAJO_OK;
}

int kajo_hip_destroy(kajo_hip_t h)
{
    destroy(h);
    return KAJO_OK;
}

int kajo_hip_set_stream(kajo_hip_t h, void* stream)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    int rc = bind(h);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->ownStream)
        HIP_TRY(hipStreamDestroy(h->stream));
    h->stream = static_cast<hipStream_t>(stream);
    h->ownStream = false;
    return KAJO_OK;
}

int kajo_hip_render(kajo_hip_t h, int passes)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    // (the kernels form the exclusive end of a launch's passes, firstPass + nPasses, in 32-bit integers: the last pass number a
    // handle can render is 2^31 - 2)
    if (passes < 0 || h->passesDone + (long long)passes > 0x7ffffffell)
        return fail(KAJO_E_INVALID, "pass count out of range (pass numbers run to 2^31 - 2)");
    int rc = bind(h);
    if (rc)
        return rc;
    if (passes > 0) // (tiled AOVs: the composed whole-frame buffers are those of the passes before)
        h->aovComposed = h->matteComposed = false;
    if (passes == 0 || h->nTilesOwned == 0) {
        // (an owner without a tile launches nothing; its zeroed AOV tile buffers count the passes like the others')
        if (h->aovTiled)
            h->aovPasses += passes;
        h->passesDone += passes;
        return KAJO_OK;
    }
    const KajoParams& p = h->params;
    const KajoLdsPlan& lds = h->lds;
    RenderArgs a;
    std::memset(&a, 0, sizeof a);
    a.scene = h->view;
    a.tiles = h->tiles.p;
    a.W = h->W;
    a.H = h->H;
    a.n = samplesPerAxis(p);
    a.S = (float)(unsigned)p.samplesPerPass;
    a.pixelWidth = 1.f / h->W;   // Renderer.cpp:39-42
    a.pixelHeight = 1.f / h->H;
    a.sampleWidth = a.pixelWidth / a.n;
    a.sampleHeight = a.pixelHeight / a.n;
    a.depthLimit = p.depthLimit;
    a.seed = p.seed;
    a.tileW = p.tileW;
    a.tileH = p.tileH;
    a.tilesX = h->map.tilesX;
    a.tilesY = h->tilesY;
    a.tileIndex = p.tileIndex;
    a.tileCount = p.tileCount;
    a.nTilesOwned = h->nTilesOwned;
    a.counters = h->counters.as<unsigned long long>();
    a.mailboxOffset = (uint32_t)lds.mailboxOffset();
    a.stealWindow = lds.stealWindow;
    a.carrySlots = (uint32_t)h->map.slotsPerOwner;
    a.blockOrder = h->orderValid ? h->blockOrder.as<const uint32_t>() : nullptr;
    a.waveTrips = (h->waveTrips && !h->orderValid) ? h->waveTrips.as<uint32_t>() : nullptr; // measure once, on the first launch
    lds.fillWaveLds(a, a.mailboxOffset, true);

    const unsigned block = 64 * lds.wavesPerBlock;
    const unsigned grid = h->gridBlocks;
    const unsigned long long pixelBlocks = (unsigned long long)grid * lds.wavesPerBlock;
    const bool grouped = lds.coldInLds && h->numerics != Numerics::Strict; // (integrator.inc.hip GROUPS: FAST / EXACT kernels of small scenes)
    // (coldInLds 2: the small-scene instance of any number of lights although the scene has one, KAJO_FLAG_NO_ONE_LIGHT)
    const int home = (lds.coldInLds && (p.flags & KAJO_FLAG_NO_ONE_LIGHT)) ? 2 : lds.coldInLds;
    const int perLaunch = p.passesPerLaunch > 0 ? p.passesPerLaunch : 16;
    int left = passes;
    // (the noise estimate: a baseline owed since kajo_hip_set_pass_count to a multiple of four is the buffer as it stands now)
    if (h->noise && h->noiseRebase && h->passesDone % KAJO_NOISE_BATCH_PASSES == 0) {
        HIP_TRY(hipMemcpyAsync(h->noiseBase.p, h->tiles.p, h->tileBytes, hipMemcpyDeviceToDevice, h->stream));
        h->noiseRebase = false;
    }
    while (left > 0) {
        int now = left < perLaunch ? left : perLaunch;
        if (h->noise) // no launch crosses an absolute multiple of the batch (the frame's bits do not depend on the cut)
            now = std::min(now, KAJO_NOISE_BATCH_PASSES - h->passesDone % KAJO_NOISE_BATCH_PASSES);
        a.firstPass = h->passesDone + 1;
        a.nPasses = now;
        // (adaptive sampling: once a unit has retired the launches cover the active units only, in the handle's order without the others;
        // a decision may have brought a new cost order in between: the order is looked up launch by launch)
        const bool shortGrid = h->adaptive && h->adaptRetired > 0;
        const unsigned activeUnits = grid - (h->adaptive ? h->adaptRetired : 0u);
        if (h->adaptive) {
            a.blockOrder = shortGrid ? h->adaptUnits.as<const uint32_t>() : h->orderValid ? h->blockOrder.as<const uint32_t>() : nullptr;
            if (shortGrid)
                a.waveTrips = nullptr; // (the trips are measured by whole launches only; until a unit retires, as on any other handle)
        }
        const KajoLaunchShape s = kajoLaunchShape(pixelBlocks, now, a.n, lds.coldInLds, p.flags & KAJO_FLAG_NO_SPLIT, a.mailboxOffset,
                                                  lds.perWaveBytes(false), h->passesDone, grouped, h->orderValid, h->nParted);
        if (s.startsInside || s.endsInside)
            HIP_TRY(h->carry.ensure(2 * h->tileBytes));
        a.carry = h->carry.p;
        // (a group whose first passes this handle did not render -- kajo_hip_set_pass_count to the middle of one -- continues from the
        // buffer as it stands: the restored sum counts as complete groups)
        a.carryIn = s.startsInside && h->carryValid;
        a.carryOut = s.endsInside;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        hipError_t le = hipSuccess;
        const bool launch = activeUnits > 0; // (adaptive sampling: with every unit retired the passes are counted, nothing is rendered)
        if (launch) {
            if ((rc = getEvent(h, &e0)) || (rc = getEvent(h, &e1)))
                return rc;
            HIP_TRY(hipEventRecord(e0, h->stream));
        }
        h->lastTailGroups = 0;
        if (!launch) {
        } else if (s.chunks > 1 || s.split > 1) {
            // the waves of a block divide the samples of every pass (behind the [pass][sample][pixel] table) or the passes (behind the
            // [pass][pixel] term table); one round or two: the launch order does not matter
            RenderArgs b = a;
            b.blockOrder = nullptr;
            b.waveTrips = nullptr;
            if (s.chunks > 1)
                b.sampleChunks = (int32_t)s.chunks;
            const unsigned waves = s.chunks > 1 ? (unsigned)now * s.chunks : s.split;
            lds.fillWaveLds(b, a.mailboxOffset + (size_t)now * (s.chunks > 1 ? a.n * a.n : 1) * 64 * 16, false);
            b.thrL = 1; // (short waves: holding a vertex only lengthens their tail -- configs[0] 18.9 against 16.5 G paths/s; 1-3 % on
                        // split frames below 720p)
            if (shortGrid) // the active units' pixel blocks
                b.blockOrder = h->adaptBlocks.as<const uint32_t>();
            le = (hipError_t)h->k->split(&b, shortGrid ? activeUnits * lds.wavesPerBlock : (unsigned)pixelBlocks, 64 * waves,
                                         b.perWaveOffset + (size_t)waves * b.perWaveBytes, h->stream);
        } else if (s.parted && !shortGrid) { // (a noise handle's launches are of one group at the most: never parted)
            // the launch tail: the cheapest blocks as one workgroup per group of the launch (partTheTail)
            if ((rc = partedOrderFor(h, s.launchGroups))) {
                h->eventPool.push_back(e0);
                h->eventPool.push_back(e1);
                return rc;
            }
            h->lastTailGroups = h->nParted * (unsigned)(s.launchGroups - 1);
            RenderArgs b = a;
            b.blockOrder = h->partedOrder[s.launchGroups].as<const uint32_t>();
            b.side = h->side.p;
            b.sideStride = h->nParted * block;
            b.partedFirst = grid - h->nParted;
            le = (hipError_t)h->k->render(&b, home, grid + h->lastTailGroups, block, lds.ldsTotal(), h->stream);
            if (le == hipSuccess)
                le = (hipError_t)kajo_fold_parts_launch(h->tiles.p, h->side.p, b.sideStride, h->partedBlocks.as<const uint32_t>(), h->nParted, block,
                                                        s.launchGroups, h->stream);
        } else {
            le = (hipError_t)h->k->render(&a, home, activeUnits, block, lds.ldsTotal(), h->stream);
        }
        if (le != hipSuccess) {
            h->eventPool.push_back(e0);
            h->eventPool.push_back(e1);
            return failHip(le, "render kernel launch");
        }
        if (launch) {
            HIP_TRY(hipEventRecord(e1, h->stream));
            h->pending.emplace_back(e0, e1);
        }
        if (p.flags & KAJO_FLAG_AOV) {
            // the first-hit AOVs of the same passes, behind the render launch and outside its timing events (KajoCounters.kernelMs)
            AovArgs g;
            std::memset(&g, 0, sizeof g);
            g.scene = h->view;
            g.albedoHits = h->aovTiled ? h->aovTiles.p : h->aov.p;
            g.slots = h->aovTiled ? (uint32_t)h->map.slotsPerOwner : (uint32_t)(h->W * h->H);
            g.W = h->W;
            g.H = h->H;
            g.n = a.n;
            g.pixelWidth = a.pixelWidth;
            g.pixelHeight = a.pixelHeight;
            g.sampleWidth = a.sampleWidth;
            g.sampleHeight = a.sampleHeight;
            g.firstPass = a.firstPass;
            g.nPasses = now;
            g.seed = a.seed;
            if (p.flags & KAJO_FLAG_AOV_MATTE)
                g.matteIds = h->aovTiled ? h->matteTiles.p : h->matte.p;
            unsigned long long blocks = (unsigned long long)((h->W + 7) / 8) * ((h->H + 7) / 8);
            if (h->aovTiled) {
                // one wave per 8x8 block of the handle's own tiles, in the tile buffer's order (nTilesOwned > 0 here: no empty grid)
                blocks = (unsigned long long)h->nTilesOwned * (p.tileW / 8) * (p.tileH / 8);
                g.tiledBlocks = (int32_t)blocks;
                g.tileWaves = (uint32_t)(p.tileW / 8) | ((uint32_t)(p.tileH / 8) << 16);
                g.tileIndex = p.tileIndex;
                g.tileCount = p.tileCount;
            }
            HIP_TRY((hipError_t)h->k->aov(&g, h->aovInstance, (unsigned)((blocks + 3) / 4), h->aovLds, h->stream));
            h->aovPasses += now;
        }
        if (shortGrid) {
            // adaptive sampling, behind every launch and outside the timing events: the retired slots extended to the new pass count and,
            // at a batch boundary, the batch into the moments of the active ones (a handle that retires has rendered every pass: no rebase)
            const int after = h->passesDone + now, boundary = after % KAJO_NOISE_BATCH_PASSES == 0;
            HIP_TRY((hipError_t)kajo_adapt_step_launch(h->tiles.p, h->noiseBase.p, h->noiseMoments.p, h->adaptStateDev.p,
                                                       (uint32_t)((size_t)h->nTilesOwned * p.tileW * p.tileH), h->adaptShift, boundary, after,
                                                       h->stream));
        } else if (h->noise && (h->passesDone + now) % KAJO_NOISE_BATCH_PASSES == 0) {
            // a batch boundary, behind the launch (and its fold) and outside the timing events: the batch into the moments -- or, where this
            // handle did not render all of it, only the baseline
            if (h->noiseRebase)
                HIP_TRY(hipMemcpyAsync(h->noiseBase.p, h->tiles.p, h->tileBytes, hipMemcpyDeviceToDevice, h->stream));
            else
                HIP_TRY((hipError_t)kajo_noise_update_launch(h->tiles.p, h->noiseBase.p, h->noiseMoments.p,
                                                             (uint32_t)((size_t)h->nTilesOwned * p.tileW * p.tileH), h->stream));
            h->noiseRebase = false;
        }
        if (a.waveTrips && s.split == 1 && s.chunks == 1) {
            h->tripsPending = true;
            a.waveTrips = nullptr; // later launches of this call keep the first measurement
        }
        if (launch)
            h->launches++;
        h->passesDone += now;
        h->carryValid = s.endsInside;
        left -= now;
        if (h->adaptive) {
            h->adaptPaths += h->adaptActivePixels * a.n * a.n * now;
            if (h->adaptSet && activeUnits > 0 && !h->noiseRebase && h->passesDone >= h->adaptParams.minPasses &&
                h->passesDone % (KAJO_NOISE_BATCH_PASSES * h->adaptParams.checkEvery) == 0 && (rc = adaptDecide(h)))
                return rc;
        }
    }
    h->frameValid = false;
    return KAJO_OK;
}

int kajo_hip_wait(kajo_hip_t h)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    int rc = bind(h);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    // (an adaptive handle: trips are measured only while no unit has retired, and a decision applies a waiting cost order before it
    // counts retirements, so no filtered order has to follow the update here)
    if (h->tripsPending && (rc = updateBlockOrder(h)))
        return rc;
    return drainEvents(h);
}

int kajo_hip_reset(kajo_hip_t h)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    int rc = kajo_hip_wait(h);
    if (rc)
        return rc;
    HIP_TRY(hipMemsetAsync(h->tiles.p, 0, h->tileBytes, h->stream));
    if (h->counters)
        HIP_TRY(hipMemsetAsync(h->counters.p, 0, 32 * sizeof(unsigned long long), h->stream));
    if (h->aov)
        HIP_TRY(hipMemsetAsync(h->aov.p, 0, 2 * (size_t)h->W * h->H * 16, h->stream));
    if (h->matte)
        HIP_TRY(hipMemsetAsync(h->matte.p, 0, matteTableBytes(h), h->stream));
    if (h->aovTiles)
        HIP_TRY(hipMemsetAsync(h->aovTiles.p, 0, aovTileBytes(h), h->stream));
    if (h->matteTiles)
        HIP_TRY(hipMemsetAsync(h->matteTiles.p, 0, matteTileBytes(h), h->stream));
    if (h->noise) {
        HIP_TRY(hipMemsetAsync(h->noiseBase.p, 0, h->tileBytes, h->stream));
        HIP_TRY(hipMemsetAsync(h->noiseMoments.p, 0, 2 * h->tileBytes, h->stream));
        h->noiseRebase = false;
    }
    if (h->adaptive)
        HIP_TRY(hipMemsetAsync(h->adaptStateDev.p, 0, (size_t)h->gridBlocks * sizeof(uint32_t), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    adaptReactivate(h);
    h->aovComposed = h->matteComposed = false;
    h->aovPasses = 0;
    h->passesDone = 0;
    h->guideStamp = -1;
    h->carryValid = false;
    h->frameValid = false;
    h->kernelMs = 0.0;
    h->launches = 0;
    return KAJO_OK;
}

int kajo_hip_set_pass_count(kajo_hip_t h, int passesDone)
{
    if (!h || passesDone < 0 || passesDone > 0x7ffffffe)
        return fail(KAJO_E_INVALID, "invalid argument");
    if (h->adaptive && passesDone != 0)
        return fail(KAJO_E_STATE, "an adaptive handle keeps a pass count per unit, which a restored buffer does not tell: set_pass_count is refused");
    int rc = kajo_hip_wait(h);
    if (rc)
        return rc;
    if (h->adaptive) { // (to pass 0: the moments start over below, and so do the units)
        HIP_TRY(hipMemsetAsync(h->adaptStateDev.p, 0, (size_t)h->gridBlocks * sizeof(uint32_t), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        adaptReactivate(h);
    }
    if (h->noise) {
        // the moments start over; the baseline is the buffer at the first batch boundary from here on (kajo_hip_render)
        HIP_TRY(hipMemsetAsync(h->noiseMoments.p, 0, 2 * h->tileBytes, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->noiseRebase = true;
    }
    h->passesDone = passesDone;
    h->guideStamp = -1;
    h->carryValid = false; // (a group in progress is not known apart from the buffer the caller declares: include/kajo_hip.h)
    h->frameValid = false;
    return KAJO_OK;
}

int kajo_hip_tile_buffer(kajo_hip_t h, void** devicePtr, size_t* bytes)
{
    if (!h || !devicePtr || !bytes)
        return fail(KAJO_E_INVALID, "null argument");
    *devicePtr = h->tiles.p;
    *bytes = h->tileBytes;
    return KAJO_OK;
}

int kajo_hip_compose(kajo_hip_t h, const void* gathered)
{
    if (!h || !gathered)
        return fail(KAJO_E_INVALID, "null argument");
    int rc = bind(h);
    if (rc)
        return rc;
    HIP_TRY(h->frame.ensure((size_t)h->W * h->H * 16));
    HIP_TRY((hipError_t)kajo_compose_launch(gathered, &h->map, h->frame.p, h->stream));
    h->frameValid = true;
    return KAJO_OK;
}

int kajo_hip_aov_tile_buffers(kajo_hip_t h, void** aov, size_t* aovBytes, void** matte, size_t* matteBytes)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    if (!h->aovTiled)
        return fail(KAJO_E_STATE, "the handle was created without the tiled AOV flag: its AOV sums are whole-frame buffers");
    if (aov)
        *aov = h->aovTiles.p;
    if (aovBytes)
        *aovBytes = aovTileBytes(h);
    if (matte)
        *matte = h->matteTiles.p;
    if (matteBytes)
        *matteBytes = h->matteTiles ? matteTileBytes(h) : 0;
    return KAJO_OK;
}

int kajo_hip_compose_aov(kajo_hip_t h, const void* gatheredAov, const void* gatheredMatte)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    if (!h->aovTiled)
        return fail(KAJO_E_STATE, "the handle was created without the tiled AOV flag: its AOV sums are whole-frame buffers already");
    if (h->map.tileCount == 1) {
        if (!gatheredAov)
            gatheredAov = h->aovTiles.p;
        if (!gatheredMatte)
            gatheredMatte = h->matteTiles.p;
    } else if (!gatheredAov)
        return fail(KAJO_E_INVALID, "a handle that owns part of the frame needs the gathered AOV tile buffers");
    if (!(h->params.flags & KAJO_FLAG_AOV_MATTE))
        gatheredMatte = nullptr;
    int rc = bind(h);
    if (rc)
        return rc;
    HIP_TRY(h->aov.ensure(2 * (size_t)h->W * h->H * 16));
    if (gatheredMatte)
        HIP_TRY(h->matte.ensure(matteTableBytes(h)));
    HIP_TRY((hipError_t)kajo_compose_aov_launch(gatheredAov, gatheredMatte, &h->map, h->aov.p, gatheredMatte ? h->matte.p : nullptr, h->stream));
    h->aovComposed = true;
    h->matteComposed = gatheredMatte != nullptr;
    return KAJO_OK;
}

int kajo_hip_resolve_gathered_argb8_device(kajo_hip_t h, const void* gathered, void* dst)
{
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    Image img;
    int rc = imageOf(h, true, gathered, &img);
    return rc ? rc : resolve(h, img, dst);
}

int kajo_hip_resolve_argb8_device(kajo_hip_t h, void* dst)
{
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    Image img;
    int rc = imageOf(h, false, nullptr, &img);
    return rc ? rc : resolve(h, img, dst);
}

int kajo_hip_resolve_argb8(kajo_hip_t h, uint32_t* dst)
{
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    int rc = bind(h);
    if (rc)
        return rc;
    const size_t bytes = (size_t)h->W * h->H * 4;
    HIP_TRY(h->argb.ensure(bytes));
    if ((rc = kajo_hip_resolve_argb8_device(h, h->argb.p)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dst, h->argb.p, bytes, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_read_radiance(kajo_hip_t h, float* dst)
{
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    int rc = bind(h);
    if (rc)
        return rc;
    if ((rc = composeOwn(h)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dst, h->frame.p, (size_t)h->W * h->H * 16, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_read_aov(kajo_hip_t h, float* albedoHits, float* normalDepth, int64_t* samples)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    int rc = aovReady(h, "the handle was created without the AOV flag: no first-hit AOVs to read");
    if (rc)
        return rc;
    if ((rc = bind(h)))
        return rc;
    const size_t bytes = (size_t)h->W * h->H * 16;
    if (albedoHits)
        HIP_TRY(hipMemcpyAsync(albedoHits, h->aov.p, bytes, hipMemcpyDeviceToHost, h->stream));
    if (normalDepth)
        HIP_TRY(hipMemcpyAsync(normalDepth, h->aov.as<char>() + bytes, bytes, hipMemcpyDeviceToHost, h->stream));
    if ((rc = kajo_hip_wait(h)))
        return rc;
    if (samples)
        *samples = (int64_t)aovSamples(h);
    return KAJO_OK;
}

const char* kajo_hip_aov_kernel(kajo_hip_t h)
{
    if (!h || !(h->params.flags & KAJO_FLAG_AOV))
        return nullptr;
    return h->k->aovNames[h->aovInstance];
}

int kajo_hip_read_matte(kajo_hip_t h, int32_t* ids, uint32_t* counts, int64_t* samples)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    int rc = matteReady(h);
    if (rc)
        return rc;
    if ((rc = bind(h)))
        return rc;
    const size_t count = (size_t)h->W * h->H, words = count * KAJO_MATTE_SLOTS * 4;
    if (ids || counts) {
        HIP_TRY(h->matteScratch.ensure(matteScratchBytes(h)));
        char* ranked = h->matteScratch.as<char>();
        hipError_t le = (hipError_t)kajo_matte_rank_launch(h->matte.p, h->matte.as<char>() + words, h->W, h->H, ranked, ranked + words, h->stream);
        if (le != hipSuccess)
            return failHip(le, "matte rank kernel launch");
        if (ids)
            HIP_TRY(hipMemcpyAsync(ids, ranked, words, hipMemcpyDeviceToHost, h->stream));
        if (counts)
            HIP_TRY(hipMemcpyAsync(counts, ranked + words, words, hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = kajo_hip_wait(h)))
        return rc;
    if (samples)
        *samples = (int64_t)aovSamples(h);
    return KAJO_OK;
}

int kajo_hip_matte_mask(kajo_hip_t h, const int32_t* objects, int n, float* mask, float* dominant)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    if (n < 0 || (n > 0 && !objects))
        return fail(KAJO_E_INVALID, "invalid object list");
    int rc = matteReady(h);
    if (rc)
        return rc;
    const int nObjects = h->staged.nPlanes + h->staged.nSpheres;
    std::vector<uint32_t> selected(matteBitsetWords(h), 0u);
    for (int i = 0; i < n; i++) {
        if (objects[i] < 0 || objects[i] > nObjects)
            return fail(KAJO_E_INVALID, "object id out of range: 0 (the background) .. the number of planes and spheres");
        selected[(size_t)objects[i] >> 5] |= 1u << (objects[i] & 31);
    }
    if ((rc = bind(h)))
        return rc;
    if (mask || dominant) {
        const size_t count = (size_t)h->W * h->H, words = count * KAJO_MATTE_SLOTS * 4;
        HIP_TRY(h->matteScratch.ensure(matteScratchBytes(h)));
        char* scratch = h->matteScratch.as<char>();
        float* maskDevice = reinterpret_cast<float*>(scratch + 2 * words);
        float* dominantDevice = maskDevice + count;
        void* bits = dominantDevice + count;
        // (pageable host memory: the copy has left `selected` when the call returns)
        HIP_TRY(hipMemcpyAsync(bits, selected.data(), selected.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        hipError_t le = (hipError_t)kajo_matte_mask_launch(h->matte.p, h->matte.as<char>() + words, h->W, h->H, bits, (unsigned)nObjects,
                                                           (float)aovSamples(h), mask ? maskDevice : nullptr, dominant ? dominantDevice : nullptr,
                                                           h->stream);
        if (le != hipSuccess)
            return failHip(le, "matte mask kernel launch");
        if (mask)
            HIP_TRY(hipMemcpyAsync(mask, maskDevice, count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (dominant)
            HIP_TRY(hipMemcpyAsync(dominant, dominantDevice, count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    return kajo_hip_wait(h);
}

void kajo_hip_default_denoise_params(KajoDenoiseParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->iterations = 5;
    p->flags = 0;
    p->sigmaLuminance = 4.0f;
    p->sigmaNormal = 128.0f;
    p->sigmaDepth = 1.0f;
}

} // extern "C"

namespace
{

// the planes of kajo_hip_denoise_guide_planes describe the frame as it stands
bool guidePlanesValid(const KajoHip* h)
{
    return h->guidePlanes && h->guideStamp >= 0 && h->guideStamp == h->passesDone;
}

// kajo_hip_denoise's refusals of the parameters (before the handle is looked at) and of the handle
int checkDenoise(kajo_hip_t h, const KajoDenoiseParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null denoise parameters");
    if (p->iterations < 0 || p->iterations > 8)
        return fail(KAJO_E_INVALID, "denoise iterations must be in [0, 8]");
    for (float sigma : {p->sigmaLuminance, p->sigmaNormal, p->sigmaDepth})
        if (!std::isfinite(sigma) || sigma < 0.0f)
            return fail(KAJO_E_INVALID, "denoise sigmas must be finite and not negative");
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    int rc = aovReady(h, "the handle was created without the AOV flag: nothing to guide the denoiser");
    if (rc)
        return rc;
    if (h->passesDone < 1)
        return fail(KAJO_E_STATE, "nothing rendered yet");
    // (tiled AOVs on an owner of part of the frame: the frame to filter is the composed one)
    if (h->map.tileCount != 1 && !h->frameValid)
        return fail(KAJO_E_STATE, "whole-frame output needs kajo_hip_compose() when tileCount > 1");
    // the noise-guided filter needs every pixel's m and se: uploaded planes of this pass count, or the records of the frame's one owner
    if ((p->flags & KAJO_DENOISE_NOISE_GUIDED) && p->iterations >= 1 && !guidePlanesValid(h) && !(h->noise && h->map.tileCount == 1)) {
        if (h->guideStamp >= 0)
            return fail(KAJO_E_STATE, "noise-guided denoise: the uploaded guide planes are for another pass count");
        if (!h->noise)
            return fail(KAJO_E_STATE, "noise-guided denoise: the handle was created without the noise flag and no guide planes are uploaded");
        return fail(KAJO_E_STATE, "noise-guided denoise: the handle holds the records of part of the frame only and no guide planes are uploaded");
    }
    return KAJO_OK;
}

// The denoised frame (sums over passes, row-major) on the handle's stream, in the denoiser's scratch: *out points into it. Checked by
// checkDenoise, device bound. staged: the frame to filter where a stage ran in front (what despeckleImage wrote), in the handle's tile
// layout or row-major -- null = the accumulation: the handle's own tiles while it is the frame's one owner, else the composed frame
// (tiled AOVs; checkDenoise has seen it valid).
int denoiseFrame(KajoHip* h, const KajoDenoiseParams* p, void** out, const Image* staged = nullptr)
{
    const Image img = staged ? *staged : h->map.tileCount == 1 ? Image{h->tiles.p, true} : Image{h->frame.p, false};
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->denoise.ensure(count * (3 * 16 + 4)));
    char* scratch = h->denoise.as<char>();
    *out = scratch + count * 16;
    if (p->iterations == 0) {
        // the frame itself
        if (img.fromTiles)
            HIP_TRY((hipError_t)kajo_compose_launch(img.src, &h->map, *out, h->stream));
        else
            HIP_TRY(hipMemcpyAsync(*out, img.src, count * 16, hipMemcpyDeviceToDevice, h->stream));
    } else {
        const long long samples = std::max(aovSamples(h), 1LL);
        hipError_t le;
        if (p->flags & KAJO_DENOISE_NOISE_GUIDED) {
            // (checkDenoise has seen one of the two sources at hand; the planes come first. The records describe the accumulation, also
            // where the frame to filter is a staged one)
            const bool planes = guidePlanesValid(h);
            const float* m = planes ? h->guidePlanes.as<float>() : nullptr;
            le = (hipError_t)kajo_denoise_guided_launch(img.src, &h->map, img.fromTiles ? 1 : 0, h->aov.p, h->aov.as<char>() + count * 16,
                                                        (float)h->passesDone, (float)samples, p->iterations,
                                                        (p->flags & KAJO_DENOISE_NO_DEMODULATE) ? 0 : 1, p->sigmaLuminance, p->sigmaNormal,
                                                        p->sigmaDepth, planes ? nullptr : h->noiseMoments.p, m, planes ? m + count : nullptr, scratch,
                                                        out, h->stream);
        } else
            le = (hipError_t)kajo_denoise_launch(img.src, &h->map, img.fromTiles ? 1 : 0, h->aov.p, h->aov.as<char>() + count * 16,
                                                 (float)h->passesDone, (float)samples, p->iterations,
                                                 (p->flags & KAJO_DENOISE_NO_DEMODULATE) ? 0 : 1, p->sigmaLuminance, p->sigmaNormal,
                                                 p->sigmaDepth, scratch, out, h->stream);
        if (le != hipSuccess)
            return failHip(le, "denoise kernel launch");
    }
    return KAJO_OK;
}

// KajoToneParams -> the kernels' ToneArgs, or a refusal (KAJO_E_INVALID) before any device work
int toneArgsOf(const KajoToneParams* p, ToneArgs* t)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null tone parameters");
    if (p->curve != KAJO_TONE_CLAMP && p->curve != KAJO_TONE_REINHARD && p->curve != KAJO_TONE_ACES)
        return fail(KAJO_E_INVALID, "unknown tone curve");
    if (p->flags & ~KAJO_TONE_AUTO_EXPOSURE)
        return fail(KAJO_E_INVALID, "unknown tone flag");
    if (!std::isfinite(p->exposure) || p->exposure < -32.0f || p->exposure > 32.0f)
        return fail(KAJO_E_INVALID, "tone exposure must be finite and in [-32, 32]");
    if (!std::isfinite(p->white) || p->white < 0.0f)
        return fail(KAJO_E_INVALID, "tone white point must be finite and not negative");
    if ((p->flags & KAJO_TONE_AUTO_EXPOSURE) && !(std::isfinite(p->key) && p->key > 0.0f))
        return fail(KAJO_E_INVALID, "tone key must be finite and positive");
    for (float r : p->reserved)
        if (r != 0.0f)
            return fail(KAJO_E_INVALID, "tone reserved fields must be 0");
    t->curve = p->curve;
    t->autoExposure = (p->flags & KAJO_TONE_AUTO_EXPOSURE) ? 1 : 0;
    t->exposureScale = std::exp2(p->exposure);
    t->white = p->white;
    t->key = p->key;
    return KAJO_OK;
}

// Enqueue the tone mapping of an image (tiles through h->map's geometry, or the row-major frame) into dst (device)
int toneLaunch(KajoHip* h, Image img, const ToneArgs& t, void* dst)
{
    const size_t scratch = KAJO_TONE_PARTIALS_OFFSET + (size_t)((h->W + 63) / 64) * (size_t)((h->H + 15) / 16) * 16; // tonemap.inc.hip kToneRect*
    if (t.autoExposure)
        HIP_TRY(h->tone.ensure(scratch));
    hipError_t le = (hipError_t)h->k->tone(img.src, &h->map, img.fromTiles ? 1 : 0, (float)h->passesDone, &t, h->tone.p, dst, h->stream);
    if (le != hipSuccess)
        return failHip(le, "tone mapping kernel launch");
    h->toneScaleState = t.autoExposure ? 2 : 1;
    h->toneScale = t.exposureScale;
    return KAJO_OK;
}

constexpr int kGlareMaxLevels = 12;

// The refusals of KajoGlareParams (KAJO_E_INVALID), before any device work and before the handle is looked at
int checkGlare(const KajoGlareParams* g)
{
    if (!g)
        return fail(KAJO_E_INVALID, "null glare parameters");
    if (g->levels < 0 || g->levels > kGlareMaxLevels)
        return fail(KAJO_E_INVALID, "glare levels must be in [0, 12]");
    if (g->flags)
        return fail(KAJO_E_INVALID, "unknown glare flag");
    if (!std::isfinite(g->strength) || g->strength < 0.0f || g->strength > 1.0f)
        return fail(KAJO_E_INVALID, "glare strength must be finite and in [0, 1]");
    if (!std::isfinite(g->threshold) || g->threshold < 0.0f)
        return fail(KAJO_E_INVALID, "glare threshold must be finite and not negative");
    for (float r : g->reserved)
        if (r != 0.0f)
            return fail(KAJO_E_INVALID, "glare reserved fields must be 0");
    return KAJO_OK;
}

// Enqueue the glare of an image (tiles through h->map's geometry, or a row-major frame): *out = the row-major frame in the glare scratch
// that holds the result -- or the image itself where the definition makes the output a copy (strength 0, no level). Checked by checkGlare,
// device bound.
int glareImage(KajoHip* h, const KajoGlareParams* g, Image img, Image* out)
{
    const int n = kajo_glare_plan(h->W, h->H, g->levels, nullptr);
    if (n == 0 || g->strength == 0.0f) {
        *out = img;
        return KAJO_OK;
    }
    size_t pyramid = 0;
    (void)kajo_glare_plan(h->W, h->H, kGlareMaxLevels, &pyramid);
    HIP_TRY(h->glare.ensure((pyramid + (size_t)h->W * h->H) * 16));
    void* frame = h->glare.as<char>() + pyramid * 16;
    hipError_t le = (hipError_t)kajo_glare_launch(img.src, &h->map, img.fromTiles ? 1 : 0, (float)h->passesDone, n, g->strength, g->threshold,
                                                  h->glare.p, frame, h->stream);
    if (le != hipSuccess)
        return failHip(le, "glare kernel launch");
    *out = Image{frame, false};
    return KAJO_OK;
}

// The refusals of KajoDespeckleParams (KAJO_E_INVALID), before any device work and before the handle is looked at
int checkDespeckle(const KajoDespeckleParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null despeckle parameters");
    if (!std::isfinite(p->factor) || p->factor < 0.0f || (p->factor > 0.0f && p->factor < 1.0f))
        return fail(KAJO_E_INVALID, "despeckle factor must be 0 or a finite number >= 1");
    if (p->rank < 1 || p->rank > 4)
        return fail(KAJO_E_INVALID, "despeckle rank must be in [1, 4]");
    if (!std::isfinite(p->floor) || p->floor < 0.0f)
        return fail(KAJO_E_INVALID, "despeckle floor must be finite and not negative");
    if (p->flags)
        return fail(KAJO_E_INVALID, "unknown despeckle flag");
    for (float r : p->reserved)
        if (r != 0.0f)
            return fail(KAJO_E_INVALID, "despeckle reserved fields must be 0");
    return KAJO_OK;
}

// Enqueue the despeckle of an image (tiles through h->map's geometry, or a row-major frame): *out = the frame in the despeckle scratch
// that holds the result -- row-major, or with asTiles in the handle's own tile layout (one owner), where the denoiser takes it for the
// accumulation. The counts stay in the scratch's first two words. Checked by checkDespeckle, device bound.
int despeckleImage(KajoHip* h, const KajoDespeckleParams* p, Image img, bool asTiles, Image* out)
{
    const size_t count = (size_t)h->W * h->H;
    const size_t partials = (2 * (size_t)kajo_despeckle_groups(h->W, h->H) * 4 + 15) / 16 * 16;
    const size_t outSlots = std::max(count, h->map.tileCount == 1 ? (size_t)h->map.slotsPerOwner : (size_t)0);
    HIP_TRY(h->despeckle.ensure(16 + partials + (count + outSlots) * 16));
    char* base = h->despeckle.as<char>();
    void* clamped = base + 16 + partials;
    void* frame = base + 16 + partials + count * 16;
    hipError_t le = (hipError_t)kajo_despeckle_launch(img.src, &h->map, img.fromTiles ? 1 : 0, (float)h->passesDone, p->factor, p->rank, p->floor,
                                                      clamped, frame, asTiles ? 1 : 0, base + 16, base, h->stream);
    if (le != hipSuccess)
        return failHip(le, "despeckle kernel launch");
    h->despeckled = true;
    *out = Image{frame, asTiles};
    return KAJO_OK;
}

// the rays of the known-answer entry points as the kernels read them: float [n][6], origin then direction
std::vector<float> packRays(int n, const float* origins, const float* dirs)
{
    std::vector<float> rays(6 * (size_t)n);
    for (int i = 0; i < n; i++) {
        std::memcpy(&rays[6 * (size_t)i], origins + 3 * (size_t)i, 12);
        std::memcpy(&rays[6 * (size_t)i + 3], dirs + 3 * (size_t)i, 12);
    }
    return rays;
}

} // namespace

extern "C" {

int kajo_hip_denoise(kajo_hip_t h, const KajoDenoiseParams* p, float* radiance, uint32_t* argb8)
{
    // (the parameters first: their refusals do not need a handle)
    int rc = checkDenoise(h, p);
    if (rc)
        return rc;
    if ((rc = bind(h)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    void* out = nullptr;
    if ((rc = denoiseFrame(h, p, &out)))
        return rc;
    void* argb = h->denoise.as<char>() + 3 * count * 16;
    if (argb8) {
        if ((rc = resolve(h, Image{out, false}, argb)))
            return rc;
        HIP_TRY(hipMemcpyAsync(argb8, argb, count * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (radiance)
        HIP_TRY(hipMemcpyAsync(radiance, out, count * 16, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_denoise_guide_planes(kajo_hip_t h, const float* mean, const float* stderror)
{
    if ((mean == nullptr) != (stderror == nullptr))
        return fail(KAJO_E_INVALID, "guide planes: mean and stderror are given together or not at all");
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    if (!mean) {
        h->guideStamp = -1;
        return KAJO_OK;
    }
    int rc = bind(h);
    if (rc)
        return rc;
    const size_t plane = (size_t)h->W * h->H * sizeof(float);
    h->guideStamp = -1;
    HIP_TRY(h->guidePlanes.ensure(2 * plane));
    HIP_TRY(hipMemcpyAsync(h->guidePlanes.p, mean, plane, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->guidePlanes.as<char>() + plane, stderror, plane, hipMemcpyHostToDevice, h->stream));
    if ((rc = kajo_hip_wait(h)))
        return rc;
    h->guideStamp = h->passesDone;
    return KAJO_OK;
}

void kajo_hip_default_tone_params(KajoToneParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->curve = KAJO_TONE_CLAMP;
    p->flags = 0;
    p->exposure = 0.0f;
    p->white = 0.0f;
    p->key = 0.18f;
}

int kajo_hip_tonemap_argb8(kajo_hip_t h, const KajoToneParams* p, const KajoDenoiseParams* denoise, uint32_t* argb8, float* scale)
{
    // (every refusal before any device work: the parameters, the denoiser's, then the handle)
    ToneArgs t{};
    int rc = toneArgsOf(p, &t);
    if (rc)
        return rc;
    if (denoise) {
        if ((rc = checkDenoise(h, denoise)))
            return rc;
    } else if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    // (with the AOV flag, which the denoiser needs, the handle is the frame's one owner: nothing is composed here)
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->argb.ensure(count * 4));
    if (denoise) {
        void* out = nullptr;
        if ((rc = denoiseFrame(h, denoise, &out)))
            return rc;
        img = Image{out, false};
    }
    if ((rc = toneLaunch(h, img, t, h->argb.p)))
        return rc;
    if (argb8)
        HIP_TRY(hipMemcpyAsync(argb8, h->argb.p, count * 4, hipMemcpyDeviceToHost, h->stream));
    return scale ? kajo_hip_tone_scale(h, scale) : kajo_hip_wait(h);
}

int kajo_hip_tonemap_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoToneParams* p, void* dst)
{
    ToneArgs t{};
    int rc = toneArgsOf(p, &t);
    if (rc)
        return rc;
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    Image img;
    return (rc = imageOf(h, true, gathered, &img)) ? rc : toneLaunch(h, img, t, dst);
}

void kajo_hip_default_glare_params(KajoGlareParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->levels = 6;
    p->flags = 0;
    p->strength = 0.1f;
    p->threshold = 0.0f;
}

int kajo_hip_glare(kajo_hip_t h, const KajoGlareParams* g, const KajoDenoiseParams* denoise, float* radiance)
{
    // (every refusal before any device work: the parameters, the denoiser's, then the handle)
    int rc = checkGlare(g);
    if (rc)
        return rc;
    if (denoise) {
        if ((rc = checkDenoise(h, denoise)))
            return rc;
    } else if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    if (denoise) {
        void* out = nullptr;
        if ((rc = denoiseFrame(h, denoise, &out)))
            return rc;
        img = Image{out, false};
    }
    if ((rc = glareImage(h, g, img, &img)))
        return rc;
    if (img.fromTiles) {
        // (a copy of the accumulation: the composed frame, as kajo_hip_read_radiance)
        if ((rc = composeOwn(h)))
            return rc;
        img = Image{h->frame.p, false};
    }
    if (radiance)
        HIP_TRY(hipMemcpyAsync(radiance, img.src, (size_t)h->W * h->H * 16, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_display_argb8(kajo_hip_t h, const KajoDenoiseParams* denoise, const KajoGlareParams* g, const KajoToneParams* tone, uint32_t* argb8,
                           float* scale)
{
    // (every refusal before any device work: the glare parameters, the tone parameters, the denoiser's, then the handle)
    int rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    ToneArgs t{};
    if ((rc = toneArgsOf(tone, &t)))
        return rc;
    if (denoise) {
        if ((rc = checkDenoise(h, denoise)))
            return rc;
    } else if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->argb.ensure(count * 4));
    if (denoise) {
        void* out = nullptr;
        if ((rc = denoiseFrame(h, denoise, &out)))
            return rc;
        img = Image{out, false};
    }
    if (g && (rc = glareImage(h, g, img, &img)))
        return rc;
    if ((rc = toneLaunch(h, img, t, h->argb.p)))
        return rc;
    if (argb8)
        HIP_TRY(hipMemcpyAsync(argb8, h->argb.p, count * 4, hipMemcpyDeviceToHost, h->stream));
    return scale ? kajo_hip_tone_scale(h, scale) : kajo_hip_wait(h);
}

int kajo_hip_display_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoGlareParams* g, const KajoToneParams* tone, void* dst)
{
    int rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    ToneArgs t{};
    if ((rc = toneArgsOf(tone, &t)))
        return rc;
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    Image img;
    if ((rc = imageOf(h, true, gathered, &img)))
        return rc;
    if (g && (rc = glareImage(h, g, img, &img)))
        return rc;
    return toneLaunch(h, img, t, dst);
}

void kajo_hip_default_despeckle_params(KajoDespeckleParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->factor = 16.0f; // (the quality sweep)
    p->rank = 1;
    p->floor = 0.2f;
    p->flags = 0;
}

int kajo_hip_despeckle(kajo_hip_t h, const KajoDespeckleParams* p, float* radiance, int64_t counts[2])
{
    int rc = checkDespeckle(p);
    if (rc)
        return rc;
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    if ((rc = despeckleImage(h, p, img, false, &img)))
        return rc;
    if (radiance)
        HIP_TRY(hipMemcpyAsync(radiance, img.src, (size_t)h->W * h->H * 16, hipMemcpyDeviceToHost, h->stream));
    return counts ? kajo_hip_despeckle_counts(h, counts) : kajo_hip_wait(h);
}

int kajo_hip_despeckle_counts(kajo_hip_t h, int64_t counts[2])
{
    if (!h || !counts)
        return fail(KAJO_E_INVALID, "null argument");
    if (!h->despeckled)
        return fail(KAJO_E_STATE, "nothing despeckled yet");
    int rc = bind(h);
    if (rc)
        return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "despeckle.hip writes the counts as long long");
    HIP_TRY(hipMemcpyAsync(counts, h->despeckle.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_present_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                           const KajoToneParams* tone, uint32_t* argb8, float* scale)
{
    if (!despeckle)
        return kajo_hip_display_argb8(h, denoise, g, tone, argb8, scale);
    // (every refusal before any device work: the despeckle parameters, the glare's, the tone's, the denoiser's, then the handle)
    int rc = checkDespeckle(despeckle);
    if (rc)
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    ToneArgs t{};
    if ((rc = toneArgsOf(tone, &t)))
        return rc;
    if (denoise) {
        if ((rc = checkDenoise(h, denoise)))
            return rc;
    } else if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->argb.ensure(count * 4));
    // (with the denoiser behind it the stage writes the handle's tile layout where the handle is the frame's one owner, else -- tiled AOVs,
    // the composed frame -- row-major: the denoiser reads either)
    if ((rc = despeckleImage(h, despeckle, img, denoise != nullptr && h->map.tileCount == 1, &img)))
        return rc;
    if (denoise) {
        void* out = nullptr;
        if ((rc = denoiseFrame(h, denoise, &out, &img)))
            return rc;
        img = Image{out, false};
    }
    if (g && (rc = glareImage(h, g, img, &img)))
        return rc;
    if ((rc = toneLaunch(h, img, t, h->argb.p)))
        return rc;
    if (argb8)
        HIP_TRY(hipMemcpyAsync(argb8, h->argb.p, count * 4, hipMemcpyDeviceToHost, h->stream));
    return scale ? kajo_hip_tone_scale(h, scale) : kajo_hip_wait(h);
}

int kajo_hip_present_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                           const KajoToneParams* tone, void* dst)
{
    if (!despeckle)
        return kajo_hip_display_gathered_argb8_device(h, gathered, g, tone, dst);
    int rc = checkDespeckle(despeckle);
    if (rc)
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    ToneArgs t{};
    if ((rc = toneArgsOf(tone, &t)))
        return rc;
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    Image img;
    if ((rc = imageOf(h, true, gathered, &img)))
        return rc;
    if ((rc = despeckleImage(h, despeckle, img, false, &img)))
        return rc;
    if (g && (rc = glareImage(h, g, img, &img)))
        return rc;
    return toneLaunch(h, img, t, dst);
}

} // extern "C"

namespace
{

constexpr int kMeterRow = KAJO_METER_BINS + 1; // meter.hip: a row of counts is the bins, then the pixels that do not count

// The refusals of KajoMeterParams (KAJO_E_INVALID), before any device work and before the handle is looked at
int checkMeter(const KajoMeterParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null meter parameters");
    if (!(std::isfinite(p->percentile) && p->percentile > 0.0f && p->percentile <= 1.0f))
        return fail(KAJO_E_INVALID, "meter percentile must be finite and in (0, 1]");
    if (!(std::isfinite(p->key) && p->key > 0.0f))
        return fail(KAJO_E_INVALID, "meter key must be finite and positive");
    if (!(std::isfinite(p->whitePercentile) && p->whitePercentile > 0.0f && p->whitePercentile <= 1.0f))
        return fail(KAJO_E_INVALID, "meter white percentile must be finite and in (0, 1]");
    if (p->flags & ~KAJO_METER_AUTO_WHITE)
        return fail(KAJO_E_INVALID, "unknown meter flag");
    for (float r : p->reserved)
        if (r != 0.0f)
            return fail(KAJO_E_INVALID, "meter reserved fields must be 0");
    return KAJO_OK;
}

// the float with the bits (b - 1 + base) << 19: the lower edge of inner bin b, b = 1 .. 513 (include/kajo_hip.h)
double meterEdge(int b)
{
    const uint32_t bits = (uint32_t)(b - 1 + ((127 - 16) << 4)) << 19;
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return (double)f;
}

double meterCentre(int b)
{
    return b >= KAJO_METER_BINS - 1 ? meterEdge(KAJO_METER_BINS - 1) : 0.5 * (meterEdge(b) + meterEdge(b + 1));
}

// the centre of the smallest bin b >= 1 whose cumulative count over bins 1..b reaches the rank of q among n > 0 metered pixels
double meterValue(const uint32_t* hist, int64_t n, float q)
{
    const int64_t rank = std::min(n, std::max((int64_t)1, (int64_t)std::ceil((double)q * (double)n)));
    int64_t seen = 0;
    for (int b = 1; b < KAJO_METER_BINS; b++)
        if ((seen += hist[b]) >= rank)
            return meterCentre(b);
    return meterCentre(KAJO_METER_BINS - 1);
}

// Enqueue the metering of an image (tiles through h->map's geometry, or a row-major frame), read the counts back and wait: counts = the
// 514 bins, then the pixels that do not count. Device bound.
int meterImage(KajoHip* h, Image img, uint32_t counts[kMeterRow])
{
    const size_t head = ((size_t)kMeterRow * 4 + 15) / 16 * 16;
    HIP_TRY(h->meter.ensure(head + (size_t)kajo_meter_groups(h->W, h->H) * kMeterRow * 4));
    hipError_t le = (hipError_t)kajo_meter_launch(img.src, &h->map, img.fromTiles ? 1 : 0, (float)h->passesDone, h->meter.as<char>() + head,
                                                  h->meter.p, h->stream);
    if (le != hipSuccess)
        return failHip(le, "meter kernel launch");
    HIP_TRY(hipMemcpyAsync(counts, h->meter.p, (size_t)kMeterRow * 4, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

// counts (meterImage) -> the caller's histogram and the whole result
int meterResult(KajoHip* h, const uint32_t counts[kMeterRow], const KajoMeterParams* p, uint32_t* hist, KajoMeterResult* result)
{
    if (hist)
        std::memcpy(hist, counts, (size_t)KAJO_METER_BINS * 4);
    if (!result)
        return KAJO_OK;
    std::memset(result, 0, sizeof *result);
    result->pixels = (int64_t)h->W * h->H;
    result->nonfinite = counts[KAJO_METER_BINS];
    return kajo_hip_meter_evaluate(counts, p, result);
}

// The chain in front of the tone curves on the handle's stream: despeckle -> denoise -> glare, each optional, *img the frame it starts
// from and then the one it ends with. Checked by the stages' checks, device bound.
int chainImage(KajoHip* h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g, Image* img)
{
    int rc;
    // (with the denoiser behind it the despeckle writes the handle's tile layout where the handle is the frame's one owner, else -- tiled
    // AOVs, the composed frame -- row-major: the denoiser reads either)
    if (despeckle && (rc = despeckleImage(h, despeckle, *img, denoise != nullptr && h->map.tileCount == 1, img)))
        return rc;
    if (denoise) {
        void* out = nullptr;
        if ((rc = denoiseFrame(h, denoise, &out, despeckle ? img : nullptr)))
            return rc;
        *img = Image{out, false};
    }
    if (g && (rc = glareImage(h, g, *img, img)))
        return rc;
    return KAJO_OK;
}

// the refusals of the two metered chain calls in front of the handle's: despeckle, glare, meter, tone (-> *t is not formed here: the
// metering patches the parameters first)
int checkMeteredChain(const KajoDespeckleParams* despeckle, const KajoGlareParams* g, const KajoMeterParams* meter, const KajoToneParams* tone)
{
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    if ((rc = checkMeter(meter)))
        return rc;
    ToneArgs t{};
    if ((rc = toneArgsOf(tone, &t)))
        return rc;
    if (tone->flags & KAJO_TONE_AUTO_EXPOSURE)
        return fail(KAJO_E_INVALID, "metered exposure and the tone parameters' automatic exposure are two automatic exposures: give one");
    return KAJO_OK;
}

// meter *img, evaluate, patch the tone parameters: *t = the kernels' arguments of the metered mapping
int meterAndPatch(KajoHip* h, Image img, const KajoMeterParams* meter, const KajoToneParams* tone, KajoMeterResult* result, ToneArgs* t)
{
    uint32_t counts[kMeterRow];
    int rc = meterImage(h, img, counts);
    if (rc)
        return rc;
    KajoMeterResult measured;
    if ((rc = meterResult(h, counts, meter, nullptr, &measured)))
        return rc;
    KajoToneParams patched;
    if ((rc = kajo_hip_meter_tone(&measured, meter, tone, &patched)))
        return rc;
    if ((rc = toneArgsOf(&patched, t)))
        return rc;
    if (result)
        *result = measured;
    return KAJO_OK;
}

} // namespace

extern "C" {

void kajo_hip_default_meter_params(KajoMeterParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->percentile = 0.5f;
    p->key = 0.18f;
    p->whitePercentile = 0.995f;
    p->flags = 0;
}

int kajo_hip_meter_evaluate(const uint32_t hist[KAJO_METER_BINS], const KajoMeterParams* p, KajoMeterResult* result)
{
    int rc = checkMeter(p);
    if (rc)
        return rc;
    if (!hist || !result)
        return fail(KAJO_E_INVALID, "null argument");
    int64_t n = 0;
    int first = 0, last = 0;
    for (int b = 1; b < KAJO_METER_BINS; b++) {
        n += hist[b];
        if (hist[b]) {
            first = first ? first : b;
            last = b;
        }
    }
    result->under = hist[0];
    result->over = hist[KAJO_METER_BINS - 1];
    result->metered = n;
    result->minBin = first;
    result->maxBin = last;
    result->reserved = 0;
    result->anchorL = result->whiteL = result->exposure = 0.0f;
    if (n > 0) {
        const double anchor = meterValue(hist, n, p->percentile);
        result->anchorL = (float)anchor; // (exact: a bin's centre is a float)
        result->whiteL = (float)meterValue(hist, n, p->whitePercentile);
        result->exposure = (float)std::log2((double)p->key / anchor);
    }
    return KAJO_OK;
}

int kajo_hip_meter_tone(const KajoMeterResult* result, const KajoMeterParams* p, const KajoToneParams* in, KajoToneParams* out)
{
    int rc = checkMeter(p);
    if (rc)
        return rc;
    if (!result || !in || !out)
        return fail(KAJO_E_INVALID, "null argument");
    if (in->flags & KAJO_TONE_AUTO_EXPOSURE)
        return fail(KAJO_E_INVALID, "metered exposure and the tone parameters' automatic exposure are two automatic exposures: give one");
    KajoToneParams t = *in;
    t.exposure = std::min(std::max(in->exposure + result->exposure, -32.0f), 32.0f);
    if (p->flags & KAJO_METER_AUTO_WHITE)
        t.white = (float)((double)result->whiteL * std::exp2((double)t.exposure));
    *out = t;
    return KAJO_OK;
}

int kajo_hip_meter(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                   const KajoMeterParams* meter, uint32_t* hist, KajoMeterResult* result)
{
    // (every refusal before any device work: the despeckle parameters, the glare's, the meter's, the denoiser's, then the handle)
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    if ((rc = checkMeter(meter)))
        return rc;
    if (denoise) {
        if ((rc = checkDenoise(h, denoise)))
            return rc;
    } else if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    if ((rc = chainImage(h, despeckle, denoise, g, &img)))
        return rc;
    uint32_t counts[kMeterRow];
    if ((rc = meterImage(h, img, counts)))
        return rc;
    return meterResult(h, counts, meter, hist, result);
}

int kajo_hip_present_metered_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                                   const KajoMeterParams* meter, const KajoToneParams* tone, uint32_t* argb8, KajoMeterResult* result)
{
    if (!meter)
        return kajo_hip_present_argb8(h, despeckle, denoise, g, tone, argb8, nullptr);
    int rc = checkMeteredChain(despeckle, g, meter, tone);
    if (rc)
        return rc;
    if (denoise) {
        if ((rc = checkDenoise(h, denoise)))
            return rc;
    } else if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->argb.ensure(count * 4));
    if ((rc = chainImage(h, despeckle, denoise, g, &img)))
        return rc;
    ToneArgs t{};
    if ((rc = meterAndPatch(h, img, meter, tone, result, &t)))
        return rc;
    // (the frame the histogram was taken of is still where the chain left it: the same frame is mapped)
    if ((rc = toneLaunch(h, img, t, h->argb.p)))
        return rc;
    if (argb8)
        HIP_TRY(hipMemcpyAsync(argb8, h->argb.p, count * 4, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_present_metered_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle,
                                                   const KajoGlareParams* g, const KajoMeterParams* meter, const KajoToneParams* tone, void* dst,
                                                   KajoMeterResult* result)
{
    if (!meter)
        return kajo_hip_present_gathered_argb8_device(h, gathered, despeckle, g, tone, dst);
    int rc = checkMeteredChain(despeckle, g, meter, tone);
    if (rc)
        return rc;
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    Image img;
    if ((rc = imageOf(h, true, gathered, &img)))
        return rc;
    if ((rc = chainImage(h, despeckle, nullptr, g, &img)))
        return rc;
    ToneArgs t{};
    if ((rc = meterAndPatch(h, img, meter, tone, result, &t))) // (the one wait: include/kajo_hip.h)
        return rc;
    return toneLaunch(h, img, t, dst);
}

} // extern "C"

namespace
{

static_assert(sizeof(KajoNoiseParams) == 8 && sizeof(KajoNoiseMoments) == 32 && sizeof(KajoNoiseResult) == 48, "include/kajo_hip.h states the sizes");
static_assert(KAJO_NOISE_BATCH_PASSES == KAJO_GROUP_PASSES, "a batch boundary is a group boundary: no group in progress, nothing in `carry`");
static_assert(KAJO_NOISE_HIST_WORDS == KAJO_METER_BINS + 2, "the meter's bins, the unknown pixels, the pixels with bad > 0");

bool quantileOk(float q)
{
    return std::isfinite(q) && q > 0.0f && q <= 1.0f;
}

// The refusals of KajoNoiseParams (KAJO_E_INVALID), before any device work and before the handle is looked at
int checkNoise(const KajoNoiseParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null noise parameters");
    if (!(std::isfinite(p->floor) && p->floor > 0.0f))
        return fail(KAJO_E_INVALID, "noise floor must be finite and positive");
    if (!quantileOk(p->quantile))
        return fail(KAJO_E_INVALID, "noise quantile must be finite and in (0, 1]");
    return KAJO_OK;
}

} // namespace

extern "C" {

void kajo_hip_default_noise_params(KajoNoiseParams* p)
{
    if (!p)
        return;
    p->floor = 1e-2f;
    p->quantile = 0.95f;
}

int kajo_hip_noise_evaluate(const uint32_t hist[KAJO_NOISE_HIST_WORDS], float quantile, float* value)
{
    if (!quantileOk(quantile))
        return fail(KAJO_E_INVALID, "noise quantile must be finite and in (0, 1]");
    if (!hist || !value)
        return fail(KAJO_E_INVALID, "null argument");
    int64_t known = 0;
    for (int b = 0; b < KAJO_METER_BINS; b++)
        known += hist[b];
    *value = -1.0f;
    if (known == 0)
        return KAJO_OK;
    const int64_t rank = std::min(known, std::max((int64_t)1, (int64_t)std::ceil((double)quantile * (double)known)));
    int64_t seen = 0;
    int b = 0;
    while (b < KAJO_METER_BINS - 1 && (seen += hist[b]) < rank)
        b++;
    *value = b == 0 ? 0x1p-17f : (float)meterCentre(b);
    return KAJO_OK;
}

int kajo_hip_noise(kajo_hip_t h, const KajoNoiseParams* params, float* mean, float* stderror, float* relative, uint32_t* batches, uint32_t* hist,
                   KajoNoiseResult* result)
{
    int rc = checkNoise(params);
    if (rc)
        return rc;
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    if (!h->noise)
        return fail(KAJO_E_STATE, "the handle was created without the noise flag");
    if ((rc = bind(h)))
        return rc;
    uint32_t counts[KAJO_NOISE_HIST_WORDS] = {};
    const size_t pixels = (size_t)h->W * h->H, plane = pixels * 4;
    void* const dst[4] = {mean, stderror, relative, batches};
    const bool part = h->map.tileCount > 1;
    if (part && h->nTilesOwned > 0 && h->noiseStaged.size() < 4 * pixels)
        h->noiseStaged.resize(4 * pixels);
    if (h->nTilesOwned > 0) {
        HIP_TRY(h->noiseOut.ensure(4 * plane + sizeof counts));
        char* out = h->noiseOut.as<char>();
        HIP_TRY(hipMemsetAsync(out + 4 * plane, 0, sizeof counts, h->stream));
        hipError_t le = (hipError_t)kajo_noise_map_launch(h->noiseMoments.p, &h->map, h->params.tileIndex, (double)params->floor, out, out + plane,
                                                          out + 2 * plane, out + 3 * plane, out + 4 * plane, h->stream);
        if (le != hipSuccess)
            return failHip(le, "noise map kernel launch");
        for (int k = 0; k < 4; k++) {
            if (!dst[k])
                continue;
            void* to = part ? (void*)(h->noiseStaged.data() + k * pixels) : dst[k];
            HIP_TRY(hipMemcpyAsync(to, out + k * plane, plane, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(hipMemcpyAsync(counts, out + 4 * plane, sizeof counts, hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = kajo_hip_wait(h)))
        return rc;
    if (part && h->nTilesOwned > 0 && (mean || stderror || relative || batches))
        for (int y = 0; y < h->H; y++)
            for (int x = 0; x < h->W; x++) {
                int owner;
                uint32_t slot;
                kajoTileSlot(h->map, x, y, &owner, &slot);
                if (owner != h->params.tileIndex)
                    continue;
                const size_t at = (size_t)y * h->W + x;
                for (int k = 0; k < 4; k++)
                    if (dst[k])
                        static_cast<uint32_t*>(dst[k])[at] = h->noiseStaged[k * pixels + at];
            }
    if (hist)
        std::memcpy(hist, counts, sizeof counts);
    if (result) {
        std::memset(result, 0, sizeof *result);
        for (int b = 0; b < KAJO_METER_BINS; b++)
            result->known += counts[b];
        result->unknown = counts[KAJO_METER_BINS];
        result->bad = counts[KAJO_METER_BINS + 1];
        result->pixels = result->known + result->unknown;
        return kajo_hip_noise_evaluate(counts, params->quantile, &result->quantileValue);
    }
    return KAJO_OK;
}

int kajo_hip_read_noise_moments(kajo_hip_t h, KajoNoiseMoments* records)
{
    if (!h || !records)
        return fail(KAJO_E_INVALID, "null argument");
    if (!h->noise)
        return fail(KAJO_E_STATE, "the handle was created without the noise flag");
    int rc = bind(h);
    if (rc)
        return rc;
    std::vector<KajoNoiseMoments> own((size_t)h->map.slotsPerOwner);
    HIP_TRY(hipMemcpyAsync(own.data(), h->noiseMoments.p, own.size() * sizeof(KajoNoiseMoments), hipMemcpyDeviceToHost, h->stream));
    if ((rc = kajo_hip_wait(h)))
        return rc;
    for (int y = 0; y < h->H; y++)
        for (int x = 0; x < h->W; x++) {
            int owner;
            uint32_t slot;
            kajoTileSlot(h->map, x, y, &owner, &slot);
            if (owner == h->params.tileIndex)
                records[(size_t)y * h->W + x] = own[slot];
        }
    return KAJO_OK;
}

static_assert(sizeof(KajoAdaptParams) == 32 && sizeof(KajoAdaptState) == 48, "include/kajo_hip.h states the sizes");

// The refusals of KajoAdaptParams (KAJO_E_INVALID), before the handle is looked at
static int checkAdapt(const KajoAdaptParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null adaptive parameters");
    if (!(p->target > 0.0f))
        return fail(KAJO_E_INVALID, "adaptive target must be above 0");
    if (!(std::isfinite(p->floor) && p->floor > 0.0f))
        return fail(KAJO_E_INVALID, "adaptive floor must be finite and positive");
    if (p->minPasses < 0)
        return fail(KAJO_E_INVALID, "adaptive minPasses must not be negative");
    if (p->checkEvery < 1 || p->checkEvery > 65536)
        return fail(KAJO_E_INVALID, "adaptive checkEvery must be in [1, 65536]");
    if (p->allowance < 0 || p->allowance > 63)
        return fail(KAJO_E_INVALID, "adaptive allowance must be in [0, 63]");
    if (p->reserved[0] || p->reserved[1] || p->reserved[2])
        return fail(KAJO_E_INVALID, "adaptive reserved words must be 0");
    return KAJO_OK;
}

void kajo_hip_default_adapt_params(KajoAdaptParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->floor = 1e-2f;
    p->minPasses = 16;
    p->checkEvery = 4;
}

int kajo_hip_set_adaptive(kajo_hip_t h, const KajoAdaptParams* params)
{
    int rc = checkAdapt(params);
    if (rc)
        return rc;
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    if (!h->adaptive)
        return fail(KAJO_E_STATE, "the handle was created without the adaptive flag");
    if (h->passesDone != 0)
        return fail(KAJO_E_STATE, "the adaptive parameters are set before the first pass (or after kajo_hip_reset)");
    h->adaptParams = *params;
    const long long step = (long long)KAJO_NOISE_BATCH_PASSES * params->checkEvery;
    h->adaptParams.minPasses = (int32_t)std::min<long long>((params->minPasses + step - 1) / step * step, 0x7ffffffell);
    h->adaptSet = true;
    return KAJO_OK;
}

int kajo_hip_adapt_state(kajo_hip_t h, KajoAdaptState* state)
{
    if (!h || !state)
        return fail(KAJO_E_INVALID, "null argument");
    if (!h->adaptive)
        return fail(KAJO_E_STATE, "the handle was created without the adaptive flag");
    int rc = kajo_hip_wait(h);
    if (rc)
        return rc;
    state->units = h->gridBlocks;
    state->activeUnits = h->gridBlocks - h->adaptRetired;
    state->pixels = h->adaptPixels;
    state->activePixels = h->adaptActivePixels;
    state->paths = h->adaptPaths;
    state->lastDecisionPass = h->adaptLastDecision;
    state->unitSlots = (int32_t)(64u * h->lds.wavesPerBlock);
    return KAJO_OK;
}

int kajo_hip_adapt_passes(kajo_hip_t h, uint32_t* plane)
{
    if (!h || !plane)
        return fail(KAJO_E_INVALID, "null argument");
    if (!h->adaptive)
        return fail(KAJO_E_STATE, "the handle was created without the adaptive flag");
    int rc = bind(h);
    if (rc)
        return rc;
    if (h->nTilesOwned == 0)
        return kajo_hip_wait(h);
    const size_t pixels = (size_t)h->W * h->H;
    const bool part = h->map.tileCount > 1;
    if (part && h->adaptStaged.size() < pixels)
        h->adaptStaged.resize(pixels);
    HIP_TRY(h->adaptOut.ensure(pixels * 4));
    hipError_t le = (hipError_t)kajo_adapt_passes_launch(h->noiseMoments.p, h->adaptStateDev.p, &h->map, h->params.tileIndex, h->adaptShift,
                                                         (uint32_t)h->passesDone, h->adaptOut.p, h->stream);
    if (le != hipSuccess)
        return failHip(le, "adaptive pass plane kernel launch");
    HIP_TRY(hipMemcpyAsync(part ? h->adaptStaged.data() : plane, h->adaptOut.p, pixels * 4, hipMemcpyDeviceToHost, h->stream));
    if ((rc = kajo_hip_wait(h)))
        return rc;
    if (part)
        for (int y = 0; y < h->H; y++)
            for (int x = 0; x < h->W; x++) {
                int owner;
                uint32_t slot;
                kajoTileSlot(h->map, x, y, &owner, &slot);
                if (owner == h->params.tileIndex)
                    plane[(size_t)y * h->W + x] = h->adaptStaged[(size_t)y * h->W + x];
            }
    return KAJO_OK;
}

int kajo_hip_adapt_evaluate(const KajoNoiseMoments* records, int64_t count, const KajoAdaptParams* params, uint8_t* loud, int64_t* nLoud)
{
    int rc = checkAdapt(params);
    if (rc)
        return rc;
    if (count < 0 || (count > 0 && !records))
        return fail(KAJO_E_INVALID, "invalid argument");
    const AdaptRule rule{params->target, params->floor, (uint32_t)params->allowance};
    int64_t total = 0;
    for (int64_t i = 0; i < count; i++) {
        const bool is = kajo::adaptLoud(records[i].s1, records[i].s2, records[i].n, rule);
        total += is;
        if (loud)
            loud[i] = is ? 1 : 0;
    }
    if (nLoud)
        *nLoud = total;
    return KAJO_OK;
}

int64_t kajo_hip_adapt_order(const uint32_t* order, uint32_t nUnits, const uint32_t* state, uint32_t wavesPerBlock, int32_t split, uint32_t* out,
                             size_t capacity)
{
    if ((nUnits > 0 && !state) || wavesPerBlock < 1 || wavesPerBlock > 4)
        return fail(KAJO_E_INVALID, "invalid argument");
    if (order)
        for (uint32_t i = 0; i < nUnits; i++)
            if (order[i] >= nUnits)
                return fail(KAJO_E_INVALID, "an order word names a unit the handle does not have");
    std::vector<uint32_t> words;
    kajoAdaptOrder(order, nUnits, state, wavesPerBlock, split != 0, words);
    if (out) {
        if (capacity < words.size())
            return fail(KAJO_E_INVALID, "capacity too small");
        std::copy(words.begin(), words.end(), out);
    }
    return (int64_t)words.size();
}

} // extern "C"

namespace
{

// The refusals of KajoLocalParams (KAJO_E_INVALID), before any device work and before the handle is looked at
int checkLocal(const KajoLocalParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null local parameters");
    if (p->iterations < 0 || p->iterations > 8)
        return fail(KAJO_E_INVALID, "local iterations must be in [0, 8]");
    if (p->flags & ~KAJO_LOCAL_PIVOT_METERED)
        return fail(KAJO_E_INVALID, "unknown local flag");
    if (!(std::isfinite(p->compression) && p->compression > 0.0f && p->compression <= 1.0f))
        return fail(KAJO_E_INVALID, "local compression must be finite and in (0, 1]");
    if (!(std::isfinite(p->detail) && p->detail >= 0.0f && p->detail <= 4.0f))
        return fail(KAJO_E_INVALID, "local detail must be finite and in [0, 4]");
    if (!(std::isfinite(p->sigmaRange) && p->sigmaRange > 0.0f))
        return fail(KAJO_E_INVALID, "local range sigma must be finite and positive");
    if (!(std::isfinite(p->pivot) && p->pivot >= -16.0f && p->pivot <= 16.0f))
        return fail(KAJO_E_INVALID, "local pivot must be finite and in [-16, 16]");
    if (!(std::isfinite(p->pivotPercentile) && p->pivotPercentile > 0.0f && p->pivotPercentile <= 1.0f))
        return fail(KAJO_E_INVALID, "local pivot percentile must be finite and in (0, 1]");
    if (p->reserved != 0.0f)
        return fail(KAJO_E_INVALID, "local reserved fields must be 0");
    return KAJO_OK;
}

// Enqueue the local tone mapping of an image (tiles through h->map's geometry, or a row-major frame): *out = the row-major frame in the
// stage's scratch that holds the result -- or the image itself where the definition makes the output a copy (compression 1 and detail 1).
// With KAJO_LOCAL_PIVOT_METERED the image is metered first and the histogram waited for. Checked by checkLocal, device bound.
int localImage(KajoHip* h, const KajoLocalParams* p, Image img, Image* out)
{
    if (p->compression == 1.0f && p->detail == 1.0f) {
        *out = img;
        return KAJO_OK;
    }
    float pivot = p->pivot;
    if (p->flags & KAJO_LOCAL_PIVOT_METERED) {
        uint32_t counts[kMeterRow];
        int rc = meterImage(h, img, counts);
        if (rc)
            return rc;
        KajoMeterParams m;
        kajo_hip_default_meter_params(&m);
        m.percentile = p->pivotPercentile;
        KajoMeterResult r{};
        if ((rc = kajo_hip_meter_evaluate(counts, &m, &r)))
            return rc;
        if (r.metered > 0)
            pivot = (float)std::log2((double)r.anchorL); // (anchorL = value(pivotPercentile): a bin's centre, exact in float)
    }
    const size_t plane = kajo_local_plane(h->W, h->H);
    HIP_TRY(h->local.ensure(3 * plane * 4 + (size_t)h->W * h->H * 16));
    void* frame = h->local.as<char>() + 3 * plane * 4;
    hipError_t le = (hipError_t)kajo_local_launch(img.src, &h->map, img.fromTiles ? 1 : 0, (float)h->passesDone, p->iterations, p->compression,
                                                  p->detail, p->sigmaRange, pivot, h->local.p, frame, h->stream);
    if (le != hipSuccess)
        return failHip(le, "local tone mapping kernel launch");
    h->localRun = true;
    h->localPivot = pivot;
    *out = Image{frame, false};
    return KAJO_OK;
}

// the refusals of the local chain calls in front of the handle's: despeckle, glare, local, meter, tone
int checkLocalChain(const KajoDespeckleParams* despeckle, const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                    const KajoToneParams* tone, ToneArgs* t)
{
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    if ((rc = checkLocal(local)))
        return rc;
    if (meter && (rc = checkMeter(meter)))
        return rc;
    if ((rc = toneArgsOf(tone, t)))
        return rc;
    if (meter && (tone->flags & KAJO_TONE_AUTO_EXPOSURE))
        return fail(KAJO_E_INVALID, "metered exposure and the tone parameters' automatic exposure are two automatic exposures: give one");
    return KAJO_OK;
}

} // namespace

extern "C" {

void kajo_hip_default_local_params(KajoLocalParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->iterations = 5;
    p->flags = 0;
    p->compression = 0.6f;
    p->detail = 1.0f;
    p->sigmaRange = 2.0f;
    p->pivot = (float)std::log2(0.18);
    p->pivotPercentile = 0.5f;
}

int kajo_hip_local(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                   const KajoLocalParams* local, float* radiance)
{
    // (every refusal before any device work: the despeckle parameters, the glare's, the stage's own, the denoiser's, then the handle)
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    if ((rc = checkLocal(local)))
        return rc;
    if (denoise) {
        if ((rc = checkDenoise(h, denoise)))
            return rc;
    } else if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    if ((rc = chainImage(h, despeckle, denoise, g, &img)))
        return rc;
    if ((rc = localImage(h, local, img, &img)))
        return rc;
    if (img.fromTiles) {
        // (a copy of the accumulation: the composed frame, as kajo_hip_read_radiance)
        if ((rc = composeOwn(h)))
            return rc;
        img = Image{h->frame.p, false};
    }
    if (radiance)
        HIP_TRY(hipMemcpyAsync(radiance, img.src, (size_t)h->W * h->H * 16, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_present_local_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                                 const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone, uint32_t* argb8,
                                 KajoMeterResult* result)
{
    if (!local)
        return kajo_hip_present_metered_argb8(h, despeckle, denoise, g, meter, tone, argb8, result);
    ToneArgs t{};
    int rc = checkLocalChain(despeckle, g, local, meter, tone, &t);
    if (rc)
        return rc;
    if (denoise) {
        if ((rc = checkDenoise(h, denoise)))
            return rc;
    } else if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->argb.ensure(count * 4));
    if ((rc = chainImage(h, despeckle, denoise, g, &img)))
        return rc;
    if ((rc = localImage(h, local, img, &img)))
        return rc;
    // (the meter measures the frame after the stage: what the tone kernels are handed)
    if (meter && (rc = meterAndPatch(h, img, meter, tone, result, &t)))
        return rc;
    if ((rc = toneLaunch(h, img, t, h->argb.p)))
        return rc;
    if (argb8)
        HIP_TRY(hipMemcpyAsync(argb8, h->argb.p, count * 4, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_present_local_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                                 const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone, void* dst,
                                                 KajoMeterResult* result)
{
    if (!local)
        return kajo_hip_present_metered_gathered_argb8_device(h, gathered, despeckle, g, meter, tone, dst, result);
    ToneArgs t{};
    int rc = checkLocalChain(despeckle, g, local, meter, tone, &t);
    if (rc)
        return rc;
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    Image img;
    if ((rc = imageOf(h, true, gathered, &img)))
        return rc;
    if ((rc = chainImage(h, despeckle, nullptr, g, &img)))
        return rc;
    if ((rc = localImage(h, local, img, &img))) // (one wait with KAJO_LOCAL_PIVOT_METERED: include/kajo_hip.h)
        return rc;
    if (meter && (rc = meterAndPatch(h, img, meter, tone, result, &t))) // (and one more)
        return rc;
    return toneLaunch(h, img, t, dst);
}

int kajo_hip_local_pivot(kajo_hip_t h, float* pivot)
{
    if (!h || !pivot)
        return fail(KAJO_E_INVALID, "null argument");
    if (!h->localRun)
        return fail(KAJO_E_STATE, "no local tone mapping yet");
    *pivot = h->localPivot; // (formed on the host before the launch: nothing to wait for)
    return KAJO_OK;
}

} // extern "C"

namespace
{

// The refusals of KajoLensParams (KAJO_E_INVALID), before any device work and before the handle is looked at
int checkLens(const KajoLensParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null lens parameters");
    if (!(std::isfinite(p->aperture) && p->aperture >= 0.0f && p->aperture <= 1.0f))
        return fail(KAJO_E_INVALID, "lens aperture must be finite and in [0, 1]");
    if (!(std::isfinite(p->focusDistance) && p->focusDistance > 0.0f))
        return fail(KAJO_E_INVALID, "lens focus distance must be finite and positive");
    if (p->maxRadius < 1 || p->maxRadius > KAJO_LENS_MAX_RADIUS)
        return fail(KAJO_E_INVALID, "lens max radius must be in [1, 16]");
    if (p->flags)
        return fail(KAJO_E_INVALID, "unknown lens flag");
    for (float r : p->reserved)
        if (r != 0.0f)
            return fail(KAJO_E_INVALID, "lens reserved fields must be 0");
    return KAJO_OK;
}

// ... and of the handle (KAJO_E_STATE), by the denoiser's rules: the whole-frame AOVs at hand, something rendered, the whole frame
int checkLensHandle(kajo_hip_t h)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    int rc = aovReady(h, "the handle was created without the AOV flag: no depth to focus the lens by");
    if (rc)
        return rc;
    if (h->passesDone < 1)
        return fail(KAJO_E_STATE, "nothing rendered yet");
    if (h->map.tileCount != 1 && !h->frameValid)
        return fail(KAJO_E_STATE, "whole-frame output needs kajo_hip_compose() when tileCount > 1");
    return KAJO_OK;
}

size_t lensScratchBytes(const KajoHip* h)
{
    return 2 * kajo_lens_plane(h->W, h->H) * 4 + 2 * (size_t)h->W * h->H * 16;
}

// Enqueue the lens blur of an image (tiles through h->map's geometry, or a row-major frame): *out = the row-major frame in the stage's
// scratch that holds the result -- or the image itself where the definition makes the output a copy (aperture 0). Checked by checkLens
// and checkLensHandle, device bound.
int lensImage(KajoHip* h, const KajoLensParams* p, Image img, Image* out)
{
    if (p->aperture == 0.0f) {
        *out = img;
        return KAJO_OK;
    }
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->lens.ensure(lensScratchBytes(h)));
    void* frame = h->lens.as<char>() + 2 * kajo_lens_plane(h->W, h->H) * 4 + count * 16;
    hipError_t le = (hipError_t)kajo_lens_launch(img.src, &h->map, img.fromTiles ? 1 : 0, (float)h->passesDone, h->aov.p,
                                                 h->aov.as<char>() + count * 16, p->aperture, p->focusDistance, p->maxRadius, h->lens.p, frame,
                                                 h->stream);
    if (le != hipSuccess)
        return failHip(le, "lens kernel launch");
    *out = Image{frame, false};
    return KAJO_OK;
}

} // namespace

extern "C" {

void kajo_hip_default_lens_params(KajoLensParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->aperture = 0.01f;
    p->focusDistance = 10.0f;
    p->maxRadius = KAJO_LENS_MAX_RADIUS;
}

int kajo_hip_lens(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                  float* radiance)
{
    // (every refusal before any device work: the despeckle parameters, the stage's own, the denoiser's, then the handle)
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if ((rc = checkLens(lens)))
        return rc;
    if (denoise && (rc = checkDenoise(h, denoise)))
        return rc;
    if ((rc = checkLensHandle(h)))
        return rc;
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    if ((rc = chainImage(h, despeckle, denoise, nullptr, &img)))
        return rc;
    if ((rc = lensImage(h, lens, img, &img)))
        return rc;
    if (img.fromTiles) {
        // (a copy of the accumulation: the composed frame, as kajo_hip_read_radiance)
        if ((rc = composeOwn(h)))
            return rc;
        img = Image{h->frame.p, false};
    }
    if (radiance)
        HIP_TRY(hipMemcpyAsync(radiance, img.src, (size_t)h->W * h->H * 16, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_lens_coc(kajo_hip_t h, const KajoLensParams* lens, float* radius, float* depth)
{
    int rc = checkLens(lens);
    if (rc)
        return rc;
    if ((rc = checkLensHandle(h)))
        return rc;
    if ((rc = bind(h)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->lens.ensure(lensScratchBytes(h)));
    hipError_t le = (hipError_t)kajo_lens_coc_launch(&h->map, h->aov.p, h->aov.as<char>() + count * 16, lens->aperture, lens->focusDistance,
                                                     lens->maxRadius, h->lens.p, h->stream);
    if (le != hipSuccess)
        return failHip(le, "lens kernel launch");
    if (radius)
        HIP_TRY(hipMemcpyAsync(radius, h->lens.p, count * 4, hipMemcpyDeviceToHost, h->stream));
    if (depth)
        HIP_TRY(hipMemcpyAsync(depth, h->lens.as<float>() + kajo_lens_plane(h->W, h->H), count * 4, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_lens_depth_at(kajo_hip_t h, int x, int y, float* z)
{
    if (!h || !z)
        return fail(KAJO_E_INVALID, "null argument");
    if (x < 0 || y < 0 || x >= h->W || y >= h->H)
        return fail(KAJO_E_INVALID, "the pixel is outside the frame");
    int rc = checkLensHandle(h);
    if (rc)
        return rc;
    if ((rc = bind(h)))
        return rc;
    const size_t count = (size_t)h->W * h->H, at = (size_t)y * h->W + x;
    float a = 0.0f, b = 0.0f; // A.w (hits) and B.w (depth) of the pixel
    HIP_TRY(hipMemcpyAsync(&a, h->aov.as<float>() + at * 4 + 3, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&b, h->aov.as<float>() + (count + at) * 4 + 3, 4, hipMemcpyDeviceToHost, h->stream));
    if ((rc = kajo_hip_wait(h)))
        return rc;
    // (one IEEE float32 division, as the kernel's)
    *z = std::numeric_limits<float>::infinity();
    if (a > 0.0f) {
        const float q = b / a;
        if (std::isfinite(q) && q > 0.0f)
            *z = q;
    }
    return KAJO_OK;
}

int kajo_hip_present_lens_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                                const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                uint32_t* argb8, KajoMeterResult* result)
{
    if (!lens)
        return kajo_hip_present_local_argb8(h, despeckle, denoise, g, local, meter, tone, argb8, result);
    // (every refusal before any device work: despeckle, lens, glare, local, meter, tone, the denoiser's, then the handle)
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if ((rc = checkLens(lens)))
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    if (local && (rc = checkLocal(local)))
        return rc;
    if (meter && (rc = checkMeter(meter)))
        return rc;
    ToneArgs t{};
    if ((rc = toneArgsOf(tone, &t)))
        return rc;
    if (meter && (tone->flags & KAJO_TONE_AUTO_EXPOSURE))
        return fail(KAJO_E_INVALID, "metered exposure and the tone parameters' automatic exposure are two automatic exposures: give one");
    if (denoise && (rc = checkDenoise(h, denoise)))
        return rc;
    if ((rc = checkLensHandle(h)))
        return rc;
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->argb.ensure(count * 4));
    if ((rc = chainImage(h, despeckle, denoise, nullptr, &img)))
        return rc;
    if ((rc = lensImage(h, lens, img, &img)))
        return rc;
    if (g && (rc = glareImage(h, g, img, &img)))
        return rc;
    if (local && (rc = localImage(h, local, img, &img)))
        return rc;
    // (the meter measures the frame the tone kernels are handed)
    if (meter && (rc = meterAndPatch(h, img, meter, tone, result, &t)))
        return rc;
    if ((rc = toneLaunch(h, img, t, h->argb.p)))
        return rc;
    if (argb8)
        HIP_TRY(hipMemcpyAsync(argb8, h->argb.p, count * 4, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

} // extern "C"

namespace
{

// The refusals of KajoViewParams that need no handle (KAJO_E_INVALID), in the header's order
int checkView(const KajoViewParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null view parameters");
    if (!(std::isfinite(p->x0) && std::isfinite(p->y0) && std::isfinite(p->x1) && std::isfinite(p->y1)))
        return fail(KAJO_E_INVALID, "view rectangle edges must be finite");
    const bool whole = p->x0 == 0.0f && p->y0 == 0.0f && p->x1 == 0.0f && p->y1 == 0.0f;
    if (!whole && !(0.0f <= p->x0 && p->x0 < p->x1 && 0.0f <= p->y0 && p->y0 < p->y1))
        return fail(KAJO_E_INVALID, "view rectangle must satisfy 0 <= x0 < x1 and 0 <= y0 < y1");
    if (p->outW < 1 || p->outW > KAJO_VIEW_MAX_OUT || p->outH < 1 || p->outH > KAJO_VIEW_MAX_OUT)
        return fail(KAJO_E_INVALID, "view output size must be in [1, 16384]");
    if (!whole && (((double)p->x1 - p->x0) / p->outW > KAJO_VIEW_MAX_SCALE || ((double)p->y1 - p->y0) / p->outH > KAJO_VIEW_MAX_SCALE))
        return fail(KAJO_E_INVALID, "view minification must be at most 64");
    if (p->filter > KAJO_VIEW_LANCZOS3)
        return fail(KAJO_E_INVALID, "unknown view filter");
    if (p->flags)
        return fail(KAJO_E_INVALID, "unknown view flag");
    return KAJO_OK;
}

struct ViewRect
{
    double x0, y0, x1, y1;
    bool copy; // the copy case: the whole frame at its own size
};

// ... and those that need the frame's size: last of all, behind the null handle
int checkViewHandle(kajo_hip_t h, const KajoViewParams* p, ViewRect* r)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    const bool whole = p->x0 == 0.0f && p->y0 == 0.0f && p->x1 == 0.0f && p->y1 == 0.0f;
    *r = ViewRect{p->x0, p->y0, whole ? (double)h->W : (double)p->x1, whole ? (double)h->H : (double)p->y1, false};
    if (r->x1 > h->W || r->y1 > h->H)
        return fail(KAJO_E_INVALID, "view rectangle must lie inside the frame");
    if ((r->x1 - r->x0) / p->outW > KAJO_VIEW_MAX_SCALE || (r->y1 - r->y0) / p->outH > KAJO_VIEW_MAX_SCALE)
        return fail(KAJO_E_INVALID, "view minification must be at most 64");
    r->copy = p->outW == h->W && p->outH == h->H && r->x0 == 0.0 && r->y0 == 0.0 && r->x1 == h->W && r->y1 == h->H;
    return KAJO_OK;
}

hipError_t growBuffer(DeviceBuffer& b, size_t* have, size_t want)
{
    if (b && *have >= want)
        return hipSuccess;
    *have = 0;
    hipError_t e = b.alloc(want); // (hipFree of the smaller one waits for the device: nothing in flight reads it after)
    if (e == hipSuccess)
        *have = want;
    return e;
}

// Form the weight rows of *p and upload them with the tables, unless they are the last call's. One block: lin[256], thresholds[255 + 1
// pad], firstX / countX [outW], wxT [strideX][outW] (tap-major: view.hip), firstY / countY [outH], wy [outH][strideY].
int viewPlan(KajoHip* h, const KajoViewParams* p, const ViewRect& r)
{
    if (h->viewPlanned && std::memcmp(&h->viewLast, p, sizeof *p) == 0)
        return KAJO_OK;
    h->viewPlanned = false;
    kajo::ViewAxis ax, ay;
    if (!kajo::viewAxis(h->W, r.x0, r.x1, p->outW, p->filter, &ax) || !kajo::viewAxis(h->H, r.y0, r.y1, p->outH, p->filter, &ay))
        return fail(KAJO_E_INVALID, "view row longer than 384 taps");
    auto& pl = h->viewPlan;
    size_t at = 512 * 4;
    pl.firstX = at, at += (size_t)p->outW * 4;
    pl.countX = at, at += (size_t)p->outW * 4;
    pl.wx = at, at += (size_t)p->outW * ax.stride * 4;
    pl.firstY = at, at += (size_t)p->outH * 4;
    pl.countY = at, at += (size_t)p->outH * 4;
    pl.wy = at, at += (size_t)p->outH * ay.stride * 4;
    pl.strideX = ax.stride;
    pl.strideY = ay.stride;
    pl.row0 = ay.lo;
    pl.rows = ay.hi - ay.lo;
    if (!h->viewUploaded)
        HIP_TRY(hipEventCreateWithFlags(&h->viewUploaded, hipEventDisableTiming));
    else
        HIP_TRY(hipEventSynchronize(h->viewUploaded)); // (the copy before this one has left the staging block; kernels are not waited for)
    if (h->viewStagingBytes < at) {
        if (h->viewStaging)
            (void)hipHostFree(h->viewStaging);
        h->viewStaging = nullptr;
        h->viewStagingBytes = 0;
        HIP_TRY(hipHostMalloc(&h->viewStaging, at, hipHostMallocDefault));
        h->viewStagingBytes = at;
    }
    HIP_TRY(growBuffer(h->viewRows, &h->viewRowsBytes, at));
    char* host = static_cast<char*>(h->viewStaging);
    float* tables = reinterpret_cast<float*>(host);
    kajo::viewTables(tables, tables + 256);
    tables[511] = tables[510]; // (the pad: staged by the kernel, never compared)
    std::memcpy(host + pl.firstX, ax.first.data(), (size_t)p->outW * 4);
    std::memcpy(host + pl.countX, ax.count.data(), (size_t)p->outW * 4);
    float* wxT = reinterpret_cast<float*>(host + pl.wx);
    for (int i = 0; i < p->outW; i++)
        for (int k = 0; k < ax.stride; k++)
            wxT[(size_t)k * p->outW + i] = ax.weights[(size_t)i * ax.stride + k];
    std::memcpy(host + pl.firstY, ay.first.data(), (size_t)p->outH * 4);
    std::memcpy(host + pl.countY, ay.count.data(), (size_t)p->outH * 4);
    std::memcpy(host + pl.wy, ay.weights.data(), (size_t)p->outH * ay.stride * 4);
    HIP_TRY(hipMemcpyAsync(h->viewRows.p, host, at, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->viewUploaded, h->stream));
    h->viewLast = *p;
    h->viewPlanned = true;
    return KAJO_OK;
}

// Enqueue the stage: src (device, W x H words) -> dst (device, outW x outH words). Checked by checkView and checkViewHandle, device
// bound. The copy case launches nothing.
int viewImage(KajoHip* h, const KajoViewParams* p, const ViewRect& r, const void* src, void* dst)
{
    if (r.copy) {
        if (src != dst)
            HIP_TRY(hipMemcpyAsync(dst, src, (size_t)h->W * h->H * 4, hipMemcpyDeviceToDevice, h->stream));
        return KAJO_OK;
    }
    int rc = viewPlan(h, p, r);
    if (rc)
        return rc;
    const auto& pl = h->viewPlan;
    HIP_TRY(growBuffer(h->viewMid, &h->viewMidBytes, (size_t)p->outW * pl.rows * 16));
    const char* rows = h->viewRows.as<char>();
    hipError_t le = (hipError_t)kajo_view_launch(src, h->W, rows, rows + pl.firstX, rows + pl.countX, rows + pl.wx, pl.strideX, rows + pl.firstY,
                                                 rows + pl.countY, rows + pl.wy, pl.strideY, p->outW, p->outH, pl.row0, pl.rows, h->viewMid.p, dst,
                                                 h->stream);
    if (le != hipSuccess)
        return failHip(le, "view kernel launch");
    return KAJO_OK;
}

// the refusals of the view chain calls in front of the denoiser's and the handle's: despeckle, lens, glare, local, meter, tone, view
int checkViewChain(const KajoDespeckleParams* despeckle, const KajoLensParams* lens, const KajoGlareParams* g, const KajoLocalParams* local,
                   const KajoMeterParams* meter, const KajoToneParams* tone, const KajoViewParams* view)
{
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if (lens && (rc = checkLens(lens)))
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    if (local && (rc = checkLocal(local)))
        return rc;
    if (meter && (rc = checkMeter(meter)))
        return rc;
    ToneArgs t{};
    if ((rc = toneArgsOf(tone, &t)))
        return rc;
    if (meter && (tone->flags & KAJO_TONE_AUTO_EXPOSURE))
        return fail(KAJO_E_INVALID, "metered exposure and the tone parameters' automatic exposure are two automatic exposures: give one");
    return checkView(view);
}

} // namespace

extern "C" {

void kajo_hip_default_view_params(KajoViewParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->filter = KAJO_VIEW_AREA;
}

int kajo_hip_view_weights(int32_t srcN, double a0, double a1, int32_t outN, uint32_t filter, int32_t* first, int32_t* count, float* weights,
                          size_t capacity)
{
    if (!kajo::viewAxisValid(srcN, a0, a1, outN, filter))
        return fail(KAJO_E_INVALID, "invalid view axis");
    kajo::ViewAxis ax;
    if (!kajo::viewAxis(srcN, a0, a1, outN, filter, &ax))
        return fail(KAJO_E_INVALID, "view row longer than 384 taps");
    if (first || count || weights) {
        if (!first || !count || !weights)
            return fail(KAJO_E_INVALID, "null argument");
        if (capacity < ax.weights.size())
            return fail(KAJO_E_INVALID, "weights array too small");
        std::memcpy(first, ax.first.data(), ax.first.size() * sizeof(int32_t));
        std::memcpy(count, ax.count.data(), ax.count.size() * sizeof(int32_t));
        std::memcpy(weights, ax.weights.data(), ax.weights.size() * sizeof(float));
    }
    return (int)ax.weights.size();
}

void kajo_hip_view_tables(float lin[256], float thresholds[255])
{
    kajo::viewTables(lin, thresholds);
}

int kajo_hip_view_argb8(kajo_hip_t h, const KajoViewParams* view, const uint32_t* src, uint32_t* dst)
{
    int rc = checkView(view);
    if (rc)
        return rc;
    ViewRect r{};
    if ((rc = checkViewHandle(h, view, &r)))
        return rc;
    if (!src || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    if ((rc = bind(h)))
        return rc;
    const size_t count = (size_t)h->W * h->H, outBytes = (size_t)view->outW * view->outH * 4;
    HIP_TRY(h->viewIn.ensure(count * 4));
    HIP_TRY(growBuffer(h->viewOut, &h->viewOutBytes, outBytes));
    HIP_TRY(hipMemcpyAsync(h->viewIn.p, src, count * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = viewImage(h, view, r, h->viewIn.p, h->viewOut.p)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dst, h->viewOut.p, outBytes, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_present_view_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                                const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                const KajoViewParams* view, uint32_t* argb8, KajoMeterResult* result)
{
    if (!view)
        return kajo_hip_present_lens_argb8(h, despeckle, denoise, lens, g, local, meter, tone, argb8, result);
    // (every refusal before any device work: the stages' parameters, the view's, the denoiser's, the handle, the view against the frame)
    int rc = checkViewChain(despeckle, lens, g, local, meter, tone, view);
    if (rc)
        return rc;
    if (denoise && (rc = checkDenoise(h, denoise)))
        return rc;
    ViewRect r{};
    if ((rc = checkViewHandle(h, view, &r)))
        return rc;
    // the chain's image into the handle's ARGB8 frame (the call reads nothing back), then the stage
    if ((rc = kajo_hip_present_lens_argb8(h, despeckle, denoise, lens, g, local, meter, tone, nullptr, result)))
        return rc;
    const size_t outBytes = (size_t)view->outW * view->outH * 4;
    HIP_TRY(growBuffer(h->viewOut, &h->viewOutBytes, outBytes));
    if ((rc = viewImage(h, view, r, h->argb.p, h->viewOut.p)))
        return rc;
    if (argb8)
        HIP_TRY(hipMemcpyAsync(argb8, h->viewOut.p, outBytes, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_present_view_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                                const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                                const KajoViewParams* view, void* dst, KajoMeterResult* result)
{
    if (!view)
        return kajo_hip_present_local_gathered_argb8_device(h, gathered, despeckle, g, local, meter, tone, dst, result);
    int rc = checkViewChain(despeckle, nullptr, g, local, meter, tone, view);
    if (rc)
        return rc;
    ViewRect r{};
    if ((rc = checkViewHandle(h, view, &r)))
        return rc;
    if (!dst)
        return fail(KAJO_E_INVALID, "null argument");
    if ((rc = bind(h)))
        return rc;
    if (r.copy)
        return kajo_hip_present_local_gathered_argb8_device(h, gathered, despeckle, g, local, meter, tone, dst, result);
    HIP_TRY(h->viewIn.ensure((size_t)h->W * h->H * 4));
    if ((rc = kajo_hip_present_local_gathered_argb8_device(h, gathered, despeckle, g, local, meter, tone, h->viewIn.p, result)))
        return rc;
    return viewImage(h, view, r, h->viewIn.p, dst);
}

} // extern "C"

namespace
{

static_assert(sizeof(KajoGradeOp) == 48 && sizeof(KajoGradeRegion) == 128 && sizeof(KajoGradeParams) == 576, "include/kajo_hip.h states the sizes");

// the parameter block grade.hip reads (its GradeBlock): the global op, then the regions', twelve floats each
struct GradeOpWords
{
    float slope[3], offset[3], power[3], saturation, amount, pad;
};
constexpr size_t kGradeBlockBytes = (1 + KAJO_GRADE_MAX_REGIONS) * sizeof(GradeOpWords);
constexpr size_t kGradeMaxBitsetBytes = 64 * 1024; // the regions' bitsets are staged in LDS: kajo_grade_launch

int checkGradeOp(const KajoGradeOp& op)
{
    for (int c = 0; c < 3; c++) {
        if (!(std::isfinite(op.slope[c]) && op.slope[c] >= 0.0f && op.slope[c] <= 65536.0f))
            return fail(KAJO_E_INVALID, "grade slope must be finite and in [0, 65536]");
        if (!(std::isfinite(op.offset[c]) && std::fabs(op.offset[c]) <= 65536.0f))
            return fail(KAJO_E_INVALID, "grade offset must be finite and in [-65536, 65536]");
        if (!(std::isfinite(op.power[c]) && op.power[c] >= 0.125f && op.power[c] <= 8.0f))
            return fail(KAJO_E_INVALID, "grade power must be finite and in [1/8, 8]");
    }
    if (!(std::isfinite(op.saturation) && op.saturation >= 0.0f && op.saturation <= 4.0f))
        return fail(KAJO_E_INVALID, "grade saturation must be finite and in [0, 4]");
    for (float r : op.reserved)
        if (r != 0.0f)
            return fail(KAJO_E_INVALID, "grade reserved fields must be 0");
    return KAJO_OK;
}

// The refusals of KajoGradeParams (KAJO_E_INVALID), before any device work and before the handle is looked at
int checkGrade(const KajoGradeParams* p)
{
    if (!p)
        return fail(KAJO_E_INVALID, "null grade parameters");
    int rc = checkGradeOp(p->global);
    if (rc)
        return rc;
    if (p->nRegions < 0 || p->nRegions > KAJO_GRADE_MAX_REGIONS)
        return fail(KAJO_E_INVALID, "grade regions must number 0 to 4");
    if (p->flags)
        return fail(KAJO_E_INVALID, "unknown grade flag");
    if (p->reserved[0] || p->reserved[1])
        return fail(KAJO_E_INVALID, "grade reserved fields must be 0");
    for (int k = 0; k < p->nRegions; k++) {
        const KajoGradeRegion& r = p->regions[k];
        if ((rc = checkGradeOp(r.op)))
            return rc;
        if (r.n < 1 || r.n > KAJO_GRADE_REGION_OBJECTS)
            return fail(KAJO_E_INVALID, "a grade region selects 1 to 16 objects");
        for (int i = 0; i < r.n; i++)
            if (r.objects[i] < 0)
                return fail(KAJO_E_INVALID, "object id out of range: 0 (the background) .. the number of planes and spheres");
        if (!(std::isfinite(r.amount) && r.amount >= 0.0f && r.amount <= 1.0f))
            return fail(KAJO_E_INVALID, "grade region amount must be finite and in [0, 1]");
        if (r.reserved[0] || r.reserved[1])
            return fail(KAJO_E_INVALID, "grade reserved fields must be 0");
    }
    return KAJO_OK;
}

bool gradeIsIdentity(const KajoGradeParams* p)
{
    return p->nRegions == 0 && kajo::gradeOpIsDefault(p->global);
}

// ... and of the handle. wholeFrame: the call works on the handle's own frame (not on gathered tile buffers). With regions the state
// follows kajo_hip_matte_mask's rules; without them the handle needs no AOVs.
int checkGradeHandle(kajo_hip_t h, const KajoGradeParams* p, bool wholeFrame)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    if (p->nRegions > 0) {
        int rc = matteReady(h);
        if (rc)
            return rc;
    }
    if (wholeFrame || p->nRegions > 0) {
        if (h->passesDone < 1)
            return fail(KAJO_E_STATE, "nothing rendered yet");
        if (wholeFrame && h->map.tileCount != 1 && !h->frameValid)
            return fail(KAJO_E_STATE, "whole-frame output needs kajo_hip_compose() when tileCount > 1");
    }
    if (p->nRegions > 0) {
        const int nObjects = h->staged.nPlanes + h->staged.nSpheres;
        for (int k = 0; k < p->nRegions; k++)
            for (int i = 0; i < p->regions[k].n; i++)
                if (p->regions[k].objects[i] > nObjects)
                    return fail(KAJO_E_INVALID, "object id out of range: 0 (the background) .. the number of planes and spheres");
        if ((size_t)p->nRegions * matteBitsetWords(h) * sizeof(uint32_t) > kGradeMaxBitsetBytes)
            return fail(KAJO_E_INVALID, "grade regions: the scene has too many objects for " + std::to_string(p->nRegions) +
                                            " regions (their id bitsets must fit 64 KiB: 524287 objects with one region, 131071 with four)");
    }
    return KAJO_OK;
}

// Form the parameter block of *p and, with regions, their bitsets, and upload them, unless they are the last call's
// (the upload is ordered on the stream it was enqueued on, as the view's cached rows are: a caller that changes the handle's stream with
// kajo_hip_set_stream between two calls with equal parameters orders the two streams itself, as for every other buffer of the handle)
int gradePlan(KajoHip* h, const KajoGradeParams* p)
{
    if (h->gradePlanned && std::memcmp(&h->gradeLast, p, sizeof *p) == 0)
        return KAJO_OK;
    h->gradePlanned = false;
    if (kajo_grade_block_bytes() != kGradeBlockBytes)
        return fail(KAJO_E_INVALID, "grade parameter block layout mismatch");
    const size_t words = matteBitsetWords(h);
    const size_t bytes = kGradeBlockBytes + KAJO_GRADE_MAX_REGIONS * words * sizeof(uint32_t);
    if (!h->gradeUploaded)
        HIP_TRY(hipEventCreateWithFlags(&h->gradeUploaded, hipEventDisableTiming));
    else
        HIP_TRY(hipEventSynchronize(h->gradeUploaded)); // (the copy before this one has left the staging block; kernels are not waited for)
    if (!h->gradeStaging)
        HIP_TRY(hipHostMalloc(&h->gradeStaging, bytes, hipHostMallocDefault));
    HIP_TRY(h->gradeBlock.ensure(bytes));
    std::memset(h->gradeStaging, 0, bytes);
    GradeOpWords* ops = static_cast<GradeOpWords*>(h->gradeStaging);
    uint32_t* bits = reinterpret_cast<uint32_t*>(static_cast<char*>(h->gradeStaging) + kGradeBlockBytes);
    for (int k = 0; k <= p->nRegions; k++) {
        const KajoGradeOp& op = k == 0 ? p->global : p->regions[k - 1].op;
        std::memcpy(ops[k].slope, op.slope, sizeof op.slope);
        std::memcpy(ops[k].offset, op.offset, sizeof op.offset);
        std::memcpy(ops[k].power, op.power, sizeof op.power);
        ops[k].saturation = op.saturation;
        ops[k].amount = k == 0 ? 1.0f : p->regions[k - 1].amount;
        if (k > 0)
            for (int i = 0; i < p->regions[k - 1].n; i++) {
                const int32_t id = p->regions[k - 1].objects[i]; // (0 .. nObjects: checkGradeHandle)
                bits[(size_t)(k - 1) * words + ((size_t)id >> 5)] |= 1u << (id & 31);
            }
    }
    HIP_TRY(hipMemcpyAsync(h->gradeBlock.p, h->gradeStaging, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->gradeUploaded, h->stream));
    h->gradeLast = *p;
    h->gradePlanned = true;
    return KAJO_OK;
}

// Enqueue the grade of an image (tiles through h->map's geometry, or a row-major frame): *out = the row-major frame in the stage's
// scratch that holds the result -- or the image itself in the identity case. Checked by checkGrade and checkGradeHandle, device bound.
int gradeImage(KajoHip* h, const KajoGradeParams* p, Image img, Image* out)
{
    if (gradeIsIdentity(p)) {
        *out = img;
        return KAJO_OK;
    }
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->grade.ensure(count * 16));
    int rc = gradePlan(h, p);
    if (rc)
        return rc;
    const bool regions = p->nRegions > 0;
    const size_t tableWords = count * KAJO_MATTE_SLOTS * 4;
    hipError_t le = (hipError_t)kajo_grade_launch(img.src, &h->map, img.fromTiles ? 1 : 0, (float)h->passesDone, h->gradeBlock.p, p->nRegions,
                                                  regions ? h->matte.p : nullptr, regions ? h->matte.as<char>() + tableWords : nullptr,
                                                  (unsigned)matteBitsetWords(h), (unsigned)(h->staged.nPlanes + h->staged.nSpheres),
                                                  (float)aovSamples(h), h->grade.p, h->stream);
    if (le != hipSuccess)
        return failHip(le, "grade kernel launch");
    *out = Image{h->grade.p, false};
    return KAJO_OK;
}

// the refusals of the grade chain calls in front of the denoiser's and the handle's: despeckle, grade, lens, glare, local, meter, tone,
// view; -> *t the tone kernels' arguments
int checkGradeChain(const KajoDespeckleParams* despeckle, const KajoGradeParams* grade, const KajoLensParams* lens, const KajoGlareParams* g,
                    const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone, const KajoViewParams* view, ToneArgs* t)
{
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if ((rc = checkGrade(grade)))
        return rc;
    if (lens && (rc = checkLens(lens)))
        return rc;
    if (g && (rc = checkGlare(g)))
        return rc;
    if (local && (rc = checkLocal(local)))
        return rc;
    if (meter && (rc = checkMeter(meter)))
        return rc;
    if ((rc = toneArgsOf(tone, t)))
        return rc;
    if (meter && (tone->flags & KAJO_TONE_AUTO_EXPOSURE))
        return fail(KAJO_E_INVALID, "metered exposure and the tone parameters' automatic exposure are two automatic exposures: give one");
    return view ? checkView(view) : KAJO_OK;
}

} // namespace

extern "C" {

void kajo_hip_default_grade_params(KajoGradeParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    KajoGradeOp op{};
    for (int c = 0; c < 3; c++)
        op.slope[c] = op.power[c] = 1.0f;
    op.saturation = 1.0f;
    p->global = op;
    for (KajoGradeRegion& r : p->regions) {
        r.op = op;
        r.amount = 1.0f;
    }
}

int kajo_hip_grade_pixels(const KajoGradeParams* p, const float* rgb, const float* masks, int64_t n, float* out)
{
    int rc = checkGrade(p);
    if (rc)
        return rc;
    if (n < 0 || (n > 0 && (!rgb || !out || (p->nRegions > 0 && !masks))))
        return fail(KAJO_E_INVALID, "null argument");
    const bool identity = gradeIsIdentity(p);
    for (int64_t i = 0; i < n; i++) {
        const float* m = rgb + 3 * i;
        float* o = out + 3 * i;
        if (identity || !(kajo::gradeFinite(m[0]) && kajo::gradeFinite(m[1]) && kajo::gradeFinite(m[2]))) {
            std::memmove(o, m, 3 * sizeof(float));
            continue;
        }
        float c[3];
        kajo::gradeOp(p->global, m, c);
        for (int k = 0; k < p->nRegions; k++)
            kajo::gradeRegion(p->regions[k].op, p->regions[k].amount, masks[i * p->nRegions + k], c);
        std::memcpy(o, c, sizeof c);
    }
    return KAJO_OK;
}

namespace
{
// g normalised to luminance 1, rounded to float32
void gradeGainsOut(double r, double g, double b, float gains[3])
{
    const double y = 0.2126 * r + 0.7152 * g + 0.0722 * b;
    gains[0] = (float)(r / y);
    gains[1] = (float)(g / y);
    gains[2] = (float)(b / y);
}
} // namespace

int kajo_hip_grade_white_balance(double kelvin, double tint, float gains[3])
{
    if (!gains)
        return fail(KAJO_E_INVALID, "null argument");
    if (!(std::isfinite(kelvin) && kelvin >= 1667.0 && kelvin <= 25000.0))
        return fail(KAJO_E_INVALID, "white balance temperature must be in [1667, 25000] kelvin");
    if (!(std::isfinite(tint) && std::fabs(tint) <= 1.0))
        return fail(KAJO_E_INVALID, "white balance tint must be in [-1, 1]");
    const double T = kelvin, T2 = T * T, T3 = T2 * T;
    const double x = T <= 4000.0 ? -0.2661239e9 / T3 - 0.2343589e6 / T2 + 0.8776956e3 / T + 0.179910
                                 : -3.0258469e9 / T3 + 2.1070379e6 / T2 + 0.2226347e3 / T + 0.240390;
    const double x2 = x * x, x3 = x2 * x;
    const double y = T <= 2222.0   ? -1.1063814 * x3 - 1.34811020 * x2 + 2.18555832 * x - 0.20219683
                     : T <= 4000.0 ? -0.9549476 * x3 - 1.37418593 * x2 + 2.09137015 * x - 0.16748867
                                   : 3.0817580 * x3 - 5.87338670 * x2 + 3.75112997 * x - 0.37001483;
    const double X = x / y, Y = 1.0, Z = (1.0 - x - y) / y;
    const double rgb[3] = {3.2404542 * X - 1.5371385 * Y - 0.4985314 * Z, -0.9692660 * X + 1.8760108 * Y + 0.0415560 * Z,
                           0.0556434 * X - 0.2040259 * Y + 1.0572252 * Z};
    for (double c : rgb)
        if (!(c > 1e-3))
            return fail(KAJO_E_INVALID, "white balance temperature is outside sRGB");
    gradeGainsOut(1.0 / rgb[0], (1.0 / rgb[1]) * std::exp2(tint), 1.0 / rgb[2], gains);
    return KAJO_OK;
}

int kajo_hip_grade_neutral(const float rgb[3], float gains[3])
{
    if (!rgb || !gains)
        return fail(KAJO_E_INVALID, "null argument");
    for (int c = 0; c < 3; c++)
        if (!(std::isfinite(rgb[c]) && rgb[c] > 0.0f))
            return fail(KAJO_E_INVALID, "a neutral needs three finite positive channels");
    const double r = rgb[0], g = rgb[1], b = rgb[2];
    const double Y = 0.2126 * r + 0.7152 * g + 0.0722 * b;
    gradeGainsOut(Y / r, Y / g, Y / b, gains);
    return KAJO_OK;
}

int kajo_hip_grade(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                   float* radiance)
{
    // (every refusal before any device work: the despeckle parameters, the stage's own, the denoiser's, then the handle)
    int rc;
    if (despeckle && (rc = checkDespeckle(despeckle)))
        return rc;
    if ((rc = checkGrade(grade)))
        return rc;
    if (denoise && (rc = checkDenoise(h, denoise)))
        return rc;
    if ((rc = checkGradeHandle(h, grade, true)))
        return rc;
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    if ((rc = chainImage(h, despeckle, denoise, nullptr, &img)))
        return rc;
    if ((rc = gradeImage(h, grade, img, &img)))
        return rc;
    if (img.fromTiles) {
        // (a copy of the accumulation: the composed frame, as kajo_hip_read_radiance)
        if ((rc = composeOwn(h)))
            return rc;
        img = Image{h->frame.p, false};
    }
    if (radiance)
        HIP_TRY(hipMemcpyAsync(radiance, img.src, (size_t)h->W * h->H * 16, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_present_grade_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                                 const KajoLensParams* lens, const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                                 const KajoToneParams* tone, const KajoViewParams* view, uint32_t* argb8, KajoMeterResult* result)
{
    if (!grade)
        return kajo_hip_present_view_argb8(h, despeckle, denoise, lens, g, local, meter, tone, view, argb8, result);
    // (every refusal before any device work: the stages' parameters, the denoiser's, the handle, the view against the frame)
    ToneArgs t{};
    int rc = checkGradeChain(despeckle, grade, lens, g, local, meter, tone, view, &t);
    if (rc)
        return rc;
    if (denoise && (rc = checkDenoise(h, denoise)))
        return rc;
    if ((rc = checkGradeHandle(h, grade, true)))
        return rc;
    if (lens && (rc = checkLensHandle(h)))
        return rc;
    ViewRect r{};
    if (view && (rc = checkViewHandle(h, view, &r)))
        return rc;
    Image img;
    if ((rc = imageOf(h, false, nullptr, &img)))
        return rc;
    const size_t count = (size_t)h->W * h->H;
    HIP_TRY(h->argb.ensure(count * 4));
    if ((rc = chainImage(h, despeckle, denoise, nullptr, &img)))
        return rc;
    if ((rc = gradeImage(h, grade, img, &img)))
        return rc;
    if (lens && (rc = lensImage(h, lens, img, &img)))
        return rc;
    if (g && (rc = glareImage(h, g, img, &img)))
        return rc;
    if (local && (rc = localImage(h, local, img, &img)))
        return rc;
    // (the meter measures the frame the tone kernels are handed)
    if (meter && (rc = meterAndPatch(h, img, meter, tone, result, &t)))
        return rc;
    if ((rc = toneLaunch(h, img, t, h->argb.p)))
        return rc;
    if (!view) {
        if (argb8)
            HIP_TRY(hipMemcpyAsync(argb8, h->argb.p, count * 4, hipMemcpyDeviceToHost, h->stream));
        return kajo_hip_wait(h);
    }
    const size_t outBytes = (size_t)view->outW * view->outH * 4;
    HIP_TRY(growBuffer(h->viewOut, &h->viewOutBytes, outBytes));
    if ((rc = viewImage(h, view, r, h->argb.p, h->viewOut.p)))
        return rc;
    if (argb8)
        HIP_TRY(hipMemcpyAsync(argb8, h->viewOut.p, outBytes, hipMemcpyDeviceToHost, h->stream));
    return kajo_hip_wait(h);
}

int kajo_hip_present_grade_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle,
                                                 const KajoGradeParams* grade, const KajoGlareParams* g, const KajoLocalParams* local,
                                                 const KajoMeterParams* meter, const KajoToneParams* tone, const KajoViewParams* view, void* dst,
                                                 KajoMeterResult* result)
{
    if (!grade)
        return kajo_hip_present_view_gathered_argb8_device(h, gathered, despeckle, g, local, meter, tone, view, dst, result);
    ToneArgs t{};
    int rc = checkGradeChain(despeckle, grade, nullptr, g, local, meter, tone, view, &t);
    if (rc)
        return rc;
    if (grade->nRegions > 0)
        return fail(KAJO_E_INVALID, "grade regions need the whole frame's coverage tables: kajo_hip_present_grade_argb8 on the root");
    if (!h || !dst)
        return fail(KAJO_E_INVALID, "null argument");
    ViewRect r{};
    if (view && (rc = checkViewHandle(h, view, &r)))
        return rc;
    Image img;
    if ((rc = imageOf(h, true, gathered, &img)))
        return rc;
    if ((rc = chainImage(h, despeckle, nullptr, nullptr, &img)))
        return rc;
    if ((rc = gradeImage(h, grade, img, &img)))
        return rc;
    if (g && (rc = glareImage(h, g, img, &img)))
        return rc;
    if (local && (rc = localImage(h, local, img, &img))) // (one wait with KAJO_LOCAL_PIVOT_METERED: include/kajo_hip.h)
        return rc;
    if (meter && (rc = meterAndPatch(h, img, meter, tone, result, &t))) // (and one more)
        return rc;
    if (!view || r.copy)
        return toneLaunch(h, img, t, dst);
    HIP_TRY(h->viewIn.ensure((size_t)h->W * h->H * 4));
    if ((rc = toneLaunch(h, img, t, h->viewIn.p)))
        return rc;
    return viewImage(h, view, r, h->viewIn.p, dst);
}

int kajo_hip_tone_scale(kajo_hip_t h, float* scale)
{
    if (!h || !scale)
        return fail(KAJO_E_INVALID, "null argument");
    if (h->toneScaleState == 0)
        return fail(KAJO_E_STATE, "nothing tone-mapped yet");
    int rc = bind(h);
    if (rc)
        return rc;
    float s = h->toneScale;
    if (h->toneScaleState == 2)
        HIP_TRY(hipMemcpyAsync(&s, h->tone.p, sizeof s, hipMemcpyDeviceToHost, h->stream));
    if ((rc = kajo_hip_wait(h)))
        return rc;
    *scale = s;
    return KAJO_OK;
}

int kajo_hip_kat_trace(kajo_hip_t h, int n, const float* origins, const float* dirs, int32_t* objIndex, float* t,
                       float* position, float* normal, float* tangent, float* binormal)
{
    if (!h || n < 0 || !origins || !dirs || !objIndex || !t || !position || !normal || !tangent || !binormal)
        return fail(KAJO_E_INVALID, "null argument");
    // (any scene create() accepted: its hot records are within the plan's 160 KiB, and the launcher opts in above 48 KiB)
    int rc = bind(h);
    if (rc || n == 0)
        return rc;
    const std::vector<float> rays = packRays(n, origins, dirs);
    DeviceBuffer dRays, dIdx, dOut;
    HIP_TRY(dRays.alloc(rays.size() * 4));
    HIP_TRY(dIdx.alloc((size_t)n * 4));
    HIP_TRY(dOut.alloc((size_t)n * 13 * 4));
    HIP_TRY(hipMemcpyAsync(dRays.p, rays.data(), rays.size() * 4, hipMemcpyHostToDevice, h->stream));
    KatTraceArgs a;
    a.scene = h->view;
    a.rays = dRays.as<const float>();
    a.count = n;
    a.idx = dIdx.as<int32_t>();
    a.out = dOut.as<float>();
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipError_t le = (hipError_t)h->k->katTrace(&a, grid, h->lds.hotBytes, h->stream);
    if (le != hipSuccess)
        return failHip(le, "kat trace launch");
    std::vector<float> out((size_t)n * 13);
    HIP_TRY(hipMemcpyAsync(objIndex, dIdx.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(out.data(), dOut.p, out.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++) {
        t[i] = out[13 * (size_t)i];
        std::memcpy(position + 3 * i, &out[13 * (size_t)i + 1], 12);
        std::memcpy(normal + 3 * i, &out[13 * (size_t)i + 4], 12);
        std::memcpy(tangent + 3 * i, &out[13 * (size_t)i + 7], 12);
        std::memcpy(binormal + 3 * i, &out[13 * (size_t)i + 10], 12);
    }
    return KAJO_OK;
}

int kajo_hip_kat_shade(kajo_hip_t h, int n, const float* origins, const float* dirs, const uint64_t* states, float* rgb,
                       uint64_t* finalStates)
{
    if (!h || n < 0 || !origins || !dirs || !states || !rgb || !finalStates)
        return fail(KAJO_E_INVALID, "null argument");
    if (h->lds.hotBytes > 48 * 1024)
        return fail(KAJO_E_INVALID, "known-answer entry points are limited to scenes whose hot records fit 48 KiB of LDS");
    int rc = bind(h);
    if (rc || n == 0)
        return rc;
    const std::vector<float> rays = packRays(n, origins, dirs);
    DeviceBuffer dRays, dStates, dRgb, dFinal;
    HIP_TRY(dRays.alloc(rays.size() * 4));
    HIP_TRY(dStates.alloc((size_t)n * 16));
    HIP_TRY(dRgb.alloc((size_t)n * 16));
    HIP_TRY(dFinal.alloc((size_t)n * 16));
    HIP_TRY(hipMemcpyAsync(dRays.p, rays.data(), rays.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dStates.p, states, (size_t)n * 16, hipMemcpyHostToDevice, h->stream));
    RenderArgs a;
    std::memset(&a, 0, sizeof a);
    a.scene = h->view;
    a.W = a.H = 1;
    a.n = 1;
    a.S = 1.f;
    a.depthLimit = h->params.depthLimit;
    a.tileW = 64;
    a.tileH = 16;
    a.tilesX = a.tilesY = 1;
    a.tileCount = 1;
    a.katRays = dRays.as<const float>();
    a.katStates = dStates.as<const uint64_t>();
    a.katRgb = dRgb.as<float>();
    a.katFinal = dFinal.as<uint64_t>();
    a.katCount = n;
    a.stealWindow = 1;
    a.mailboxOffset = (uint32_t)((h->lds.hotBytes + 15) & ~(size_t)15);
    h->lds.fillWaveLds(a, a.mailboxOffset, false);
    const size_t ldsKat = a.mailboxOffset + 4 * (size_t)a.perWaveBytes;
    if (ldsKat > 64 * 1024)
        return fail(KAJO_E_INVALID, "known-answer entry points are limited to scenes whose hot records and wave areas fit 64 KiB of LDS");
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipError_t le = (hipError_t)h->k->katShade(&a, grid, ldsKat, h->stream);
    if (le != hipSuccess)
        return failHip(le, "kat shade launch");
    std::vector<float> out4((size_t)n * 4);
    HIP_TRY(hipMemcpyAsync(out4.data(), dRgb.p, out4.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(finalStates, dFinal.p, (size_t)n * 16, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++)
        std::memcpy(rgb + 3 * i, &out4[4 * (size_t)i], 12);
    return KAJO_OK;
}

int kajo_hip_kat_strictmath(kajo_hip_t h, int fn, int n, const float* x, const float* y, float* out)
{
    if (!h || n < 0 || !x || !y || !out)
        return fail(KAJO_E_INVALID, "null argument");
    int rc = bind(h);
    if (rc || n == 0)
        return rc;
    DeviceBuffer dx, dy, dout;
    HIP_TRY(dx.alloc((size_t)n * 4));
    HIP_TRY(dy.alloc((size_t)n * 4));
    HIP_TRY(dout.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpyAsync(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dy.p, y, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    hipError_t le = (hipError_t)kajo_kat_math_launch(fn, n, dx.p, dy.p, dout.p, h->stream);
    if (le != hipSuccess)
        return failHip(le, "kat math launch");
    HIP_TRY(hipMemcpyAsync(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return KAJO_OK;
}

int kajo_hip_kat_strictmath_sweep(kajo_hip_t h, int fn, float y, uint64_t* sums)
{
    if (!h || !sums)
        return fail(KAJO_E_INVALID, "null argument");
    if (fn < 0 || fn > 7 || fn == 5)
        return fail(KAJO_E_INVALID, "strictmath sweep: fn must be 0 sin, 1 cos, 2 asin, 3 acos, 4 pow, 6 sqrt or 7 the walk's sqrt (x / y is binary)");
    int rc = bind(h);
    if (rc)
        return rc;
    const size_t perBinade = 64, words = 512 * perBinade * 2; // kernel_strict.hip KAJO_SWEEP_BLOCKS_PER_BINADE
    DeviceBuffer dPartial;
    HIP_TRY(dPartial.alloc(words * 8));
    hipError_t le = (hipError_t)kajo_kat_math_sweep_launch(fn, y, dPartial.p, h->stream);
    if (le != hipSuccess)
        return failHip(le, "kat math sweep launch");
    std::vector<uint64_t> partial(words);
    HIP_TRY(hipMemcpyAsync(partial.data(), dPartial.p, words * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < 512; b++) {
        uint64_t A = 0, B = 0;
        for (size_t c = 0; c < perBinade; c++) {
            A += partial[2 * (b * perBinade + c)];
            B += partial[2 * (b * perBinade + c) + 1];
        }
        sums[2 * b] = A;
        sums[2 * b + 1] = B;
    }
    return KAJO_OK;
}

// Diagnostic builds only (-DKAJO_PROFILE): 28 raw block-profile words (16 block counts, 5 stamp sums, spare) behind the work counters.
extern "C" int kajo_hip_debug_profile(kajo_hip_t h, unsigned long long* out28)
{
    if (!h || !out28 || !h->counters)
        return fail(KAJO_E_INVALID, "no counters");
    int rc = kajo_hip_wait(h);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpy(out28, h->counters.as<unsigned long long>() + 4, 28 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return KAJO_OK;
}

int kajo_hip_counters(kajo_hip_t h, KajoCounters* out)
{
    if (!h || !out)
        return fail(KAJO_E_INVALID, "null argument");
    int rc = kajo_hip_wait(h);
    if (rc)
        return rc;
    std::memset(out, 0, sizeof *out);
    const int n = samplesPerAxis(h->params);
    // pixels this handle owns
    unsigned long long pixels = 0;
    for (int t = h->params.tileIndex; t < h->nTiles; t += h->params.tileCount) {
        const int tx = t % h->map.tilesX, ty = t / h->map.tilesX;
        const int w = std::min(h->map.tileW, h->W - tx * h->map.tileW);
        const int hh = std::min(h->map.tileH, h->H - ty * h->map.tileH);
        pixels += (unsigned long long)w * hh;
    }
    out->passes = (uint64_t)h->passesDone;
    out->paths = pixels * (unsigned long long)(n * n) * (unsigned long long)h->passesDone;
    out->kernelMs = h->kernelMs;
    out->launches = h->launches;
    out->tailGroups = h->lastTailGroups;
    if (h->counters) {
        unsigned long long c[4];
        HIP_TRY(hipMemcpy(c, h->counters.p, sizeof c, hipMemcpyDeviceToHost));
        out->traversals = c[0];
        out->vertices = c[1];
        out->laneSlots = c[2];
        out->shadowQueries = c[3];
        out->primitiveTests = c[0] * (unsigned long long)(h->view.nPlanes + h->view.nSpheres);
    }
    return KAJO_OK;
}

} // extern "C"
