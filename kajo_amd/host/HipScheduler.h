// HipScheduler.h -- the "-r hip" backend behind Kajo's Scheduler plugin interface.
//
// Drop-in counterpart of cpu::Scheduler (renderer/cpu/Scheduler.h:22-34, .cpp:53-85): same
// constructor shape (const scene::Scene&, Image*, Preview*), same single blocking run(). Where the
// CPU backend cuts the image into one row slice per core and renders them with std::async
// (cpu/Scheduler.cpp:32-42), this one deals fixed-size tiles round-robin to the node's GPUs, runs
// one libkajo_hip handle per GPU (include/kajo_hip.h), gathers the tile buffers to GPU 0 once per
// displayed frame (RCCL over xGMI) and resolves into Image::pixels. The scene is only read inside
// the constructor, as in the reference (cpu/Scene.cpp:29-38 copies it).
#ifndef KAJO_HIP_SCHEDULER_H
#define KAJO_HIP_SCHEDULER_H

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "Scheduler.h"
#include "kajo_hip.h" // KajoToneParams (Options::tone), KajoGlareParams (Options::glare), KajoDespeckleParams (Options::despeckle), KajoMeterParams, KajoLocalParams, KajoLensParams, KajoViewParams, KajoGradeParams, KajoEncodeParams

class Image;
class Preview;

namespace scene
{
class Scene;
}

namespace hip
{

struct Options
{
    int samplesPerPass = 32;      // m_samples, renderer/cpu/Renderer.cpp:21
    int depthLimit = 8;           // g_depthLimit, renderer/cpu/Shader.cpp:24
    uint64_t seed = 0715517;      // renderer/cpu/Random.h:43
    int passes = 0;               // stop after this many passes; 0 = until the preview closes
                                  // (16 when there is no preview: the reference never stops by itself)
    int passesPerUpdate = 0;      // passes rendered between two image/preview refreshes; 0 = automatic: everything that is
                                  // left (up to 16) without a preview, as many as fit a 30 Hz refresh with one
    int gpus = 0;                 // devices 0 .. gpus-1; 0 = every GPU the HIP runtime shows (hipGetDeviceCount), or the
                                  // number in the environment variable KAJO_HIP_GPUS when that is set -- what the
                                  // three-argument constructor (the form renderer/Main.cpp:135-142 calls) uses, so that
                                  // `renderer -r hip scene.json` tiles the frame over the whole node with no flag the
                                  // reference does not have
    // Numerics build of the kernels (include/kajo_hip.h). Exact (the default, round 5): every path takes the decisions of
    // renderer/cpu -- same hits, same random draws -- and only the products that scale its radiance are formed in the GPU's fast
    // forms: the frame is the reference's to ~1e-6 (BASELINE.json asks for per-pixel RMSE < 1e-4). Fast: hardware
    // transcendentals and contraction everywhere, 1.6 x the rate, a few paths per million decide differently (RMSE ~6e-4 on
    // spheres.json at 512 spp). Strict: the CPU oracle bit for bit. The environment variable KAJO_HIP_NUMERICS (exact | fast |
    // strict) overrides it for the three-argument constructor, which has no options.
    enum Numerics { Exact, Fast, Strict } numerics = Exact;
    bool strict = false;          // (kept from rounds 1-4) true = Numerics::Strict
    bool numericsFromEnvironment = false; // set by the three-argument constructor: KAJO_HIP_NUMERICS may choose the build
    bool counters = false;
    enum Gather { Rccl, Copy } gather = Rccl; // Copy: hipMemcpyAsync instead of RCCL (also lets
                                              // several tile owners share ONE device, for tests)
    bool sameDevice = false;      // all tile owners on device 0 (needs gather = Copy)
    bool forceGather = false;     // run the gather + compose step with ONE owner too (a one-rank communicator whose
                                  // rank sends its tile buffer to itself): the multi-GPU call sequence on a one-GPU box
    bool aov = false;             // also accumulate the first-hit albedo / normal / depth (KAJO_FLAG_AOV; readAov): one GPU only, unless aovTiled
    bool aovSpecular = false;     // ... at the first non-delta hit, through ideal mirrors and glass (KAJO_FLAG_AOV_SPECULAR); read only with aov
    bool matte = false;           // ... with the per-pixel object-coverage tables beside them (KAJO_FLAG_AOV_MATTE; readMatte, readMatteMask); read
                                  // only with aov. Off by default: every frame then takes exactly the calls it took without this field
    bool aovTiled = false;        // ... every owner keeps the AOVs (and tables) of its own tiles (KAJO_FLAG_AOV_TILED): aov on any number of GPUs. The
                                  // AOV tile buffers are gathered to GPU 0 and composed ON DEMAND, by the readers that need them (readAov, readMatte,
                                  // readMatteMask, readDenoised*, and readDisplayed / readPresented with denoise parameters), never by a refresh of
                                  // run(): the gather is two (with matte six) times the frame's bytes. Read only with aov
    // Exposure, tone curve and automatic exposure of the image run() writes (include/kajo_hip.h kajo_hip_tonemap_argb8; with one owner
    // or after the gather). The default is the identity: every frame then takes the plain resolve, exactly as without this field.
    KajoToneParams tone = {KAJO_TONE_CLAMP, 0u, 0.0f, 0.0f, 0.18f, {0.0f, 0.0f, 0.0f}};
    // Glare (bloom) in front of the tone mapping of the image run() writes (include/kajo_hip.h kajo_hip_display_argb8; with one owner or
    // after the gather). Off by default (strength 0): every frame then takes exactly the calls it takes without this field.
    KajoGlareParams glare = {6, 0u, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f, 0.0f}};
    // Despeckle (NaN / Inf repair, firefly clamp) in front of the glare and the tone mapping of the image run() writes (include/kajo_hip.h
    // kajo_hip_present_argb8; with one owner or after the gather). Off by default: every frame then takes exactly the calls it takes
    // without these fields. A flag of its own beside the parameters, because factor 0 is a setting of the stage (repair only) and
    // cannot also mean off. The defaults are written in one place, the library: whoever sets despeckleOn fills `despeckle` with
    // kajo_hip_default_despeckle_params first (all zero, as here, is refused for its rank, loudly).
    bool despeckleOn = false;
    KajoDespeckleParams despeckle = {};
    // Histogram metering between the chain and the tone curve of the image run() writes (include/kajo_hip.h
    // kajo_hip_present_metered_argb8; with one owner or after the gather): the exposure that puts `meter.percentile` of the lit pixels
    // at `meter.key`, Options::tone's exposure a compensation on top, and with KAJO_METER_AUTO_WHITE Reinhard's white. Off by default:
    // every frame then takes exactly the calls it takes without these fields. A flag beside the parameters, as for the despeckle:
    // whoever sets meterOn fills `meter` with kajo_hip_default_meter_params first (all zero, as here, is refused, loudly).
    bool meterOn = false;
    KajoMeterParams meter = {};
    // Local tone mapping between the glare and the meter of the image run() writes (include/kajo_hip.h kajo_hip_present_local_argb8; with
    // one owner or after the gather): the base layer of log luminance is compressed about `local.pivot`, the detail kept. Off by default:
    // every frame then takes exactly the calls it takes without these fields; so does one with compression 1 and detail 1, which the
    // definition makes a copy. A flag beside the parameters, as for the despeckle: whoever sets localOn fills `local` with
    // kajo_hip_default_local_params first (all zero, as here, is refused, loudly).
    bool localOn = false;
    KajoLocalParams local = {};
    // Depth of field between the denoiser and the glare of the images readPresented() hands out (include/kajo_hip.h
    // kajo_hip_present_lens_argb8): a lens blur from the depth AOV, an image-space approximation. It needs `aov`, and with more than one GPU
    // `aovTiled` (both refused at construction otherwise). Off by default: every call is then the one made without these fields. Whoever sets
    // lensOn fills `lens` with kajo_hip_default_lens_params first. lensFocusAt: the pixel to focus on (kajo_hip_lens_depth_at; a pixel that
    // is "far" is refused when the image is read); x = -1 means "use lens.focusDistance".
    bool lensOn = false;
    KajoLensParams lens = {};
    struct { int x = -1, y = -1; } lensFocusAt;
    // The view behind the tone curves of the image readViewed() hands out (include/kajo_hip.h kajo_hip_present_view_argb8): a source
    // rectangle, an output size and a filter -- crop, zoom, or the average of a supersampled render. Off by default: readViewed() is then
    // refused, and run()'s refreshes into Kajo's own Image keep the frame's size and the calls they made in either case. Whoever sets viewOn
    // fills `view` with kajo_hip_default_view_params first and names outW and outH.
    bool viewOn = false;
    KajoViewParams view = {};
    // The grade between the denoiser and the lens of the images readPresented() and readViewed() hand out (include/kajo_hip.h
    // kajo_hip_present_grade_argb8): white balance and an ASC CDL op over the frame, per-object regrades by matte. The global op works for any
    // number of GPUs (the frame is composed on the first handle); regions need `aov` and `matte`, and with more than one GPU `aovTiled`
    // (refused at construction otherwise). Off by default: every call is then the one made without these fields. Whoever sets gradeOn fills
    // `grade` with kajo_hip_default_grade_params first. gradeNeutralAt: a pixel that should be grey -- its colour in the chain's frame in
    // front of the grade gives gains (kajo_hip_grade_neutral) that are multiplied into grade.global.slope when the image is read; a pixel
    // with a channel that is not finite and positive is refused then; x = -1 means none.
    bool gradeOn = false;
    KajoGradeParams grade = {};
    struct { int x = -1, y = -1; } gradeNeutralAt;
    // The noise estimate (include/kajo_hip.h KAJO_FLAG_NOISE, kajo_hip_noise): every handle keeps the batch moments of its own tiles, and
    // at each refresh run() adds the owners' histograms of the relative error. noiseTarget > 0 is the stop rule: run() ends when the
    // noiseQuantile-th relative error is <= noiseTarget and every pixel is known (two batches of four passes), or after maxPasses (0 = the
    // budget `passes` gives); its refreshes then end on multiples of four passes. noise = true keeps the moments without the rule
    // (readNoise, Statistics::noise*). All off by default: every run then makes exactly the calls it made without these fields.
    bool noise = false;
    float noiseTarget = 0.0f;
    float noiseQuantile = 0.95f;
    float noiseFloor = 1e-2f;
    int maxPasses = 0;
    // Adaptive sampling (include/kajo_hip.h KAJO_FLAG_ADAPTIVE, kajo_hip_set_adaptive): adaptiveTarget > 0 creates the handles with the
    // noise and the adaptive flag and gives them the rule (noiseFloor is its floor; adaptiveMinPasses / adaptiveEvery 0 = the library's
    // defaults, 16 passes and every fourth batch). run() adds the handles' states at each refresh and ends when no unit is active, or
    // after maxPasses (0 = the budget `passes` gives); its refreshes end on multiples of four passes. Together with noiseTarget:
    // whichever rule ends first. 0 = off: every run then makes exactly the calls it made without these fields.
    float adaptiveTarget = 0.0f;
    int adaptiveAllowance = 0, adaptiveMinPasses = 0, adaptiveEvery = 0;
    // The noise-guided denoiser (include/kajo_hip.h KAJO_DENOISE_NOISE_GUIDED): the handles are created with the noise flag, and the
    // readDenoised*, readDisplayed and readPresented calls that are given denoise parameters (readDenoised*: or take the defaults) set the
    // flag in them. With more than one GPU (aovTiled) every owner's kajo_hip_noise fills one set of planes, as readNoise does, which go
    // to the first handle (kajo_hip_denoise_guide_planes) before the filter runs. Off by default: every run then makes exactly the calls
    // it made without this field.
    bool denoiseNoiseGuided = false;
    // Checkpoint and resume (include/kajo_hip.h "Checkpoints"). checkpointPath: run() writes the owners' sections -- a small container, one
    // section per GPU -- at its end and, with checkpointEvery > 0, after the refresh that reaches or passes each multiple of that many
    // passes; to a temporary name beside the file, then renamed, so that a kill during the write leaves the file of before. resumePath:
    // run() restores the handles from such a file before its first pass and counts on from the file's pass count (`passes` is the total
    // of the whole session); a file of another number of GPUs goes through kajo_hip_checkpoint_merge, which an adaptive file is refused
    // by. All empty by default: every run then makes exactly the calls it made without these fields.
    std::string checkpointPath, resumePath;
    int checkpointEvery = 0;
};

struct Statistics
{
    int passes = 0;
    unsigned long long paths = 0, traversals = 0, vertices = 0, laneSlots = 0;
    double kernelMs = 0;   // max over GPUs of the summed render-kernel time
    double wallSeconds = 0;
    int gpus = 0;          // tile owners the frame was dealt to
    std::vector<double> batchMs; // wall time of every refresh: render launch .. Image::pixels filled (host), in run() order
    std::vector<int> batchPasses;
    float toneScale = 1;   // the scale s the last image was tone-mapped with (Options::tone; 1 with the identity)
    long long clamped = 0, repaired = 0; // pixels of the last image the despeckle clamped and repaired (Options::despeckleOn)
    // the noise estimate at the last refresh (Options::noise or noiseTarget; all owners' histograms added): the noiseQuantile-th relative
    // error (-1: no pixel known), the pixels known, those with a batch that was not finite, and the pass the stop rule ended run() at (0:
    // it did not)
    float noiseQuantileValue = -1;
    long long noiseKnownPx = 0, noiseUnknownPx = 0, noiseBadPx = 0;
    int noiseStoppedAtPass = 0;
    // adaptive sampling at the last refresh (Options::adaptiveTarget; the owners' states added): the units and those still active, the camera
    // paths actually traced (`paths` above stays the nominal count), and the pass run() ended at because no unit was active (0: it did not)
    long long adaptiveUnits = 0, adaptiveActiveUnits = 0, adaptivePaths = 0;
    int adaptiveStoppedAtPass = 0;
    // checkpoints (Options::checkpointPath / resumePath): the pass count of the last file written (0: none), the pass count run() resumed
    // from, and the whole frame's SUM digest at the end of run() (the owners' kajo_hip_digest words added), taken only with one of the two
    int checkpointPasses = 0, resumedFromPasses = 0;
    unsigned long long frameDigest = 0;
};

class Scheduler : public ::Scheduler
{
public:
    Scheduler(const scene::Scene&, Image*, Preview*);
    Scheduler(const scene::Scene&, Image*, Preview*, const Options&);
    // not marked `override`: the reference's ::Scheduler (renderer/Scheduler.h:12-16) has no virtual destructor -- its
    // Main.cpp deletes backends through the base pointer at exit, so there this destructor would not run (the process
    // ends right after; GPU memory goes with it). With this repo's stand-in base it is virtual.
    ~Scheduler();

    void run() override;

    const Statistics& statistics() const;
    // whole-frame float accumulation (W*H*4, sum over passes of radiance / S) after run()
    void readRadiance(float* dst);
    // first-hit AOV sums after run() (Options::aov; include/kajo_hip.h kajo_hip_read_aov): W*H*4 floats each, either may be null
    void readAov(float* albedoHits, float* normalDepth, long long* samples);
    // the object-coverage tables after run() (Options::aov and Options::matte; include/kajo_hip.h kajo_hip_read_matte): W*H*8 ranked ids and
    // counts, any of the three may be null
    void readMatte(int32_t* ids, uint32_t* counts, long long* samples);
    // the coverage of the objects[0 .. n) and the dominant id per pixel (include/kajo_hip.h kajo_hip_matte_mask): W*H floats each, either may be null
    void readMatteMask(const int32_t* objects, int n, float* mask, float* dominant);
    // the frame denoised with the AOVs as guides after run() (Options::aov; include/kajo_hip.h kajo_hip_denoise): W*H*4 float sums and
    // W*H ARGB8 words, either may be null; params null = kajo_hip_default_denoise_params
    void readDenoised(const KajoDenoiseParams* params, float* radiance, uint32_t* argb8);
    // the same frame tone-mapped (include/kajo_hip.h kajo_hip_tonemap_argb8 with denoise = params): W*H ARGB8 words; tone null = Options::tone;
    // *scale (may be null) = the s applied
    void readDenoisedTonemapped(const KajoDenoiseParams* params, const KajoToneParams* tone, uint32_t* argb8, float* scale);
    // the whole display chain after run() (include/kajo_hip.h kajo_hip_display_argb8 on the first handle: one GPU, or a composed frame):
    // denoise (null = the accumulation; otherwise Options::aov) -> glare (null = Options::glare) -> tone (null = Options::tone)
    void readDisplayed(const KajoDenoiseParams* denoise, const KajoGlareParams* glare, const KajoToneParams* tone, uint32_t* argb8, float* scale);
    // the same chain with the despeckle in front (include/kajo_hip.h kajo_hip_present_argb8): despeckle null = Options::despeckle where
    // Options::despeckleOn, else none (then readDisplayed); counts (may be null) = pixels clamped, pixels repaired (0, 0 without the stage).
    // With Options::meterOn the chain ends in the metered call (kajo_hip_present_metered_argb8) and lastMeter() is its measurement; with
    // Options::localOn the local tone mapping sits between the glare and the meter (kajo_hip_present_local_argb8); with Options::lensOn the
    // depth of field sits between the denoiser and the glare (kajo_hip_present_lens_argb8; the AOVs are gathered and composed first, as
    // for `denoise`), and lastLens() is what it focused on; with Options::gradeOn the grade sits between the denoiser and the lens
    // (kajo_hip_present_grade_argb8; with regions the mattes are gathered and composed first), and lastGrade() is the slope it used
    void readPresented(const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* glare, const KajoToneParams* tone,
                       uint32_t* argb8, float* scale, long long counts[2]);

    // the measurement of the most recent metered image (Options::meterOn: run()'s last refresh, or readPresented); all zero before it
    const KajoMeterResult& lastMeter() const;
    // the pivot of the most recent local tone mapping (Options::localOn: run()'s last refresh, or readPresented); false where the stage has
    // not run (off, or a copy by its parameters)
    bool lastLocalPivot(float* pivot) const;
    // the focus distance of the most recent image with the depth of field (Options::lensOn: readPresented) and the largest circle of
    // confusion in it, in pixels; false where the stage has not run
    bool lastLens(float* focusDistance, float* maxRadiusPx) const;
    // the global slope of the most recent image with the grade (Options::gradeOn: readPresented, readViewed), the gains of
    // Options::gradeNeutralAt in it; false where the stage has not run
    bool lastGrade(float slope[3]) const;
    // the image of readPresented() with Options' own stages, through Options::view: dst = view.outW * view.outH words. Any number of GPUs
    // (the frame is composed on the first handle, as readPresented does). Throws where Options::viewOn is not set.
    void readViewed(uint32_t* dst);
    // the image of readPresented() with Options' own stages, through the encode in place of the 8-bit word (include/kajo_hip.h "The
    // encode"): dst = kajo_hip_encode_bytes bytes of encode's format. With several owners (or Options::forceGather) the gathered tile
    // buffers go through kajo_hip_encode_present_gathered_device; with the stages that need the whole frame's AOVs (Options::lensOn, grade
    // regions, gradeNeutralAt) the frame is composed on the first handle, as readViewed does, and kajo_hip_encode_present runs there. The
    // view takes no part. The library's refusals (the tone parameters' automatic exposure among them) are thrown.
    void readEncoded(const KajoEncodeParams* encode, void* dst);
    // ... and through Options::view as the float view, between the tone curve and the encode's transfer (include/kajo_hip.h "The float
    // view"): dst = kajo_hip_encode_bytes bytes of a view.outW x view.outH image. It composes first where readViewed and readEncoded do;
    // with several owners the gathered tile buffers go through kajo_hip_encode_view_present_gathered_device. Throws where Options::viewOn
    // is not set.
    void readEncodedViewed(const KajoEncodeParams* encode, void* dst);
    // the noise map after run() (Options::noise or noiseTarget; include/kajo_hip.h kajo_hip_noise on every owner, into the same planes):
    // W*H floats each -- mean luminance per pass, its standard error, the relative error -- any may be null. Any number of GPUs, no gather
    void readNoise(float* mean, float* stderror, float* relative);
    // the pixels the noise-guided denoiser has a measurement for after run() (Options::denoiseNoiseGuided): se >= 0 and m > 0 in the
    // owners' planes, counted on the host
    long long denoiseMeasuredPixels();
    // the per-pixel pass count after run() (Options::adaptiveTarget; include/kajo_hip.h kajo_hip_adapt_passes on every owner, into the same
    // plane): W*H words. Any number of GPUs, no gather
    void readSamplePasses(uint32_t* plane);

private:
    void readEncodedThrough(const KajoEncodeParams* encode, const KajoViewParams* view, void* dst);
    struct Impl;
    std::unique_ptr<Impl> m_impl;
};

} // namespace hip

#endif
