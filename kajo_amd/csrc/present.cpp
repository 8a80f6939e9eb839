// present.cpp -- libkajo_hip.so: the display path of include/kajo_hip.h. The stages (denoise, tone, glare, despeckle, meter, local, lens,
// view, grade, encode), each with its refusals, its scratch layout and the helpers of its own entry points; then the chain
//     despeckle -> denoise -> grade -> lens -> glare -> local -> meter -> tone -> view, or -> encode in place of the tone kernels' word
//     (with a view beside the encode: the float view, between the tone curve and the transfer)
// as one description (Chain), one check (checkChain) and one run (runChain), and every kajo_hip_tonemap_*, kajo_hip_display_*,
// kajo_hip_present_* entry point, kajo_hip_glare, _local, _lens, _grade, _meter, _encode, _encode_present, _encode_view and
// _encode_view_present as a wrapper that fills the description. The handle and what it shares with capi.cpp: handle.h. The encode's host
// half: encode_host.h; the float view's: encode_view_host.h.
#include "handle.h"

#include "encode_host.h"
#include "encode_view_host.h"

// encode.cpp's launcher (its argument block is encode_math.h's)
extern "C" {
size_t kajo_encode_table_words(void);
int kajo_encode_launch(const void* src, const TileMap* map, int fromTiles, const kajo::EncodeArgs* a, const void* table, void* dst, void* stream);
// encode_view.cpp's
int kajo_encode_view_launch(const void* src, const TileMap* map, int fromTiles, const kajo::EncodeArgs* a, const void* table, const void* firstX,
                            const void* countX, const void* wxT, const void* firstY, const void* countY, const void* wy, int strideY, int outW,
                            int outH, int row0, int rows, void* T, void* dst, void* stream);
}

extern "C" {

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

// ... and those that need the frame's size
int checkViewFrame(int W, int H, const KajoViewParams* p, ViewRect* r)
{
    const bool whole = p->x0 == 0.0f && p->y0 == 0.0f && p->x1 == 0.0f && p->y1 == 0.0f;
    *r = ViewRect{p->x0, p->y0, whole ? (double)W : (double)p->x1, whole ? (double)H : (double)p->y1, false};
    if (r->x1 > W || r->y1 > H)
        return fail(KAJO_E_INVALID, "view rectangle must lie inside the frame");
    if ((r->x1 - r->x0) / p->outW > KAJO_VIEW_MAX_SCALE || (r->y1 - r->y0) / p->outH > KAJO_VIEW_MAX_SCALE)
        return fail(KAJO_E_INVALID, "view minification must be at most 64");
    r->copy = p->outW == W && p->outH == H && r->x0 == 0.0 && r->y0 == 0.0 && r->x1 == W && r->y1 == H;
    return KAJO_OK;
}

// ... of a handle's frame: last of all, behind the null handle
int checkViewHandle(kajo_hip_t h, const KajoViewParams* p, ViewRect* r)
{
    if (!h)
        return fail(KAJO_E_INVALID, "null handle");
    return checkViewFrame(h->W, h->H, p, r);
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

} // extern "C"

namespace
{

// The refusals of KajoEncodeParams (KAJO_E_INVALID), before any device work and before the handle is looked at
int checkEncode(const KajoEncodeParams* p)
{
    const char* refusal = kajo::encodeRefusal(p);
    return refusal ? fail(KAJO_E_INVALID, refusal) : KAJO_OK;
}

// ... and of the tone parameters beside an encode: their scale would be formed inside the tone launch, which the encode replaces
int checkEncodeTone(const KajoToneParams* tone)
{
    if (tone->flags & KAJO_TONE_AUTO_EXPOSURE)
        return fail(KAJO_E_INVALID, "the encode takes no automatic exposure from the tone parameters (their scale is formed inside the tone "
                                    "launch): use metered exposure, a meter stage in the chain, which patches the tone parameters on the host");
    return KAJO_OK;
}

bool encodeTabled(const KajoEncodeParams* p)
{
    return p->format != KAJO_ENCODE_RGBA16F && p->transfer != KAJO_TRANSFER_LINEAR;
}

kajo::EncodeArgs encodeArgsOf(const KajoEncodeParams* p, const ToneArgs& t, float passes)
{
    kajo::EncodeArgs a{};
    a.format = p->format;
    a.transfer = p->transfer;
    a.flags = p->flags;
    a.curve = t.curve;
    a.scale = t.exposureScale;
    a.white = t.white;
    a.seed = p->ditherSeed;
    a.passes = passes;
    return a;
}

// Form the table of *p's transfer and upload it, unless it is the last call's (the event discipline of viewPlan and gradePlan)
int encodePlan(KajoHip* h, const KajoEncodeParams* p)
{
    const float peak = p->transfer == KAJO_TRANSFER_PQ ? p->peakNits : 0.0f;
    if (h->encodePlanned && h->encodeTransfer == p->transfer && h->encodePeak == peak)
        return KAJO_OK;
    h->encodePlanned = false;
    if (kajo_encode_table_words() != (size_t)kajo::kEncodeTableWords)
        return fail(KAJO_E_INVALID, "encode table layout mismatch");
    const size_t bytes = (size_t)kajo::kEncodeTableWords * sizeof(float);
    if (!h->encodeUploaded)
        HIP_TRY(hipEventCreateWithFlags(&h->encodeUploaded, hipEventDisableTiming));
    else
        HIP_TRY(hipEventSynchronize(h->encodeUploaded)); // (the copy before this one has left the staging block; kernels are not waited for)
    if (!h->encodeStaging)
        HIP_TRY(hipHostMalloc(&h->encodeStaging, bytes, hipHostMallocDefault));
    HIP_TRY(h->encodeTable.ensure(bytes));
    kajo::encodeTable(p->transfer, peak, static_cast<float*>(h->encodeStaging));
    HIP_TRY(hipMemcpyAsync(h->encodeTable.p, h->encodeStaging, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->encodeUploaded, h->stream));
    h->encodeTransfer = p->transfer;
    h->encodePeak = peak;
    h->encodePlanned = true;
    return KAJO_OK;
}

// Enqueue the encode of an image (tiles through h->map's geometry, or a row-major frame) into dst (device, W * H words of the format).
// Checked by checkEncode, device bound. The handle's tone scale (kajo_hip_tone_scale) stays the last tone mapping's.
int encodeLaunch(KajoHip* h, Image img, const ToneArgs& t, const KajoEncodeParams* p, void* dst)
{
    int rc;
    if (encodeTabled(p) && (rc = encodePlan(h, p)))
        return rc;
    const kajo::EncodeArgs a = encodeArgsOf(p, t, (float)h->passesDone);
    hipError_t le = (hipError_t)kajo_encode_launch(img.src, &h->map, img.fromTiles ? 1 : 0, &a, encodeTabled(p) ? h->encodeTable.p : nullptr, dst, h->stream);
    if (le != hipSuccess)
        return failHip(le, "encode kernel launch");
    return KAJO_OK;
}

// Enqueue the float view of an image (tiles through h->map's geometry, or a row-major frame) into dst (device, outW * outH words of the
// format): the view's own rows (viewPlan: its pinned staging, uploaded once per set of parameters) and its intermediate, the encode's
// table. Checked by checkView, checkEncode and checkViewHandle, device bound. The copy case launches the plain encode.
int encodeViewImage(KajoHip* h, Image img, const ToneArgs& t, const KajoEncodeParams* p, const KajoViewParams* view, const ViewRect& r, void* dst)
{
    if (r.copy)
        return encodeLaunch(h, img, t, p, dst);
    int rc;
    if (encodeTabled(p) && (rc = encodePlan(h, p)))
        return rc;
    if ((rc = viewPlan(h, view, r)))
        return rc;
    const auto& pl = h->viewPlan;
    HIP_TRY(growBuffer(h->viewMid, &h->viewMidBytes, (size_t)view->outW * pl.rows * 16));
    const kajo::EncodeArgs a = encodeArgsOf(p, t, (float)h->passesDone);
    const char* rows = h->viewRows.as<char>();
    hipError_t le = (hipError_t)kajo_encode_view_launch(img.src, &h->map, img.fromTiles ? 1 : 0, &a, encodeTabled(p) ? h->encodeTable.p : nullptr,
                                                        rows + pl.firstX, rows + pl.countX, rows + pl.wx, rows + pl.firstY, rows + pl.countY,
                                                        rows + pl.wy, pl.strideY, view->outW, view->outH, pl.row0, pl.rows, h->viewMid.p, dst,
                                                        h->stream);
    if (le != hipSuccess)
        return failHip(le, "encode view kernel launch");
    return KAJO_OK;
}

} // namespace

extern "C" {

void kajo_hip_default_encode_params(KajoEncodeParams* p)
{
    if (!p)
        return;
    std::memset(p, 0, sizeof *p);
    p->format = KAJO_ENCODE_ARGB8;
    p->transfer = KAJO_TRANSFER_GAMMA22;
    p->peakNits = 1000.0f;
}

int kajo_hip_encode_bytes(const KajoEncodeParams* p, int width, int height, size_t* bytes)
{
    int rc = checkEncode(p);
    if (rc)
        return rc;
    if (width < 1 || height < 1)
        return fail(KAJO_E_INVALID, "width and height must be at least 1");
    if (!bytes)
        return fail(KAJO_E_INVALID, "null argument");
    *bytes = (size_t)width * (size_t)height * kajo::encodePixelBytes(p->format);
    return KAJO_OK;
}

int kajo_hip_encode_table(uint32_t transfer, float peakNits, float* table, size_t capacity)
{
    if (transfer > KAJO_TRANSFER_LINEAR)
        return fail(KAJO_E_INVALID, "unknown encode transfer");
    if (transfer == KAJO_TRANSFER_LINEAR)
        return fail(KAJO_E_INVALID, "the linear transfer has no table");
    if (transfer == KAJO_TRANSFER_PQ && !(std::isfinite(peakNits) && peakNits > 0.0f && peakNits <= 10000.0f))
        return fail(KAJO_E_INVALID, "encode peak luminance must be finite and in (0, 10000] nits");
    if (table) {
        if (capacity < (size_t)kajo::kEncodeTableWords)
            return fail(KAJO_E_INVALID, "table array too small");
        kajo::encodeTable(transfer, peakNits, table);
    }
    return kajo::kEncodeTableWords;
}

int kajo_hip_encode_pixels(const KajoEncodeParams* encode, const KajoToneParams* tone, const float* meanRgb, int64_t n, int32_t x0, int32_t y0,
                           int32_t rowWidth, void* out)
{
    ToneArgs t{};
    int rc = toneArgsOf(tone, &t);
    if (rc)
        return rc;
    if ((rc = checkEncode(encode)) || (rc = checkEncodeTone(tone)))
        return rc;
    if (n < 0 || (n > 0 && (!meanRgb || !out)))
        return fail(KAJO_E_INVALID, "null argument");
    if (rowWidth < 1)
        return fail(KAJO_E_INVALID, "encode row width must be at least 1");
    std::vector<float> table;
    if (encodeTabled(encode)) {
        table.resize(kajo::kEncodeTableWords);
        kajo::encodeTable(encode->transfer, encode->transfer == KAJO_TRANSFER_PQ ? encode->peakNits : 0.0f, table.data());
    }
    kajo::encodePixels(encodeArgsOf(encode, t, 1.0f), table.data(), meanRgb, n, x0, y0, rowWidth, out);
    return KAJO_OK;
}

int kajo_hip_encode_view_pixels(const KajoEncodeParams* encode, const KajoToneParams* tone, const KajoViewParams* view, const float* meanRgb,
                                int32_t width, int32_t height, void* out)
{
    ToneArgs t{};
    int rc = toneArgsOf(tone, &t);
    if (rc)
        return rc;
    if (view && (rc = checkView(view)))
        return rc;
    if ((rc = checkEncode(encode)) || (rc = checkEncodeTone(tone)))
        return rc;
    if (width < 1 || height < 1)
        return fail(KAJO_E_INVALID, "width and height must be at least 1");
    if (!meanRgb || !out)
        return fail(KAJO_E_INVALID, "null argument");
    ViewRect r{};
    if (view && (rc = checkViewFrame(width, height, view, &r)))
        return rc;
    std::vector<float> table;
    if (encodeTabled(encode)) {
        table.resize(kajo::kEncodeTableWords);
        kajo::encodeTable(encode->transfer, encode->transfer == KAJO_TRANSFER_PQ ? encode->peakNits : 0.0f, table.data());
    }
    const kajo::EncodeArgs a = encodeArgsOf(encode, t, 1.0f);
    if (!view || r.copy) {
        kajo::encodePixels(a, table.data(), meanRgb, (int64_t)width * height, 0, 0, width, out);
        return KAJO_OK;
    }
    kajo::ViewAxis ax, ay;
    if (!kajo::viewAxis(width, r.x0, r.x1, view->outW, view->filter, &ax) || !kajo::viewAxis(height, r.y0, r.y1, view->outH, view->filter, &ay))
        return fail(KAJO_E_INVALID, "view row longer than 384 taps");
    kajo::encodeViewPixels(a, table.data(), meanRgb, width, ax, ay, out);
    return KAJO_OK;
}

} // extern "C"

namespace
{

// Where a chain's image goes
enum ChainSink
{
    kSinkRadiance,   // the float radiance after the last stage given, to the host (dst null: the stages run, nothing is copied)
    kSinkMeter,      // the histogram of that frame (dst, may be null) and its evaluation (result), to the host
    kSinkHostArgb,   // the ARGB8 image through the handle's own frame to the host (dst null: likewise)
    kSinkDeviceArgb, // the ARGB8 image to a device pointer; nothing is waited for beyond what the stages wait for themselves
    kSinkHostEncoded,   // the encoded image (Chain::encode) through the handle's own buffer to the host (dst null: likewise)
    kSinkDeviceEncoded, // the encoded image to a device pointer, as kSinkDeviceArgb
};

// stages an entry point refuses to run without (the tone parameters: every ARGB8 sink)
enum : unsigned
{
    kNeedGrade = 1,
    kNeedLens = 2,
    kNeedGlare = 4,
    kNeedLocal = 8,
    kNeedMeter = 16,
};

// The display chain of include/kajo_hip.h, despeckle -> denoise -> grade -> lens -> glare -> local -> meter -> tone -> view: the stages
// given (null: absent), the source and the sink. Every chain entry point fills one and hands it to present().
struct Chain
{
    const KajoDespeckleParams* despeckle = nullptr;
    const KajoDenoiseParams* denoise = nullptr;
    const KajoGradeParams* grade = nullptr;
    const KajoLensParams* lens = nullptr;
    const KajoGlareParams* glare = nullptr;
    const KajoLocalParams* local = nullptr;
    const KajoMeterParams* meter = nullptr;
    const KajoToneParams* tone = nullptr;
    const KajoViewParams* view = nullptr;
    const KajoEncodeParams* encode = nullptr; // the encoded sinks: in place of the tone kernels' word; a view beside it is the float view
    unsigned need = 0;
    // the source: the handle's own frame, or gathered tile buffers (tiles null: the handle's own tiles, which must be the whole frame)
    bool gathered = false;
    const void* tiles = nullptr;
    ChainSink sink = kSinkHostArgb;
    void* dst = nullptr;
    KajoMeterResult* result = nullptr; // of the meter stage, or of kSinkMeter
    float* scale = nullptr;            // kSinkHostArgb: the s of the tone mapping (kajo_hip_tone_scale)
    // what a null handle is answered with: the gathered entries say "null argument" for the handle and the destination alike, except
    // where a view without a grade is given
    const char* nullHandle = "null handle";
    // formed by checkChain
    ToneArgs toneArgs{};
    ViewRect rect{};
};

// Every refusal of a chain, before any device work, in the header's order: the stages' parameters (despeckle, grade, lens, glare, local,
// meter, tone, the two automatic exposures, view, encode), the denoiser's parameters and its handle rules, then the handle (null, the grade's
// state, the lens's, the view against the frame). -> c.toneArgs, c.rect
int checkChain(kajo_hip_t h, Chain& c)
{
    int rc;
    if (c.despeckle && (rc = checkDespeckle(c.despeckle)))
        return rc;
    if ((c.grade || (c.need & kNeedGrade)) && (rc = checkGrade(c.grade)))
        return rc;
    if ((c.lens || (c.need & kNeedLens)) && (rc = checkLens(c.lens)))
        return rc;
    if ((c.glare || (c.need & kNeedGlare)) && (rc = checkGlare(c.glare)))
        return rc;
    if ((c.local || (c.need & kNeedLocal)) && (rc = checkLocal(c.local)))
        return rc;
    if ((c.meter || (c.need & kNeedMeter)) && (rc = checkMeter(c.meter)))
        return rc;
    const bool encoded = c.sink == kSinkHostEncoded || c.sink == kSinkDeviceEncoded;
    if (c.sink == kSinkHostArgb || c.sink == kSinkDeviceArgb || encoded) {
        if ((rc = toneArgsOf(c.tone, &c.toneArgs)))
            return rc;
        if (c.meter && (c.tone->flags & KAJO_TONE_AUTO_EXPOSURE))
            return fail(KAJO_E_INVALID, "metered exposure and the tone parameters' automatic exposure are two automatic exposures: give one");
    }
    if (c.view && (rc = checkView(c.view)))
        return rc;
    if (encoded && ((rc = checkEncode(c.encode)) || (rc = checkEncodeTone(c.tone))))
        return rc;
    if (c.gathered && c.grade && c.grade->nRegions > 0)
        return fail(KAJO_E_INVALID, "grade regions need the whole frame's coverage tables: kajo_hip_present_grade_argb8 on the root");
    if (c.denoise && (rc = checkDenoise(h, c.denoise)))
        return rc;
    if (!h)
        return fail(KAJO_E_INVALID, c.nullHandle);
    if ((c.sink == kSinkDeviceArgb || c.sink == kSinkDeviceEncoded) && !c.dst)
        return fail(KAJO_E_INVALID, "null argument");
    if (c.grade && (rc = checkGradeHandle(h, c.grade, !c.gathered)))
        return rc;
    if (c.lens && (rc = checkLensHandle(h)))
        return rc;
    if (c.view && (rc = checkViewHandle(h, c.view, &c.rect)))
        return rc;
    return KAJO_OK;
}

// Run a checked chain on the handle's stream, stage by stage, each one handed the frame the one before it left
int runChain(KajoHip* h, const Chain& c)
{
    Image img;
    int rc = imageOf(h, c.gathered, c.tiles, &img);
    if (rc)
        return rc;
    const size_t count = (size_t)h->W * h->H;
    if (c.sink == kSinkHostArgb)
        HIP_TRY(h->argb.ensure(count * 4));
    // (with the denoiser behind it the despeckle writes the handle's tile layout where the handle is the frame's one owner, else -- tiled
    // AOVs, the composed frame -- row-major: the denoiser reads either. Without a despeckle the denoiser takes the accumulation itself)
    if (c.despeckle && (rc = despeckleImage(h, c.despeckle, img, c.denoise != nullptr && h->map.tileCount == 1, &img)))
        return rc;
    if (c.denoise) {
        void* out = nullptr;
        if ((rc = denoiseFrame(h, c.denoise, &out, c.despeckle ? &img : nullptr)))
            return rc;
        img = Image{out, false};
    }
    if (c.grade && (rc = gradeImage(h, c.grade, img, &img)))
        return rc;
    if (c.lens && (rc = lensImage(h, c.lens, img, &img)))
        return rc;
    if (c.glare && (rc = glareImage(h, c.glare, img, &img)))
        return rc;
    if (c.local && (rc = localImage(h, c.local, img, &img))) // (one wait with KAJO_LOCAL_PIVOT_METERED: include/kajo_hip.h)
        return rc;
    if (c.sink == kSinkMeter) {
        uint32_t counts[kMeterRow];
        if ((rc = meterImage(h, img, counts)))
            return rc;
        return meterResult(h, counts, c.meter, static_cast<uint32_t*>(c.dst), c.result);
    }
    if (c.sink == kSinkRadiance) {
        if (img.fromTiles) {
            // (a copy of the accumulation: the composed frame, as kajo_hip_read_radiance)
            if ((rc = composeOwn(h)))
                return rc;
            img = Image{h->frame.p, false};
        }
        if (c.dst)
            HIP_TRY(hipMemcpyAsync(c.dst, img.src, count * 16, hipMemcpyDeviceToHost, h->stream));
        return kajo_hip_wait(h);
    }
    // (the meter measures the frame the tone kernels are handed, which is still where the stages left it; one wait)
    ToneArgs t = c.toneArgs;
    if (c.meter && (rc = meterAndPatch(h, img, c.meter, c.tone, c.result, &t)))
        return rc;
    if (c.sink == kSinkDeviceEncoded)
        return c.view ? encodeViewImage(h, img, t, c.encode, c.view, c.rect, c.dst) : encodeLaunch(h, img, t, c.encode, c.dst);
    if (c.sink == kSinkHostEncoded) {
        const size_t encodedBytes = (c.view ? (size_t)c.view->outW * c.view->outH : count) * kajo::encodePixelBytes(c.encode->format);
        HIP_TRY(growBuffer(h->encodeOut, &h->encodeOutBytes, encodedBytes));
        if ((rc = c.view ? encodeViewImage(h, img, t, c.encode, c.view, c.rect, h->encodeOut.p) : encodeLaunch(h, img, t, c.encode, h->encodeOut.p)))
            return rc;
        if (c.dst)
            HIP_TRY(hipMemcpyAsync(c.dst, h->encodeOut.p, encodedBytes, hipMemcpyDeviceToHost, h->stream));
        return kajo_hip_wait(h);
    }
    if (c.sink == kSinkDeviceArgb) {
        if (!c.view || c.rect.copy)
            return toneLaunch(h, img, t, c.dst);
        HIP_TRY(h->viewIn.ensure(count * 4));
        if ((rc = toneLaunch(h, img, t, h->viewIn.p)))
            return rc;
        return viewImage(h, c.view, c.rect, h->viewIn.p, c.dst);
    }
    if ((rc = toneLaunch(h, img, t, h->argb.p)))
        return rc;
    const void* image = h->argb.p;
    size_t bytes = count * 4;
    if (c.view) {
        bytes = (size_t)c.view->outW * c.view->outH * 4;
        HIP_TRY(growBuffer(h->viewOut, &h->viewOutBytes, bytes));
        if ((rc = viewImage(h, c.view, c.rect, h->argb.p, h->viewOut.p)))
            return rc;
        image = h->viewOut.p;
    }
    if (c.dst)
        HIP_TRY(hipMemcpyAsync(c.dst, image, bytes, hipMemcpyDeviceToHost, h->stream));
    return c.scale ? kajo_hip_tone_scale(h, c.scale) : kajo_hip_wait(h);
}

int present(kajo_hip_t h, Chain& c)
{
    const int rc = checkChain(h, c);
    return rc ? rc : runChain(h, c);
}

// the three kinds of entry point: the handle's own frame to the host, gathered tiles to a device pointer, a partial chain's radiance
Chain hostChain(uint32_t* argb8, KajoMeterResult* result = nullptr, float* scale = nullptr)
{
    Chain c;
    c.dst = argb8;
    c.result = result;
    c.scale = scale;
    return c;
}

Chain gatheredChain(const void* tiles, void* dst, KajoMeterResult* result = nullptr)
{
    Chain c;
    c.gathered = true;
    c.tiles = tiles;
    c.sink = kSinkDeviceArgb;
    c.dst = dst;
    c.result = result;
    c.nullHandle = "null argument";
    return c;
}

Chain radianceChain(float* radiance, unsigned need)
{
    Chain c;
    c.sink = kSinkRadiance;
    c.dst = radiance;
    c.need = need;
    return c;
}

} // namespace

extern "C" {

// The chain's entry points: each fills a Chain with the stages its signature has and presents it. None calls another.

int kajo_hip_tonemap_argb8(kajo_hip_t h, const KajoToneParams* p, const KajoDenoiseParams* denoise, uint32_t* argb8, float* scale)
{
    Chain c = hostChain(argb8, nullptr, scale);
    c.denoise = denoise;
    c.tone = p;
    return present(h, c);
}

int kajo_hip_tonemap_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoToneParams* p, void* dst)
{
    Chain c = gatheredChain(gathered, dst);
    c.tone = p;
    return present(h, c);
}

int kajo_hip_glare(kajo_hip_t h, const KajoGlareParams* g, const KajoDenoiseParams* denoise, float* radiance)
{
    Chain c = radianceChain(radiance, kNeedGlare);
    c.denoise = denoise;
    c.glare = g;
    return present(h, c);
}

int kajo_hip_display_argb8(kajo_hip_t h, const KajoDenoiseParams* denoise, const KajoGlareParams* g, const KajoToneParams* tone, uint32_t* argb8,
                           float* scale)
{
    Chain c = hostChain(argb8, nullptr, scale);
    c.denoise = denoise;
    c.glare = g;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_display_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoGlareParams* g, const KajoToneParams* tone, void* dst)
{
    Chain c = gatheredChain(gathered, dst);
    c.glare = g;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_present_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                           const KajoToneParams* tone, uint32_t* argb8, float* scale)
{
    Chain c = hostChain(argb8, nullptr, scale);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.glare = g;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_present_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                           const KajoToneParams* tone, void* dst)
{
    Chain c = gatheredChain(gathered, dst);
    c.despeckle = despeckle;
    c.glare = g;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_meter(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                   const KajoMeterParams* meter, uint32_t* hist, KajoMeterResult* result)
{
    Chain c;
    c.sink = kSinkMeter;
    c.dst = hist;
    c.result = result;
    c.need = kNeedMeter;
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.glare = g;
    c.meter = meter;
    return present(h, c);
}

int kajo_hip_present_metered_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                                   const KajoMeterParams* meter, const KajoToneParams* tone, uint32_t* argb8, KajoMeterResult* result)
{
    Chain c = hostChain(argb8, result);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.glare = g;
    c.meter = meter;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_present_metered_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle,
                                                   const KajoGlareParams* g, const KajoMeterParams* meter, const KajoToneParams* tone, void* dst,
                                                   KajoMeterResult* result)
{
    Chain c = gatheredChain(gathered, dst, result);
    c.despeckle = despeckle;
    c.glare = g;
    c.meter = meter;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_local(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                   const KajoLocalParams* local, float* radiance)
{
    Chain c = radianceChain(radiance, kNeedLocal);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.glare = g;
    c.local = local;
    return present(h, c);
}

int kajo_hip_present_local_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                                 const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone, uint32_t* argb8,
                                 KajoMeterResult* result)
{
    Chain c = hostChain(argb8, result);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_present_local_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                                 const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone, void* dst,
                                                 KajoMeterResult* result)
{
    Chain c = gatheredChain(gathered, dst, result);
    c.despeckle = despeckle;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_lens(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                  float* radiance)
{
    Chain c = radianceChain(radiance, kNeedLens);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.lens = lens;
    return present(h, c);
}

int kajo_hip_present_lens_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                                const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                uint32_t* argb8, KajoMeterResult* result)
{
    Chain c = hostChain(argb8, result);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.lens = lens;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    return present(h, c);
}

int kajo_hip_present_view_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                                const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                const KajoViewParams* view, uint32_t* argb8, KajoMeterResult* result)
{
    Chain c = hostChain(argb8, result);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.lens = lens;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    c.view = view;
    return present(h, c);
}

int kajo_hip_present_view_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                                const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                                const KajoViewParams* view, void* dst, KajoMeterResult* result)
{
    Chain c = gatheredChain(gathered, dst, result);
    c.despeckle = despeckle;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    c.view = view;
    if (view)
        c.nullHandle = "null handle";
    return present(h, c);
}

int kajo_hip_grade(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                   float* radiance)
{
    Chain c = radianceChain(radiance, kNeedGrade);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.grade = grade;
    return present(h, c);
}

int kajo_hip_present_grade_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                                 const KajoLensParams* lens, const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                                 const KajoToneParams* tone, const KajoViewParams* view, uint32_t* argb8, KajoMeterResult* result)
{
    Chain c = hostChain(argb8, result);
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.grade = grade;
    c.lens = lens;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    c.view = view;
    return present(h, c);
}

int kajo_hip_present_grade_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle,
                                                 const KajoGradeParams* grade, const KajoGlareParams* g, const KajoLocalParams* local,
                                                 const KajoMeterParams* meter, const KajoToneParams* tone, const KajoViewParams* view, void* dst,
                                                 KajoMeterResult* result)
{
    Chain c = gatheredChain(gathered, dst, result);
    c.despeckle = despeckle;
    c.grade = grade;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    c.view = view;
    if (view && !grade)
        c.nullHandle = "null handle";
    return present(h, c);
}

int kajo_hip_encode(kajo_hip_t h, const KajoEncodeParams* encode, const KajoToneParams* tone, void* dst)
{
    Chain c;
    c.sink = kSinkHostEncoded;
    c.dst = dst;
    c.tone = tone;
    c.encode = encode;
    return present(h, c);
}

int kajo_hip_encode_present(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                            const KajoLensParams* lens, const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                            const KajoToneParams* tone, const KajoEncodeParams* encode, void* dst, KajoMeterResult* result)
{
    Chain c;
    c.sink = kSinkHostEncoded;
    c.dst = dst;
    c.result = result;
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.grade = grade;
    c.lens = lens;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    c.encode = encode;
    return present(h, c);
}

int kajo_hip_encode_present_gathered_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGradeParams* grade,
                                            const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                                            const KajoToneParams* tone, const KajoEncodeParams* encode, void* dst, KajoMeterResult* result)
{
    Chain c = gatheredChain(gathered, dst, result);
    c.sink = kSinkDeviceEncoded;
    c.despeckle = despeckle;
    c.grade = grade;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    c.encode = encode;
    return present(h, c);
}

int kajo_hip_encode_view(kajo_hip_t h, const KajoEncodeParams* encode, const KajoToneParams* tone, const KajoViewParams* view, void* dst)
{
    Chain c;
    c.sink = kSinkHostEncoded;
    c.dst = dst;
    c.tone = tone;
    c.view = view;
    c.encode = encode;
    return present(h, c);
}

int kajo_hip_encode_view_present(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                                 const KajoLensParams* lens, const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                                 const KajoToneParams* tone, const KajoViewParams* view, const KajoEncodeParams* encode, void* dst,
                                 KajoMeterResult* result)
{
    Chain c;
    c.sink = kSinkHostEncoded;
    c.dst = dst;
    c.result = result;
    c.despeckle = despeckle;
    c.denoise = denoise;
    c.grade = grade;
    c.lens = lens;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    c.view = view;
    c.encode = encode;
    return present(h, c);
}

int kajo_hip_encode_view_present_gathered_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle,
                                                 const KajoGradeParams* grade, const KajoGlareParams* g, const KajoLocalParams* local,
                                                 const KajoMeterParams* meter, const KajoToneParams* tone, const KajoViewParams* view,
                                                 const KajoEncodeParams* encode, void* dst, KajoMeterResult* result)
{
    Chain c = gatheredChain(gathered, dst, result);
    c.sink = kSinkDeviceEncoded;
    c.despeckle = despeckle;
    c.grade = grade;
    c.glare = g;
    c.local = local;
    c.meter = meter;
    c.tone = tone;
    c.view = view;
    c.encode = encode;
    return present(h, c);
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

} // extern "C"
