// Arguments.cpp -- kajo_render's command line: the reference's (renderer/Main.cpp:97-146: -w -h -r SCENE) plus what a window-less run
// needs, a pass budget, the output names and the backend's options. One function per stage of options, called in a fixed order: where two
// bad options are given, the first stage's message is the one printed.
#include "Arguments.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

const char* const transferNames[4] = {"gamma22", "srgb", "pq", "linear"};
const char* const viewFilterNames[4] = {"nearest", "area", "triangle", "lanczos3"};

namespace
{

// the options whose value is checked after the loop, as given: empty = not given
struct Raw
{
    std::string toneCurve, toneExposure, toneWhite, toneKey;
    bool toneAuto = false;
    std::string glareStrength, glareLevels, glareThreshold;
    std::string despeckleFactor, despeckleRank, despeckleFloor;
    std::string untilNoise, noiseQuantile, noiseFloor, maxPasses;
    std::string checkpointEvery;
    std::string adaptiveE, adaptiveAllowance, adaptiveMinPasses, adaptiveEvery;
    std::string meterExposure, meterWhite;
    std::string localContrast, localDetail, localRange, localIterations, localPivot;
    std::string transferName, peakNits, ditherSeed;
    std::string outputSize, viewRect, viewFilter, supersample;
    std::string lensAperture, lensFocus, lensFocusAt, lensMaxRadius;
    std::string gradeSlope, gradeOffset, gradePower, gradeSaturation, whiteBalance, whiteBalanceAt;
    std::vector<std::string> gradeRegions;
    std::string matteObjects;
    bool matteObjectsGiven = false;
};

int refuse(const std::string& message)
{
    std::cerr << "kajo_render: " << message << std::endl;
    return 1;
}

// a stage that the three-argument constructor cannot be told about (the encode and the view word it differently)
int refuseThreeArg(const char* stage, const char* needs = "the backend's options")
{
    return refuse(std::string("the ") + stage + " options need " + needs + " (without --three-arg)");
}

// --aov, the matte files, --denoise and --lens-aperture read buffers of ONE handle (include/kajo_hip.h KAJO_FLAG_AOV), unless every owner
// keeps its own tiles' (--aov-tiled): 0 where that holds
int needsWholeFrame(const Arguments& a, const char* option)
{
    if ((a.opt.gpus == 1 || a.opt.aovTiled) && !a.threeArg)
        return 0;
    return refuse(std::string(option) + " needs the whole frame on one GPU (--gpus 1, without --three-arg)");
}

// a float option's value, whole and finite, or false
bool parseFloat(const std::string& text, float* out)
{
    char* end = nullptr;
    const float v = std::strtof(text.c_str(), &end);
    if (text.empty() || *end != '\0' || !std::isfinite(v))
        return false;
    *out = v;
    return true;
}

// ... and in lo..hi, either end open where asked (INFINITY: no bound)
enum { OpenLo = 1, OpenHi = 2 };
bool floatIn(const std::string& text, float lo, float hi, float* out, int open = 0)
{
    return parseFloat(text, out) && ((open & OpenLo) ? *out > lo : *out >= lo) && ((open & OpenHi) ? *out < hi : *out <= hi);
}

// a whole number in lo..hi, nothing behind it. (The checks this one replaces were of two kinds, with and without `end == text`; they
// differed for the empty string alone, which means "not given" for every option and reaches none of them.)
bool wholeIn(const std::string& text, long lo, long hi, int32_t* out)
{
    char* end = nullptr;
    const long n = std::strtol(text.c_str(), &end, 10);
    if (end == text.c_str() || *end != '\0' || n < lo || n > hi)
        return false;
    *out = (int32_t)n;
    return true;
}

// X,Y: a pixel of a w x h frame
bool pixelIn(const std::string& text, int w, int h, int* x, int* y)
{
    char tail = 0;
    return std::sscanf(text.c_str(), "%d,%d%c", x, y, &tail) == 2 && *x >= 0 && *y >= 0 && *x < w && *y < h;
}

std::vector<std::string> split(const std::string& text, char separator)
{
    std::vector<std::string> items;
    size_t at = 0;
    while (true) {
        const size_t next = text.find(separator, at);
        items.push_back(text.substr(at, next == std::string::npos ? std::string::npos : next - at));
        if (next == std::string::npos)
            return items;
        at = next + 1;
    }
}

// a comma-separated list of object ids (whole numbers >= 0, at least one), or false
bool parseObjects(const std::string& text, std::vector<int32_t>* out)
{
    out->clear();
    for (const std::string& item : split(text, ',')) {
        char* end = nullptr;
        const long v = std::strtol(item.c_str(), &end, 10);
        if (item.empty() || item.size() > 9 || *end != '\0' || item[0] < '0' || item[0] > '9')
            return false;
        out->push_back((int32_t)v);
    }
    return true;
}

// three numbers R,G,B -- or, where `orOne`, one number for all three; text that is no number becomes a NaN (the library refuses it by name)
bool parseTriple(const std::string& text, bool orOne, float out[3])
{
    const std::vector<std::string> items = split(text, ',');
    if (!(items.size() == 3 || (orOne && items.size() == 1)))
        return false;
    for (int c = 0; c < 3; c++)
        if (!parseFloat(items[items.size() == 1 ? 0 : c], &out[c]))
            out[c] = NAN;
    return true;
}

// --grade-region IDS:key=v[:key=v...] into a region that holds the defaults
bool parseRegion(const std::string& text, KajoGradeRegion* r)
{
    const std::vector<std::string> parts = split(text, ':');
    std::vector<int32_t> ids;
    if (!parseObjects(parts[0], &ids) || ids.size() > KAJO_GRADE_REGION_OBJECTS)
        return false;
    r->n = (int32_t)ids.size();
    for (size_t i = 0; i < ids.size(); i++)
        r->objects[i] = ids[i];
    for (size_t i = 1; i < parts.size(); i++) {
        const size_t eq = parts[i].find('=');
        if (eq == std::string::npos)
            return false;
        const std::string key = parts[i].substr(0, eq), value = parts[i].substr(eq + 1);
        if (key == "slope" || key == "offset" || key == "power") {
            if (!parseTriple(value, true, key == "slope" ? r->op.slope : key == "offset" ? r->op.offset : r->op.power))
                return false;
        } else if (key == "saturation" || key == "amount") {
            float* field = key == "saturation" ? &r->op.saturation : &r->amount;
            if (!parseFloat(value, field))
                *field = NAN;
        } else
            return false;
    }
    return true;
}

int help(const char* program)
{
    std::printf("Usage: %s OPTIONS [SCENE]\n\n"
                "    -w SIZE         image width (640)\n"
                "    -h SIZE         image height (480)\n"
                "    -r NAME         renderer (hip)\n"
                "    --spp N         nominal samples per pixel per pass (32)\n"
                "    --passes N      passes to render (16)\n"
                "    --bounces N     depth limit (8)\n"
                "    --seed N        stream seed (236367)\n"
                "    --gpus N        GPUs to tile the frame over (1; 0 = every visible GPU, or KAJO_HIP_GPUS)\n"
                "    --three-arg     construct the backend exactly as a Kajo checkout does, hip::Scheduler(scene, image, preview):\n"
                "                    reference constants, every visible GPU (or KAJO_HIP_GPUS), until the preview closes (--passes)\n"
                "    --scene-pod F   read the scene as a flat binary image of scene::Scene (int32 nSpheres, nPlanes; background 4 f32;\n"
                "                    view 16; projection 16; spheres 39 f32 each; planes 38 f32 each) instead of a JSON file\n"
                "    --batch N       passes per image refresh (0 = automatic: 16 headless, a 30 Hz refresh with a preview)\n"
                "    --exact         numerics: the reference's decisions on every path, fast arithmetic for radiance only (default)\n"
                "    --fast          numerics: hardware transcendentals and contraction everywhere (1.6 x the rate, RMSE ~6e-4)\n"
                "    --strict        numerics: the CPU oracle bit for bit\n"
                "    --gather MODE   rccl | copy (multi-GPU gather transport)\n"
                "    --same-device   put every tile owner on GPU 0 (testing; implies --gather copy)\n"
                "    --force-gather  run the gather + compose step with one GPU too (testing: the RCCL call sequence at N = 1)\n"
                "    --close-at-event K  the headless preview's window closes at the K-th processEvents() call (testing: Esc mid-run)\n"
                "    --no-preview    hand the backend a null Preview* (what renderer/Main.cpp:132 gets without a display): run() renders\n"
                "                    --passes passes (16 when 0) in launches planned for half a second at most\n"
                "    -o FILE         PNG output (out.png)\n"
                "    --raw FILE      also dump the float4 accumulation (W*H*4 floats)\n"
                "    --hdr FILE      also write the mean radiance (the accumulation / passes) as a 3-channel PFM, no exposure or curve\n"
                "    --tonemap CURVE the image's tone curve (-o and --denoise; include/kajo_hip.h kajo_hip_tonemap_argb8): clamp (the\n"
                "                    reference's, default) | reinhard (on luminance, Reinhard et al. 2002) | aces (Narkowicz 2015)\n"
                "    --exposure EV   exposure in stops, -32..32: the mean radiance is scaled by 2^EV before the curve (0)\n"
                "    --white W       reinhard: the exposed luminance mapped to white, >= 0 (0 = none: L / (1 + L))\n"
                "    --auto-exposure scale the frame's log-average luminance to --key (on top of --exposure)\n"
                "    --key K         --auto-exposure: the grey the log-average is mapped to, > 0 (0.18)\n"
                "    --glare STRENGTH  glare (bloom) in front of the tone curve (-o and --denoise; include/kajo_hip.h kajo_hip_glare): the share\n"
                "                    of every pixel's energy, 0..1, spread over its neighbourhood (0 = none, the default; --hdr stays without)\n"
                "    --glare-levels N  --glare: levels of the pyramid, 0..12 (6): the halo's reach doubles with each\n"
                "    --glare-threshold T  --glare: only luminance above T glares, >= 0 (0: every pixel in proportion)\n"
                "    --despeckle     repair NaN / Inf pixels and clamp fireflies in front of the denoiser, the glare and the tone curve (-o and\n"
                "                    --denoise; include/kajo_hip.h kajo_hip_despeckle; any --gpus; --hdr and --raw stay without)\n"
                "    --despeckle-factor F  --despeckle: a pixel is bounded to F times its RANK-th brightest neighbour, F >= 1 (16; 0 = repair only)\n"
                "    --despeckle-rank R  --despeckle: the neighbour measured against, 1..4 (1)\n"
                "    --despeckle-floor X  --despeckle: the least luminance the bound is formed from, >= 0 (0.2)\n"
                "    --meter-exposure Q  meter the frame with a luminance histogram (-o and --denoise; include/kajo_hip.h kajo_hip_meter; any\n"
                "                    --gpus): the exposure that puts the Q-th percentile, 0 < Q <= 1, of the lit pixels at --key; --exposure EV\n"
                "                    is a compensation on top. Not with --auto-exposure (--hdr and --raw stay the raw mean)\n"
                "    --meter-white Q  --tonemap reinhard: the white point from the histogram's Q-th percentile (implies --meter-exposure 0.5)\n"
                "    --aov PREFIX    also write the first-hit AOVs a denoiser takes, averaged over the render's camera samples:\n"
                "                    PREFIX_albedo.pfm, PREFIX_normal.pfm (3 channels), PREFIX_depth.pfm (1; mean over the hits)\n"
                "                    (one GPU only, unless --aov-tiled)\n"
                "    --aov-specular  with --aov or --denoise: take the AOVs at the first non-delta hit, through ideal mirrors and glass\n"
                "                    (include/kajo_hip.h KAJO_FLAG_AOV_SPECULAR), so that the guides show what a mirror shows\n"
                "    --aov-tiled     with --aov, --matte-mask, --matte-ids or --denoise: every GPU keeps the AOVs of its own tiles\n"
                "                    (include/kajo_hip.h KAJO_FLAG_AOV_TILED), so that those options take any --gpus (--same-device too); the\n"
                "                    tiles are gathered and composed when a file is written, not at every refresh (--json: aov_tiled)\n"
                "    --matte-mask FILE  also write the coverage of the objects of --matte-objects as a 1-channel PFM: per pixel the share of\n"
                "                    the camera samples that saw one of them (include/kajo_hip.h kajo_hip_matte_mask; collects the AOVs and\n"
                "                    honours --aov-specular: the object seen in the mirror; one GPU only, unless --aov-tiled)\n"
                "    --matte-objects LIST  --matte-mask: object ids, comma-separated (0 the background, 1.. the planes, then the spheres)\n"
                "    --matte-ids FILE  also write the id of the object that covers most of each pixel as a 1-channel PFM (likewise)\n"
                "    --denoise FILE  also write the frame denoised with those AOVs as guides, as a PNG (edge-aware A-trous filter,\n"
                "                    include/kajo_hip.h kajo_hip_denoise; collects the AOVs; one GPU only, unless --aov-tiled)\n"
                "    --denoise-iterations K  the filter's iterations, 0..8 (5)\n"
                "    --denoise-noise-guided  with --denoise: scale the filter's luminance weight by the measured per-pixel variance of the\n"
                "                    noise estimate where there is one (include/kajo_hip.h KAJO_DENOISE_NOISE_GUIDED); keeps the\n"
                "                    estimate as --noise-map does (launches are cut at multiples of four passes); one GPU, or any\n"
                "                    --gpus with --aov-tiled (--json: denoise_noise_guided, denoise_measured_px)\n"
                "    --json          print run statistics as one JSON line (with a tone option: the scale applied, tone_scale; with a\n"
                "                    matte option: matte_samples per pixel and matte_dropped_pixels, the pixels whose table was full; with a\n"
                "                    meter option: meter_exposure, meter_white, meter_anchor, meter_metered, meter_under, meter_over, meter_stops)\n"
                "    -v              progress on stderr\n"
                "    --local-contrast C  local tone mapping between the glare and the meter (-o and --denoise; include/kajo_hip.h kajo_hip_local;\n"
                "                    any --gpus): the large-scale differences in log luminance are scaled by C, 0 < C <= 1, about the pivot,\n"
                "                    the small-scale ones kept (1 = none, the default; --hdr and --raw stay the raw mean)\n"
                "    --local-detail D  --local-contrast: the factor on the small-scale differences, 0..4 (1)\n"
                "    --local-range STOPS  --local-contrast: differences beyond about this many stops are edges the base layer keeps, > 0 (2)\n"
                "    --local-iterations K  --local-contrast: iterations of the edge-aware filter, 0..8 (5): its reach doubles with each\n"
                "    --local-pivot STOPS|metered[:Q]  --local-contrast: the log2 luminance that stays put, -16..16 (log2(0.18)), or the frame's own\n"
                "                    Q-th percentile, 0 < Q <= 1 (0.5), from the meter's histogram (--json: local_pivot and the parameters used)\n"
                "    --lens-aperture A  depth of field between the denoiser and the glare (-o and --denoise; include/kajo_hip.h kajo_hip_lens): a lens\n"
                "                    blur from the depth AOV, A = the blur radius at infinite depth as a fraction of the height, 0..1 (0 = none).\n"
                "                    Implies the AOVs as --denoise does (--gpus other than 1 needs --aov-tiled; honours --aov-specular); an\n"
                "                    image-space approximation; --hdr and --raw stay the raw mean (--json: lens_focus, lens_max_radius_px)\n"
                "    --lens-focus D  --lens-aperture: the distance in focus, > 0, in the depth AOV's units\n"
                "    --lens-focus-at X,Y  --lens-aperture: focus on what that pixel shows (the default: the frame's centre pixel)\n"
                "    --lens-max-radius R  --lens-aperture: the largest blur radius in pixels, 1..16 (16)\n"
                "    --output-size WxH  the view behind the tone curves (-o; include/kajo_hip.h kajo_hip_present_view_argb8): -o is written at W x H,\n"
                "                    1..16384 each, at most 64 times smaller than the frame, resampled in linear light; any --gpus. --hdr, --raw,\n"
                "                    --aov, --denoise and the matte files stay at the rendered size (--json: view_out_w, view_out_h, view_filter,\n"
                "                    view_scale_x, view_scale_y)\n"
                "    --view X0,Y0,X1,Y1  the view: the part of the frame -o shows, in pixels of the rendered frame, fractions allowed (the whole\n"
                "                    frame); without --output-size the output keeps the frame's size: a zoom\n"
                "    --view-filter nearest|area|triangle|lanczos3  the view: the resampling filter (area: the exact area average)\n"
                "    --supersample K  render and run the whole chain at K w x K h for the given -w -h, K = 2..8, the aspect unchanged, and write -o at\n"
                "                    w x h with the area filter: K x K display-referred pixels averaged per pixel. Not with --output-size\n"
                "    --grade-slope R,G,B  the grade between the denoiser and the lens (-o and --denoise; include/kajo_hip.h kajo_hip_grade): an ASC CDL\n"
                "                    op over the frame in scene-linear radiance, out = max(in * slope + offset, 0) ^ power, then the saturation;\n"
                "                    slopes in 0..65536 (1). Any --gpus. --hdr, --raw, --aov and the matte files stay ungraded (--json: grade_*)\n"
                "    --grade-offset R,G,B  the grade: offsets in -65536..65536 (0)\n"
                "    --grade-power R,G,B  the grade: powers in 1/8..8 (1)\n"
                "    --grade-saturation S  the grade: saturation about the Rec. 709 luminance, 0..4 (1)\n"
                "    --white-balance KELVIN[,TINT]  the grade: gains that make a surface lit by that colour temperature (1667..25000; the blue of\n"
                "                    one below about 1900 is outside sRGB) grey at its own luminance, multiplied into the slope; TINT in -1..1\n"
                "                    stops of green\n"
                "    --white-balance-at X,Y  the grade: the gains that make that pixel of the frame in front of the grade grey\n"
                "    --grade-region IDS:key=v[:key=v...]  the grade: regrade the objects IDS (a comma-separated list of at most 16 ids, as\n"
                "                    --matte-objects) by their coverage mattes; keys slope, offset, power (one number or R,G,B), saturation, amount\n"
                "                    (0..1, 1). Up to four times, applied in order. One GPU, or any --gpus with --aov-tiled\n"
                "    --until-noise E  render until converged (include/kajo_hip.h kajo_hip_noise; any --gpus): stop once the relative error of the\n"
                "                    mean luminance -- its standard error from batches of four passes, over the mean + the floor -- is <= E at\n"
                "                    the quantile Q of the pixels and every pixel has two batches; E >= 0 (0: never). --passes is then not the\n"
                "                    end: --max-passes is (--json: noise_quantile_value, noise_known_px, noise_bad_px, noise_stopped_at_pass)\n"
                "    --noise-quantile Q  --until-noise, --noise-map: the quantile, 0 < Q <= 1 (0.95)\n"
                "    --noise-floor F  --until-noise, --noise-map: the floor added to the mean, > 0 (0.01), so that black pixels do not dominate\n"
                "    --max-passes N  --until-noise: stop after N passes at the latest, N >= 1 (1024)\n"
                "    --adaptive E    adaptive sampling (include/kajo_hip.h kajo_hip_set_adaptive; any --gpus): units of the frame whose pixels' relative\n"
                "                    error is <= E retire and later passes render the others; ends when none is active or after --max-passes\n"
                "                    (1024). With --until-noise: whichever rule ends first. --noise-floor is the rule's floor (--json:\n"
                "                    adaptive_active_units, adaptive_units, adaptive_paths, adaptive_stopped_at_pass)\n"
                "    --adaptive-allowance K  --adaptive: loud pixels a quiet 8x8 block may have, 0..63 (0)\n"
                "    --adaptive-min-passes N  --adaptive: no unit retires before pass N (16)\n"
                "    --adaptive-every B  --adaptive: batches of four passes between decisions (4)\n"
                "    --sample-map FILE.pfm  with --adaptive: also write the per-pixel pass count as a 1-channel PFM\n"
                "    --checkpoint FILE  write the whole accumulated state (include/kajo_hip.h \"Checkpoints\"; any --gpus) to FILE when the run ends, through a\n"
                "                    temporary name (--json: checkpoint_file, checkpoint_passes, resumed_from_passes, frame_digest)\n"
                "    --checkpoint-every N  --checkpoint: also after the refresh that reaches each multiple of N passes, N >= 1\n"
                "    --resume FILE   continue the session of FILE: --passes (--max-passes) is then the total of the whole session. A file written with\n"
                "                    another --gpus is merged into one whole frame first; an --adaptive file resumes only with the --gpus it was\n"
                "                    written with and is refused otherwise\n"
                "    --noise-map FILE  also write the noise map as a 3-channel PFM: mean luminance per pass, its standard error, the relative\n"
                "                    error (-1 where a pixel has fewer than two batches); any --gpus\n"
                "    --png16 FILE.png  also write the image of the whole chain as a 16-bit RGB PNG (include/kajo_hip.h \"The encode\": RGBA16 words\n"
                "                    in place of the 8-bit ones, big-endian samples); any --gpus. Not with --auto-exposure (--meter-exposure works)\n"
                "                    (--json: encode_format, encode_transfer, encode_peak_nits, encode_dither)\n"
                "    --transfer gamma22|srgb|pq  --png16: the transfer function (gamma22, the resolve's curve); pq writes a SMPTE ST 2084 signal\n"
                "                    and a cICP chunk (1, 16, 0, 1)\n"
                "    --peak-nits N   --png16 --transfer pq: the luminance a display value of 1 is shown at, 0 < N <= 10000 (1000)\n"
                "    --dither        write -o through the encode's ARGB8 words with dither instead of the undithered resolve; any --gpus. Not with\n"
                "                    a view option or --auto-exposure\n"
                "    --dither-seed N  --dither: the seed of the pattern, 0 .. 4294967295 (0)\n"
                "    --encode-view   with a view option and --png16 or --dither: write --png16 and --dither's -o at the view's output size through\n"
                "                    the float view (include/kajo_hip.h \"The float view\": resampled between the tone curve and the transfer, the\n"
                "                    dither over output pixels); --dither then goes with a view option; any --gpus. --supersample K --png16 F\n"
                "                    --encode-view is the antialiased 16-bit image (--json: encode_view_out_w, encode_view_out_h)\n",
                program);
    return 1;
}

// The loop: an option that lacks its value, and one that is not known, is passed over; a word without a dash is the scene.
int commandLine(const std::vector<std::string>& args, Raw& r, Arguments& a)
{
    hip::Options& opt = a.opt;
    // the options whose value is kept as text, and the fact that goes with some
    const struct
    {
        const char* name;
        std::string* value;
        bool* given;
    } texts[] = {
        {"-r", &a.rendererName}, {"--scene-pod", &a.podPath}, {"-o", &a.out}, {"--raw", &a.rawOut}, {"--hdr", &a.hdrOut},
        {"--tonemap", &r.toneCurve, &a.toneGiven}, {"--exposure", &r.toneExposure, &a.toneGiven}, {"--white", &r.toneWhite, &a.toneGiven},
        {"--key", &r.toneKey, &a.toneGiven},
        {"--glare", &r.glareStrength}, {"--glare-levels", &r.glareLevels}, {"--glare-threshold", &r.glareThreshold},
        {"--despeckle-factor", &r.despeckleFactor}, {"--despeckle-rank", &r.despeckleRank}, {"--despeckle-floor", &r.despeckleFloor},
        {"--until-noise", &r.untilNoise}, {"--noise-quantile", &r.noiseQuantile}, {"--noise-floor", &r.noiseFloor}, {"--max-passes", &r.maxPasses},
        {"--noise-map", &a.noiseMapOut},
        {"--checkpoint", &opt.checkpointPath}, {"--checkpoint-every", &r.checkpointEvery}, {"--resume", &opt.resumePath},
        {"--adaptive", &r.adaptiveE}, {"--adaptive-allowance", &r.adaptiveAllowance}, {"--adaptive-min-passes", &r.adaptiveMinPasses},
        {"--adaptive-every", &r.adaptiveEvery}, {"--sample-map", &a.sampleMapOut},
        {"--meter-exposure", &r.meterExposure}, {"--meter-white", &r.meterWhite},
        {"--local-contrast", &r.localContrast}, {"--local-detail", &r.localDetail}, {"--local-range", &r.localRange},
        {"--local-iterations", &r.localIterations}, {"--local-pivot", &r.localPivot},
        {"--lens-aperture", &r.lensAperture}, {"--lens-focus", &r.lensFocus}, {"--lens-focus-at", &r.lensFocusAt}, {"--lens-max-radius", &r.lensMaxRadius},
        {"--output-size", &r.outputSize}, {"--view", &r.viewRect}, {"--view-filter", &r.viewFilter}, {"--supersample", &r.supersample},
        {"--png16", &a.png16Out}, {"--transfer", &r.transferName}, {"--peak-nits", &r.peakNits}, {"--dither-seed", &r.ditherSeed},
        {"--grade-slope", &r.gradeSlope}, {"--grade-offset", &r.gradeOffset}, {"--grade-power", &r.gradePower},
        {"--grade-saturation", &r.gradeSaturation}, {"--white-balance", &r.whiteBalance}, {"--white-balance-at", &r.whiteBalanceAt},
        {"--aov", &a.aovPrefix}, {"--matte-mask", &a.matteMaskOut}, {"--matte-objects", &r.matteObjects, &r.matteObjectsGiven},
        {"--matte-ids", &a.matteIdsOut}, {"--denoise", &a.denoiseOut},
    };
    for (size_t i = 1; i < args.size(); i++) {
        const bool more = i + 1 < args.size();
        const std::string& s = args[i];
        bool kept = false;
        for (const auto& t : texts)
            if (more && !kept && s == t.name) {
                *t.value = args[++i];
                if (t.given)
                    *t.given = true;
                kept = true;
            }
        if (kept)
            continue;
        if (s == "--help") return help(args[0].c_str());
        else if (s == "-w" && more) a.width = std::atoi(args[++i].c_str());
        else if (s == "-h" && more) a.height = std::atoi(args[++i].c_str());
        else if (s == "--spp" && more) opt.samplesPerPass = std::atoi(args[++i].c_str());
        else if (s == "--passes" && more) opt.passes = std::atoi(args[++i].c_str());
        else if (s == "--bounces" && more) opt.depthLimit = std::atoi(args[++i].c_str());
        else if (s == "--seed" && more) opt.seed = std::strtoull(args[++i].c_str(), nullptr, 0);
        else if (s == "--gpus" && more) opt.gpus = std::atoi(args[++i].c_str());
        else if (s == "--batch" && more) opt.passesPerUpdate = std::atoi(args[++i].c_str());
        else if (s == "--strict") opt.numerics = hip::Options::Strict;
        else if (s == "--exact") opt.numerics = hip::Options::Exact;
        else if (s == "--fast") opt.numerics = hip::Options::Fast;
        else if (s == "--gather" && more) opt.gather = args[++i] == "copy" ? hip::Options::Copy : hip::Options::Rccl;
        else if (s == "--same-device") { opt.sameDevice = true; opt.gather = hip::Options::Copy; }
        else if (s == "--force-gather") opt.forceGather = true;
        else if (s == "--three-arg") a.threeArg = true;
        else if (s == "--close-at-event" && more) a.closeAtEvent = std::atoi(args[++i].c_str());
        else if (s == "--no-preview") a.noPreview = true;
        else if (s == "--auto-exposure") r.toneAuto = a.toneGiven = true;
        else if (s == "--despeckle") opt.despeckleOn = true;
        else if (s == "--dither") a.dither = true;
        else if (s == "--encode-view") a.encodeView = true;
        else if (s == "--grade-region" && more) r.gradeRegions.push_back(args[++i]);
        else if (s == "--aov-specular") opt.aovSpecular = true;
        else if (s == "--aov-tiled") opt.aovTiled = true;
        else if (s == "--denoise-iterations" && more) a.denoiseIterations = std::atoi(args[++i].c_str());
        else if (s == "--denoise-noise-guided") opt.denoiseNoiseGuided = true; // (the handles keep the noise estimate, as with --noise-map)
        else if (s == "--json") a.json = true;
        else if (s == "-v") a.verbose = true;
        else if (!s.empty() && s[0] != '-') a.scenePath = s;
    }
    return 0;
}

// The stages' options, each before any device is opened: the refusals of the stage's kajo_hip_* call (include/kajo_hip.h), with the
// option's name.

int toneOptions(const Raw& r, Arguments& a) // kajo_hip_tonemap_argb8
{
    if (!a.toneGiven)
        return 0;
    if (a.threeArg)
        return refuseThreeArg("tone");
    KajoToneParams& tone = a.opt.tone;
    if (r.toneCurve == "clamp" || r.toneCurve.empty()) tone.curve = KAJO_TONE_CLAMP;
    else if (r.toneCurve == "reinhard") tone.curve = KAJO_TONE_REINHARD;
    else if (r.toneCurve == "aces") tone.curve = KAJO_TONE_ACES;
    else return refuse("--tonemap must be clamp, reinhard or aces");
    if (!r.toneExposure.empty() && !floatIn(r.toneExposure, -32.0f, 32.0f, &tone.exposure))
        return refuse("--exposure must be a number in -32..32");
    if (!r.toneWhite.empty() && !floatIn(r.toneWhite, 0.0f, INFINITY, &tone.white))
        return refuse("--white must be a finite number >= 0");
    if (!r.toneKey.empty() && !floatIn(r.toneKey, 0.0f, INFINITY, &tone.key, OpenLo))
        return refuse("--key must be a finite number > 0");
    tone.flags = r.toneAuto ? KAJO_TONE_AUTO_EXPOSURE : 0u;
    return 0;
}

int glareOptions(const Raw& r, Arguments& a) // kajo_hip_glare
{
    KajoGlareParams& glare = a.opt.glare;
    if (r.glareStrength.empty()) {
        if (!r.glareLevels.empty() || !r.glareThreshold.empty())
            return refuse("--glare-levels and --glare-threshold shape the glare that --glare STRENGTH turns on: give them with --glare");
        return 0;
    }
    if (a.threeArg)
        return refuseThreeArg("glare");
    if (!floatIn(r.glareStrength, 0.0f, 1.0f, &glare.strength))
        return refuse("--glare must be a number in 0..1");
    if (!r.glareLevels.empty() && !wholeIn(r.glareLevels, 0, 12, &glare.levels))
        return refuse("--glare-levels must be in 0..12");
    if (!r.glareThreshold.empty() && !floatIn(r.glareThreshold, 0.0f, INFINITY, &glare.threshold))
        return refuse("--glare-threshold must be a finite number >= 0");
    a.glareGiven = glare.strength > 0.0f && glare.levels > 0;
    return 0;
}

int despeckleOptions(const Raw& r, Arguments& a) // kajo_hip_despeckle
{
    KajoDespeckleParams& d = a.opt.despeckle;
    if (!a.opt.despeckleOn) {
        if (!r.despeckleFactor.empty() || !r.despeckleRank.empty() || !r.despeckleFloor.empty())
            return refuse("--despeckle-factor, --despeckle-rank and --despeckle-floor shape the stage that --despeckle turns on: give them with --despeckle");
        return 0;
    }
    if (a.threeArg)
        return refuseThreeArg("despeckle");
    kajo_hip_default_despeckle_params(&d);
    if (!r.despeckleFactor.empty() && (!floatIn(r.despeckleFactor, 0.0f, INFINITY, &d.factor) || (d.factor > 0.0f && d.factor < 1.0f)))
        return refuse("--despeckle-factor must be 0 or a finite number >= 1");
    if (!r.despeckleRank.empty() && !wholeIn(r.despeckleRank, 1, 4, &d.rank))
        return refuse("--despeckle-rank must be in 1..4");
    if (!r.despeckleFloor.empty() && !floatIn(r.despeckleFloor, 0.0f, INFINITY, &d.floor))
        return refuse("--despeckle-floor must be a finite number >= 0");
    return 0;
}

int noiseAndAdaptiveOptions(const Raw& r, Arguments& a) // kajo_hip_set_adaptive, then kajo_hip_noise
{
    hip::Options& opt = a.opt;
    if (!a.adaptiveGiven && (!r.adaptiveAllowance.empty() || !r.adaptiveMinPasses.empty() || !r.adaptiveEvery.empty() || !a.sampleMapOut.empty()))
        return refuse("--adaptive-allowance, --adaptive-min-passes, --adaptive-every and --sample-map shape what --adaptive turns on: give them with it");
    if (!a.noiseGiven && !a.adaptiveGiven && (!r.noiseQuantile.empty() || !r.noiseFloor.empty() || !r.maxPasses.empty()))
        return refuse("--noise-quantile, --noise-floor and --max-passes shape what --until-noise or --noise-map turn on: give them with one of the two");
    if (a.adaptiveGiven) {
        if (a.threeArg)
            return refuseThreeArg("adaptive");
        if (!floatIn(r.adaptiveE, 0.0f, INFINITY, &opt.adaptiveTarget, OpenLo))
            return refuse("--adaptive must be a finite number > 0");
        if (!r.adaptiveAllowance.empty() && !wholeIn(r.adaptiveAllowance, 0, 63, &opt.adaptiveAllowance))
            return refuse("--adaptive-allowance must be a whole number in 0..63");
        if (!r.adaptiveMinPasses.empty() && !wholeIn(r.adaptiveMinPasses, 1, 0x7ffffffe, &opt.adaptiveMinPasses))
            return refuse("--adaptive-min-passes must be a whole number >= 1");
        if (!r.adaptiveEvery.empty() && !wholeIn(r.adaptiveEvery, 1, 65536, &opt.adaptiveEvery))
            return refuse("--adaptive-every must be a whole number in 1..65536");
        opt.maxPasses = 1024;
    }
    if (!a.noiseGiven && !a.adaptiveGiven)
        return 0;
    if (a.threeArg)
        return refuseThreeArg("noise");
    const bool rule = !r.untilNoise.empty() || a.adaptiveGiven; // a stop rule: --max-passes is its budget
    opt.noise = true;
    if (!r.untilNoise.empty()) {
        if (!floatIn(r.untilNoise, 0.0f, INFINITY, &opt.noiseTarget))
            return refuse("--until-noise must be a finite number >= 0");
        // E = 0 is hip::Options' "no rule" (noiseTarget 0), and means "never": no estimate is <= 0, so a rule with that target would end
        // no run. The run then takes --max-passes like any pass budget (opt.passes below) and reports the estimate it ends with.
        opt.maxPasses = 1024;
    }
    if (!r.noiseQuantile.empty() && !floatIn(r.noiseQuantile, 0.0f, 1.0f, &opt.noiseQuantile, OpenLo))
        return refuse("--noise-quantile must be a quantile in (0, 1]");
    if (!r.noiseFloor.empty() && !floatIn(r.noiseFloor, 0.0f, INFINITY, &opt.noiseFloor, OpenLo))
        return refuse("--noise-floor must be a finite number > 0");
    if (!r.maxPasses.empty() && (!rule || !wholeIn(r.maxPasses, 1, 0x7ffffffe, &opt.maxPasses)))
        return refuse("--max-passes must be a whole number >= 1, with --until-noise");
    if (rule)
        opt.passes = opt.maxPasses; // (the preview's pass budget and the scheduler's: the rule ends the run before it, or it does)
    return 0;
}

int checkpointOptions(const Raw& r, Arguments& a) // kajo_hip_checkpoint_save and kajo_hip_checkpoint_restore
{
    hip::Options& opt = a.opt;
    if (opt.checkpointPath.empty() && opt.resumePath.empty() && r.checkpointEvery.empty())
        return 0;
    if (a.threeArg)
        return refuseThreeArg("checkpoint");
    if (!r.checkpointEvery.empty() && (opt.checkpointPath.empty() || !wholeIn(r.checkpointEvery, 1, 0x7ffffffe, &opt.checkpointEvery)))
        return refuse("--checkpoint-every must be a whole number >= 1, with --checkpoint");
    return 0;
}

int meterOptions(const Raw& r, Arguments& a) // kajo_hip_meter and kajo_hip_meter_tone
{
    if (!a.meterGiven)
        return 0;
    KajoMeterParams& meter = a.opt.meter;
    if (a.threeArg)
        return refuseThreeArg("meter");
    if (r.toneAuto)
        return refuse("--meter-exposure and --auto-exposure are two automatic exposures: give one");
    if (!r.meterWhite.empty() && a.opt.tone.curve != KAJO_TONE_REINHARD)
        return refuse("--meter-white sets the white point of --tonemap reinhard: give the two together");
    a.opt.meterOn = true;
    kajo_hip_default_meter_params(&meter);
    if (!r.meterExposure.empty() && !floatIn(r.meterExposure, 0.0f, 1.0f, &meter.percentile, OpenLo))
        return refuse("--meter-exposure must be a percentile in (0, 1]");
    if (!r.meterWhite.empty()) {
        if (!floatIn(r.meterWhite, 0.0f, 1.0f, &meter.whitePercentile, OpenLo))
            return refuse("--meter-white must be a percentile in (0, 1]");
        meter.flags |= KAJO_METER_AUTO_WHITE;
    }
    meter.key = a.opt.tone.key; // (--key, checked by toneOptions; 0.18 without)
    return 0;
}

int localOptions(const Raw& r, Arguments& a) // kajo_hip_local
{
    if (!a.localGiven) {
        if (!r.localDetail.empty() || !r.localRange.empty() || !r.localIterations.empty() || !r.localPivot.empty())
            return refuse("--local-detail, --local-range, --local-iterations and --local-pivot shape the stage that --local-contrast turns on: give them with --local-contrast");
        return 0;
    }
    KajoLocalParams& local = a.opt.local;
    if (a.threeArg)
        return refuseThreeArg("local tone mapping");
    a.opt.localOn = true;
    kajo_hip_default_local_params(&local);
    if (!floatIn(r.localContrast, 0.0f, 1.0f, &local.compression, OpenLo))
        return refuse("--local-contrast: local compression must be finite and in (0, 1]");
    if (!r.localDetail.empty() && !floatIn(r.localDetail, 0.0f, 4.0f, &local.detail))
        return refuse("--local-detail: local detail must be finite and in [0, 4]");
    if (!r.localRange.empty() && !floatIn(r.localRange, 0.0f, INFINITY, &local.sigmaRange, OpenLo))
        return refuse("--local-range: local range sigma must be finite and positive");
    if (!r.localIterations.empty() && !wholeIn(r.localIterations, 0, 8, &local.iterations))
        return refuse("--local-iterations: local iterations must be in [0, 8]");
    const std::string& pivot = r.localPivot;
    if (pivot.compare(0, 7, "metered") == 0 && (pivot.size() == 7 || pivot[7] == ':')) {
        local.flags |= KAJO_LOCAL_PIVOT_METERED;
        if (pivot.size() > 7 && !floatIn(pivot.substr(8), 0.0f, 1.0f, &local.pivotPercentile, OpenLo))
            return refuse("--local-pivot metered:Q: local pivot percentile must be finite and in (0, 1]");
    } else if (!pivot.empty() && !floatIn(pivot, -16.0f, 16.0f, &local.pivot))
        return refuse("--local-pivot: local pivot must be finite and in [-16, 16], or metered[:Q]");
    return 0;
}

// the encode: --png16 (RGBA16 words, a transfer) and --dither (ARGB8 words with dither for -o)
int encodeOptions(const Raw& r, Arguments& a)
{
    kajo_hip_default_encode_params(&a.encode16);
    kajo_hip_default_encode_params(&a.encode8);
    if (a.encodeView && a.threeArg)
        return refuseThreeArg("encode", "the options constructor");
    if (a.encodeView && !a.viewGiven)
        return refuse("--encode-view needs a view option (--output-size, --view, --view-filter or --supersample)");
    if (a.encodeView && a.png16Out.empty() && !a.dither)
        return refuse("--encode-view needs --png16 or --dither: it is the encoded images it resamples");
    if (!a.encodeGiven)
        return 0;
    if (a.threeArg)
        return refuseThreeArg("encode", "the options constructor");
    if (a.png16Out.empty() && (!r.transferName.empty() || !r.peakNits.empty()))
        return refuse("--transfer and --peak-nits belong to --png16");
    if (!a.dither && !r.ditherSeed.empty())
        return refuse("--dither-seed belongs to --dither");
    if (r.toneAuto)
        return refuse("--png16 and --dither take no --auto-exposure (its scale is formed inside the tone mapping they replace): use --meter-exposure");
    if (a.dither && a.viewGiven && !a.encodeView)
        return refuse("--dither and a view option are not combined: the view resamples 8-bit words");
    a.encode16.format = KAJO_ENCODE_RGBA16;
    if (!r.transferName.empty()) {
        uint32_t t = 0;
        while (t < KAJO_TRANSFER_LINEAR && r.transferName != transferNames[t]) // (linear is no transfer of a PNG)
            t++;
        if (t == KAJO_TRANSFER_LINEAR)
            return refuse("--transfer must be gamma22, srgb or pq");
        a.encode16.transfer = t;
    }
    if (!r.peakNits.empty()) {
        if (a.encode16.transfer != KAJO_TRANSFER_PQ)
            return refuse("--peak-nits belongs to --transfer pq");
        if (!floatIn(r.peakNits, 0.0f, 10000.0f, &a.encode16.peakNits, OpenLo))
            return refuse("--peak-nits: encode peak luminance must be finite and in (0, 10000] nits");
    }
    if (a.dither) {
        a.encode8.flags = KAJO_ENCODE_DITHER;
        if (!r.ditherSeed.empty()) {
            // (an unsigned 32-bit number: not wholeIn, which would take "-0")
            char* end = nullptr;
            const unsigned long long seed = std::strtoull(r.ditherSeed.c_str(), &end, 10);
            if (end == r.ditherSeed.c_str() || *end != '\0' || r.ditherSeed[0] == '-' || seed > 0xffffffffull)
                return refuse("--dither-seed N must be in 0..4294967295");
            a.encode8.ditherSeed = (uint32_t)seed;
        }
    }
    return 0;
}

int viewOptions(const Raw& r, Arguments& a) // kajo_hip_present_view_argb8
{
    if (!a.viewGiven)
        return 0;
    KajoViewParams& view = a.opt.view;
    if (a.threeArg)
        return refuseThreeArg("view", "the options constructor");
    if (!r.supersample.empty() && !r.outputSize.empty())
        return refuse("--supersample and --output-size are two output sizes: give one");
    a.opt.viewOn = true;
    kajo_hip_default_view_params(&view);
    view.outW = a.width;
    view.outH = a.height;
    if (!r.supersample.empty()) {
        int32_t k = 0;
        if (!wholeIn(r.supersample, 2, 8, &k))
            return refuse("--supersample K must be in 2..8");
        if (!r.viewFilter.empty() && r.viewFilter != "area")
            return refuse("--supersample averages with the area filter: --view-filter must be area with it");
        // (the frame, and everything written at the rendered size, is K times the size asked for; the aspect is unchanged)
        a.width *= k;
        a.height *= k;
    }
    if (!r.outputSize.empty()) {
        int w = 0, h = 0;
        char tail = 0;
        if (std::sscanf(r.outputSize.c_str(), "%dx%d%c", &w, &h, &tail) != 2 || w < 1 || h < 1 || w > KAJO_VIEW_MAX_OUT || h > KAJO_VIEW_MAX_OUT)
            return refuse("--output-size WxH: view output size must be in [1, 16384]");
        view.outW = w;
        view.outH = h;
    }
    if (!r.viewRect.empty()) {
        float v[4];
        char tail = 0;
        if (std::sscanf(r.viewRect.c_str(), "%f,%f,%f,%f%c", &v[0], &v[1], &v[2], &v[3], &tail) != 4 || !std::isfinite(v[0]) || !std::isfinite(v[1]) ||
            !std::isfinite(v[2]) || !std::isfinite(v[3]) || !(0.0f <= v[0] && v[0] < v[2] && v[2] <= (float)a.width) ||
            !(0.0f <= v[1] && v[1] < v[3] && v[3] <= (float)a.height))
            return refuse("--view X0,Y0,X1,Y1: view rectangle must satisfy 0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height");
        view.x0 = v[0], view.y0 = v[1], view.x1 = v[2], view.y1 = v[3];
    }
    if (!r.viewFilter.empty()) {
        uint32_t f = 0;
        while (f < 4 && r.viewFilter != viewFilterNames[f])
            f++;
        if (f == 4)
            return refuse("--view-filter must be nearest, area, triangle or lanczos3");
        view.filter = f;
    }
    a.viewScaleX = (r.viewRect.empty() ? (double)a.width : (double)view.x1 - view.x0) / view.outW;
    a.viewScaleY = (r.viewRect.empty() ? (double)a.height : (double)view.y1 - view.y0) / view.outH;
    if (a.viewScaleX > KAJO_VIEW_MAX_SCALE || a.viewScaleY > KAJO_VIEW_MAX_SCALE)
        return refuse("view minification must be at most 64");
    return 0;
}

int lensOptions(const Raw& r, Arguments& a) // kajo_hip_lens
{
    if (!a.lensGiven) {
        if (!r.lensFocus.empty() || !r.lensFocusAt.empty() || !r.lensMaxRadius.empty())
            return refuse("--lens-focus, --lens-focus-at and --lens-max-radius shape the stage that --lens-aperture turns on: give them with --lens-aperture");
        return 0;
    }
    KajoLensParams& lens = a.opt.lens;
    if (!r.lensFocus.empty() && !r.lensFocusAt.empty())
        return refuse("--lens-focus and --lens-focus-at are two ways to focus: give one");
    if (int rc = needsWholeFrame(a, "--lens-aperture")) // (the stage reads the depth AOV)
        return rc;
    a.opt.lensOn = true;
    kajo_hip_default_lens_params(&lens);
    if (!floatIn(r.lensAperture, 0.0f, 1.0f, &lens.aperture))
        return refuse("--lens-aperture: lens aperture must be finite and in [0, 1]");
    if (!r.lensFocus.empty() && !floatIn(r.lensFocus, 0.0f, INFINITY, &lens.focusDistance, OpenLo))
        return refuse("--lens-focus: lens focus distance must be finite and positive");
    if (!r.lensMaxRadius.empty() && !wholeIn(r.lensMaxRadius, 1, KAJO_LENS_MAX_RADIUS, &lens.maxRadius))
        return refuse("--lens-max-radius: lens max radius must be in [1, 16]");
    if (!r.lensFocusAt.empty()) {
        int x = -1, y = -1;
        if (!pixelIn(r.lensFocusAt, a.width, a.height, &x, &y))
            return refuse("--lens-focus-at X,Y must be a pixel of the frame");
        a.opt.lensFocusAt.x = x;
        a.opt.lensFocusAt.y = y;
    } else if (r.lensFocus.empty()) {
        a.opt.lensFocusAt.x = a.width / 2;
        a.opt.lensFocusAt.y = a.height / 2;
    }
    a.opt.aov = true;
    return 0;
}

// kajo_hip_grade and kajo_hip_grade_white_balance, in the library's own words: text that is no number becomes a NaN, which they refuse
int gradeOptions(const Raw& r, Arguments& a)
{
    if (!a.gradeGiven)
        return 0;
    KajoGradeParams& grade = a.opt.grade;
    if (a.threeArg)
        return refuseThreeArg("grade");
    if (!r.whiteBalance.empty() && !r.whiteBalanceAt.empty())
        return refuse("--white-balance and --white-balance-at are two white balances: give one");
    if (r.gradeRegions.size() > KAJO_GRADE_MAX_REGIONS)
        return refuse("--grade-region can be given four times at the most");
    a.opt.gradeOn = true;
    kajo_hip_default_grade_params(&grade);
    if ((!r.gradeSlope.empty() && !parseTriple(r.gradeSlope, false, grade.global.slope)) ||
        (!r.gradeOffset.empty() && !parseTriple(r.gradeOffset, false, grade.global.offset)) ||
        (!r.gradePower.empty() && !parseTriple(r.gradePower, false, grade.global.power)))
        return refuse("--grade-slope, --grade-offset and --grade-power take three numbers R,G,B");
    if (!r.gradeSaturation.empty() && !parseFloat(r.gradeSaturation, &grade.global.saturation))
        grade.global.saturation = NAN;
    for (const std::string& text : r.gradeRegions)
        if (!parseRegion(text, &grade.regions[grade.nRegions++]))
            return refuse("--grade-region IDS:key=v[:key=v...] takes a comma-separated list of at most 16 object ids (whole numbers >= 0), then "
                          "the keys slope, offset, power (one number or R,G,B), saturation and amount");
    if (kajo_hip_grade_pixels(&grade, nullptr, nullptr, 0, nullptr) != KAJO_OK)
        return refuse(std::string("the grade options: ") + kajo_hip_last_error());
    if (!r.whiteBalance.empty()) {
        const size_t comma = r.whiteBalance.find(',');
        float kelvin = NAN, tint = 0.0f;
        if (!parseFloat(r.whiteBalance.substr(0, comma), &kelvin))
            kelvin = NAN;
        if (comma != std::string::npos && !parseFloat(r.whiteBalance.substr(comma + 1), &tint))
            tint = NAN;
        float gains[3];
        if (kajo_hip_grade_white_balance(kelvin, tint, gains) != KAJO_OK)
            return refuse(std::string("--white-balance KELVIN[,TINT]: ") + kajo_hip_last_error());
        a.whiteBalanceGiven = true;
        a.whiteBalanceKelvin = kelvin;
        a.whiteBalanceTint = tint;
        // (into the slope in binary64, rounded once; the product stays inside the slope's range or the library refuses it below)
        for (int c = 0; c < 3; c++)
            grade.global.slope[c] = (float)((double)grade.global.slope[c] * (double)gains[c]);
        if (kajo_hip_grade_pixels(&grade, nullptr, nullptr, 0, nullptr) != KAJO_OK)
            return refuse(std::string("the grade options: ") + kajo_hip_last_error());
    }
    if (!r.whiteBalanceAt.empty() && !pixelIn(r.whiteBalanceAt, a.width, a.height, &a.opt.gradeNeutralAt.x, &a.opt.gradeNeutralAt.y))
        return refuse("--white-balance-at X,Y must be a pixel of the frame");
    if (grade.nRegions > 0) {
        // (the regions read the coverage tables kept beside the AOV buffers of the one handle: the same condition as --matte-mask)
        if (a.opt.gpus != 1 && !a.opt.aovTiled)
            return refuse("--grade-region needs the whole frame's mattes: --gpus 1, or any --gpus with --aov-tiled");
        a.opt.aov = true;
        a.opt.matte = true;
    }
    return 0;
}

int aovMatteDenoiseOptions(const Raw& r, Arguments& a)
{
    hip::Options& opt = a.opt;
    const bool readsAov = !a.aovPrefix.empty() || !a.denoiseOut.empty() || a.matteGiven || a.lensGiven || (a.gradeGiven && opt.grade.nRegions > 0);
    if (opt.aovSpecular && !readsAov)
        return refuse("--aov-specular changes the AOVs that --aov writes and --denoise is guided by: give it with --aov or --denoise");
    if (opt.aovTiled && !readsAov)
        return refuse("--aov-tiled changes where the AOVs of --aov, --matte-mask, --matte-ids and --denoise are kept: give it with one of them");
    if (!a.aovPrefix.empty()) {
        if (int rc = needsWholeFrame(a, "--aov"))
            return rc;
        opt.aov = true;
    }
    if (r.matteObjectsGiven != !a.matteMaskOut.empty())
        return refuse("--matte-mask FILE writes the coverage of the objects --matte-objects LIST names: give the two together");
    if (a.matteGiven) {
        // (the coverage tables are kept beside the AOV buffers)
        if (int rc = needsWholeFrame(a, a.matteMaskOut.empty() ? "--matte-ids" : "--matte-mask"))
            return rc;
        if (r.matteObjectsGiven && !parseObjects(r.matteObjects, &a.matteObjects))
            return refuse("--matte-objects must be a comma-separated list of object ids (whole numbers >= 0)");
        opt.aov = true;
        opt.matte = true;
    }
    if (!a.denoiseOut.empty()) {
        if (int rc = needsWholeFrame(a, "--denoise"))
            return rc;
        if (a.denoiseIterations < 0 || a.denoiseIterations > 8)
            return refuse("--denoise-iterations must be in 0..8");
        opt.aov = true;
    }
    if (opt.denoiseNoiseGuided && a.denoiseOut.empty())
        return refuse("--denoise-noise-guided needs --denoise: it steers that filter");
    return 0;
}

} // namespace

int parseArguments(int argc, char** argv, Arguments* out)
{
    Arguments& a = *out;
    Raw r;
    a.opt.passes = 16;
    a.opt.gpus = 1;
    if (int rc = commandLine(std::vector<std::string>(argv, argv + argc), r, a))
        return rc;
    if (a.width <= 0 || a.height <= 0) {
        std::cerr << "Bad image size" << std::endl;
        return 1;
    }
    // which stages' options were given: each fact once (glareGiven: by glareOptions, from the values)
    a.adaptiveGiven = !r.adaptiveE.empty();
    a.noiseGiven = !r.untilNoise.empty() || !a.noiseMapOut.empty();
    a.meterGiven = !r.meterExposure.empty() || !r.meterWhite.empty();
    a.localGiven = !r.localContrast.empty();
    a.viewGiven = !r.outputSize.empty() || !r.viewRect.empty() || !r.viewFilter.empty() || !r.supersample.empty();
    a.encodeGiven = !a.png16Out.empty() || a.dither || !r.transferName.empty() || !r.peakNits.empty() || !r.ditherSeed.empty();
    a.lensGiven = !r.lensAperture.empty();
    a.gradeGiven = !r.gradeSlope.empty() || !r.gradeOffset.empty() || !r.gradePower.empty() || !r.gradeSaturation.empty() || !r.whiteBalance.empty() ||
                   !r.whiteBalanceAt.empty() || !r.gradeRegions.empty();
    a.matteGiven = !a.matteMaskOut.empty() || !a.matteIdsOut.empty();
    // (in this order: a later stage reads what an earlier one set -- the meter the tone's key and curve, the lens and the grade the size
    // the view left)
    for (auto stage : {toneOptions, glareOptions, despeckleOptions, noiseAndAdaptiveOptions, checkpointOptions, meterOptions, localOptions, encodeOptions, viewOptions,
                       lensOptions, gradeOptions, aovMatteDenoiseOptions})
        if (int rc = stage(r, a))
            return rc;
    a.opt.counters = a.json;
    return 0;
}
