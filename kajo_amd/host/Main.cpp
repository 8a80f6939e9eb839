// Main.cpp -- headless driver with the reference's command line (renderer/Main.cpp:97-146):
//   kajo_render [-w SIZE] [-h SIZE] [-r hip] [options] SCENE.json     (no SCENE: the built-in test scene)
// plus what a window-less run needs: a pass budget, an output name and the backend's options.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "HipScheduler.h"
#include "Image.h"
#include "kajo_hip.h"
#include "Preview.h"
#include "scene/Scene.h"

namespace
{

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

// a comma-separated list of object ids (whole numbers >= 0, at least one), or false
bool parseObjects(const std::string& text, std::vector<int32_t>* out)
{
    out->clear();
    size_t at = 0;
    while (true) {
        const size_t comma = text.find(',', at);
        const std::string item = text.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        char* end = nullptr;
        const long v = std::strtol(item.c_str(), &end, 10);
        if (item.empty() || item.size() > 9 || *end != '\0' || item[0] < '0' || item[0] > '9')
            return false;
        out->push_back((int32_t)v);
        if (comma == std::string::npos)
            return true;
        at = comma + 1;
    }
}

// three numbers R,G,B -- or, where `orOne`, one number for all three; text that is no number becomes a NaN (the library refuses it by name)
bool parseTriple(const std::string& text, bool orOne, float out[3])
{
    std::vector<std::string> items;
    size_t at = 0;
    while (true) {
        const size_t comma = text.find(',', at);
        items.push_back(text.substr(at, comma == std::string::npos ? std::string::npos : comma - at));
        if (comma == std::string::npos)
            break;
        at = comma + 1;
    }
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
    std::vector<std::string> parts;
    size_t at = 0;
    while (true) {
        const size_t colon = text.find(':', at);
        parts.push_back(text.substr(at, colon == std::string::npos ? std::string::npos : colon - at));
        if (colon == std::string::npos)
            break;
        at = colon + 1;
    }
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

} // namespace

int main(int argc, char** argv)
{
    std::vector<std::string> args(argv, argv + argc);
    std::string rendererName = "hip", out = "out.png", rawOut, aovPrefix, denoiseOut, hdrOut, scenePath;
    // matte options (include/kajo_hip.h kajo_hip_matte_mask): the list's raw text, checked after the loop
    std::string matteMaskOut, matteIdsOut, matteObjectsText;
    bool matteObjectsGiven = false;
    std::vector<int32_t> matteObjects;
    // tone options (include/kajo_hip.h KajoToneParams): the raw text, checked after the loop; toneGiven = any of them was given
    std::string toneCurve, toneExposure, toneWhite, toneKey;
    bool toneAuto = false, toneGiven = false;
    // glare options (include/kajo_hip.h KajoGlareParams): the raw text, checked after the loop
    std::string glareStrength, glareLevels, glareThreshold;
    // despeckle options (include/kajo_hip.h KajoDespeckleParams): the raw text, checked after the loop
    std::string despeckleFactor, despeckleRank, despeckleFloor;
    bool despeckle = false;
    // meter options (include/kajo_hip.h KajoMeterParams): the raw text, checked after the loop
    std::string meterExposure, meterWhite;
    std::string untilNoise, noiseQuantile, noiseFloor, maxPasses, noiseMapOut;
    std::string adaptiveE, adaptiveAllowance, adaptiveMinPasses, adaptiveEvery, sampleMapOut;
    // local tone mapping options (include/kajo_hip.h KajoLocalParams): the raw text, checked after the loop
    std::string localContrast, localDetail, localRange, localIterations, localPivot;
    // depth of field options (include/kajo_hip.h KajoLensParams): the raw text, checked after the loop
    std::string lensAperture, lensFocus, lensFocusAt, lensMaxRadius;
    // view options (include/kajo_hip.h KajoViewParams): the raw text, checked after the loop
    std::string outputSize, viewRect, viewFilter, supersample;
    std::string png16Out, transferName, peakNits, ditherSeed;
    bool dither = false;
    // grade options (include/kajo_hip.h KajoGradeParams): the raw text, checked after the loop
    std::string gradeSlope, gradeOffset, gradePower, gradeSaturation, whiteBalance, whiteBalanceAt;
    std::vector<std::string> gradeRegions;
    int width = 640, height = 480;
    int denoiseIterations = 5;
    hip::Options opt;
    opt.passes = 16;
    opt.gpus = 1;
    std::string podPath;
    bool verbose = false, json = false, threeArg = false, aovSpecular = false, aovTiled = false, denoiseNoiseGuided = false;
    int closeAtEvent = 0;
    bool noPreview = false;
    for (size_t i = 1; i < args.size(); i++) {
        bool more = i + 1 < args.size();
        const std::string& a = args[i];
        if (a == "--help") {
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
                        "    --dither-seed N  --dither: the seed of the pattern, 0 .. 4294967295 (0)\n",
                        args[0].c_str());
            return 1;
        } else if (a == "-w" && more) width = std::atoi(args[++i].c_str());
        else if (a == "-h" && more) height = std::atoi(args[++i].c_str());
        else if (a == "-r" && more) rendererName = args[++i];
        else if (a == "--spp" && more) opt.samplesPerPass = std::atoi(args[++i].c_str());
        else if (a == "--passes" && more) opt.passes = std::atoi(args[++i].c_str());
        else if (a == "--bounces" && more) opt.depthLimit = std::atoi(args[++i].c_str());
        else if (a == "--seed" && more) opt.seed = std::strtoull(args[++i].c_str(), nullptr, 0);
        else if (a == "--gpus" && more) opt.gpus = std::atoi(args[++i].c_str());
        else if (a == "--batch" && more) opt.passesPerUpdate = std::atoi(args[++i].c_str());
        else if (a == "--strict") opt.numerics = hip::Options::Strict;
        else if (a == "--exact") opt.numerics = hip::Options::Exact;
        else if (a == "--fast") opt.numerics = hip::Options::Fast;
        else if (a == "--gather" && more) opt.gather = args[++i] == "copy" ? hip::Options::Copy : hip::Options::Rccl;
        else if (a == "--same-device") { opt.sameDevice = true; opt.gather = hip::Options::Copy; }
        else if (a == "--force-gather") opt.forceGather = true;
        else if (a == "--three-arg") threeArg = true;
        else if (a == "--close-at-event" && more) closeAtEvent = std::atoi(args[++i].c_str());
        else if (a == "--no-preview") noPreview = true;
        else if (a == "--scene-pod" && more) podPath = args[++i];
        else if (a == "-o" && more) out = args[++i];
        else if (a == "--raw" && more) rawOut = args[++i];
        else if (a == "--hdr" && more) hdrOut = args[++i];
        else if (a == "--tonemap" && more) { toneCurve = args[++i]; toneGiven = true; }
        else if (a == "--exposure" && more) { toneExposure = args[++i]; toneGiven = true; }
        else if (a == "--white" && more) { toneWhite = args[++i]; toneGiven = true; }
        else if (a == "--auto-exposure") { toneAuto = true; toneGiven = true; }
        else if (a == "--key" && more) { toneKey = args[++i]; toneGiven = true; }
        else if (a == "--glare" && more) glareStrength = args[++i];
        else if (a == "--glare-levels" && more) glareLevels = args[++i];
        else if (a == "--glare-threshold" && more) glareThreshold = args[++i];
        else if (a == "--despeckle") despeckle = true;
        else if (a == "--despeckle-factor" && more) despeckleFactor = args[++i];
        else if (a == "--despeckle-rank" && more) despeckleRank = args[++i];
        else if (a == "--despeckle-floor" && more) despeckleFloor = args[++i];
        else if (a == "--until-noise" && more) untilNoise = args[++i];
        else if (a == "--noise-quantile" && more) noiseQuantile = args[++i];
        else if (a == "--noise-floor" && more) noiseFloor = args[++i];
        else if (a == "--max-passes" && more) maxPasses = args[++i];
        else if (a == "--noise-map" && more) noiseMapOut = args[++i];
        else if (a == "--adaptive" && more) adaptiveE = args[++i];
        else if (a == "--adaptive-allowance" && more) adaptiveAllowance = args[++i];
        else if (a == "--adaptive-min-passes" && more) adaptiveMinPasses = args[++i];
        else if (a == "--adaptive-every" && more) adaptiveEvery = args[++i];
        else if (a == "--sample-map" && more) sampleMapOut = args[++i];
        else if (a == "--meter-exposure" && more) meterExposure = args[++i];
        else if (a == "--meter-white" && more) meterWhite = args[++i];
        else if (a == "--local-contrast" && more) localContrast = args[++i];
        else if (a == "--local-detail" && more) localDetail = args[++i];
        else if (a == "--local-range" && more) localRange = args[++i];
        else if (a == "--local-iterations" && more) localIterations = args[++i];
        else if (a == "--local-pivot" && more) localPivot = args[++i];
        else if (a == "--lens-aperture" && more) lensAperture = args[++i];
        else if (a == "--lens-focus" && more) lensFocus = args[++i];
        else if (a == "--lens-focus-at" && more) lensFocusAt = args[++i];
        else if (a == "--lens-max-radius" && more) lensMaxRadius = args[++i];
        else if (a == "--output-size" && more) outputSize = args[++i];
        else if (a == "--view" && more) viewRect = args[++i];
        else if (a == "--view-filter" && more) viewFilter = args[++i];
        else if (a == "--supersample" && more) supersample = args[++i];
        else if (a == "--png16" && more) png16Out = args[++i];
        else if (a == "--transfer" && more) transferName = args[++i];
        else if (a == "--peak-nits" && more) peakNits = args[++i];
        else if (a == "--dither") dither = true;
        else if (a == "--dither-seed" && more) ditherSeed = args[++i];
        else if (a == "--grade-slope" && more) gradeSlope = args[++i];
        else if (a == "--grade-offset" && more) gradeOffset = args[++i];
        else if (a == "--grade-power" && more) gradePower = args[++i];
        else if (a == "--grade-saturation" && more) gradeSaturation = args[++i];
        else if (a == "--white-balance" && more) whiteBalance = args[++i];
        else if (a == "--white-balance-at" && more) whiteBalanceAt = args[++i];
        else if (a == "--grade-region" && more) gradeRegions.push_back(args[++i]);
        else if (a == "--aov" && more) aovPrefix = args[++i];
        else if (a == "--aov-specular") aovSpecular = true;
        else if (a == "--aov-tiled") aovTiled = true;
        else if (a == "--matte-mask" && more) matteMaskOut = args[++i];
        else if (a == "--matte-objects" && more) { matteObjectsText = args[++i]; matteObjectsGiven = true; }
        else if (a == "--matte-ids" && more) matteIdsOut = args[++i];
        else if (a == "--denoise" && more) denoiseOut = args[++i];
        else if (a == "--denoise-iterations" && more) denoiseIterations = std::atoi(args[++i].c_str());
        else if (a == "--denoise-noise-guided") denoiseNoiseGuided = true;
        else if (a == "--json") json = true;
        else if (a == "-v") verbose = true;
        else if (!a.empty() && a[0] != '-') scenePath = a;
    }
    if (width <= 0 || height <= 0) {
        std::cerr << "Bad image size" << std::endl;
        return 1;
    }
    if (toneGiven) {
        // (before any device is opened: the refusals of kajo_hip_tonemap_argb8, with the option's name)
        if (threeArg) {
            std::cerr << "kajo_render: the tone options need the backend's options (without --three-arg)" << std::endl;
            return 1;
        }
        if (toneCurve == "clamp" || toneCurve.empty()) opt.tone.curve = KAJO_TONE_CLAMP;
        else if (toneCurve == "reinhard") opt.tone.curve = KAJO_TONE_REINHARD;
        else if (toneCurve == "aces") opt.tone.curve = KAJO_TONE_ACES;
        else {
            std::cerr << "kajo_render: --tonemap must be clamp, reinhard or aces" << std::endl;
            return 1;
        }
        if (!toneExposure.empty() && (!parseFloat(toneExposure, &opt.tone.exposure) || opt.tone.exposure < -32.0f || opt.tone.exposure > 32.0f)) {
            std::cerr << "kajo_render: --exposure must be a number in -32..32" << std::endl;
            return 1;
        }
        if (!toneWhite.empty() && (!parseFloat(toneWhite, &opt.tone.white) || opt.tone.white < 0.0f)) {
            std::cerr << "kajo_render: --white must be a finite number >= 0" << std::endl;
            return 1;
        }
        if (!toneKey.empty() && (!parseFloat(toneKey, &opt.tone.key) || opt.tone.key <= 0.0f)) {
            std::cerr << "kajo_render: --key must be a finite number > 0" << std::endl;
            return 1;
        }
        opt.tone.flags = toneAuto ? KAJO_TONE_AUTO_EXPOSURE : 0u;
    }
    if (glareStrength.empty() && (!glareLevels.empty() || !glareThreshold.empty())) {
        std::cerr << "kajo_render: --glare-levels and --glare-threshold shape the glare that --glare STRENGTH turns on: give them with --glare" << std::endl;
        return 1;
    }
    if (!glareStrength.empty()) {
        // (before any device is opened: the refusals of kajo_hip_glare, with the option's name)
        if (threeArg) {
            std::cerr << "kajo_render: the glare options need the backend's options (without --three-arg)" << std::endl;
            return 1;
        }
        if (!parseFloat(glareStrength, &opt.glare.strength) || opt.glare.strength < 0.0f || opt.glare.strength > 1.0f) {
            std::cerr << "kajo_render: --glare must be a number in 0..1" << std::endl;
            return 1;
        }
        if (!glareLevels.empty()) {
            char* end = nullptr;
            const long n = std::strtol(glareLevels.c_str(), &end, 10);
            if (*end != '\0' || n < 0 || n > 12) {
                std::cerr << "kajo_render: --glare-levels must be in 0..12" << std::endl;
                return 1;
            }
            opt.glare.levels = (int32_t)n;
        }
        if (!glareThreshold.empty() && (!parseFloat(glareThreshold, &opt.glare.threshold) || opt.glare.threshold < 0.0f)) {
            std::cerr << "kajo_render: --glare-threshold must be a finite number >= 0" << std::endl;
            return 1;
        }
    }
    const bool glareGiven = opt.glare.strength > 0.0f && opt.glare.levels > 0;
    if (!despeckle && (!despeckleFactor.empty() || !despeckleRank.empty() || !despeckleFloor.empty())) {
        std::cerr << "kajo_render: --despeckle-factor, --despeckle-rank and --despeckle-floor shape the stage that --despeckle turns on: give them with --despeckle" << std::endl;
        return 1;
    }
    if (despeckle) {
        // (before any device is opened: the refusals of kajo_hip_despeckle, with the option's name)
        if (threeArg) {
            std::cerr << "kajo_render: the despeckle options need the backend's options (without --three-arg)" << std::endl;
            return 1;
        }
        opt.despeckleOn = true;
        kajo_hip_default_despeckle_params(&opt.despeckle);
        if (!despeckleFactor.empty() && (!parseFloat(despeckleFactor, &opt.despeckle.factor) || opt.despeckle.factor < 0.0f ||
                                         (opt.despeckle.factor > 0.0f && opt.despeckle.factor < 1.0f))) {
            std::cerr << "kajo_render: --despeckle-factor must be 0 or a finite number >= 1" << std::endl;
            return 1;
        }
        if (!despeckleRank.empty()) {
            char* end = nullptr;
            const long n = std::strtol(despeckleRank.c_str(), &end, 10);
            if (*end != '\0' || n < 1 || n > 4) {
                std::cerr << "kajo_render: --despeckle-rank must be in 1..4" << std::endl;
                return 1;
            }
            opt.despeckle.rank = (int32_t)n;
        }
        if (!despeckleFloor.empty() && (!parseFloat(despeckleFloor, &opt.despeckle.floor) || opt.despeckle.floor < 0.0f)) {
            std::cerr << "kajo_render: --despeckle-floor must be a finite number >= 0" << std::endl;
            return 1;
        }
    }
    const bool adaptiveGiven = !adaptiveE.empty();
    if (!adaptiveGiven && (!adaptiveAllowance.empty() || !adaptiveMinPasses.empty() || !adaptiveEvery.empty() || !sampleMapOut.empty())) {
        std::cerr << "kajo_render: --adaptive-allowance, --adaptive-min-passes, --adaptive-every and --sample-map shape what --adaptive turns on: give them with it" << std::endl;
        return 1;
    }
    const bool noiseGiven = !untilNoise.empty() || !noiseMapOut.empty();
    if (!noiseGiven && !adaptiveGiven && (!noiseQuantile.empty() || !noiseFloor.empty() || !maxPasses.empty())) {
        std::cerr << "kajo_render: --noise-quantile, --noise-floor and --max-passes shape what --until-noise or --noise-map turn on: give them with one of the two" << std::endl;
        return 1;
    }
    if (adaptiveGiven) {
        // (before any device is opened: the refusals of kajo_hip_set_adaptive, with the option's name)
        if (threeArg) {
            std::cerr << "kajo_render: the adaptive options need the backend's options (without --three-arg)" << std::endl;
            return 1;
        }
        if (!parseFloat(adaptiveE, &opt.adaptiveTarget) || !(opt.adaptiveTarget > 0.0f)) {
            std::cerr << "kajo_render: --adaptive must be a finite number > 0" << std::endl;
            return 1;
        }
        auto whole = [](const std::string& text, long lo, long hi, int* out) {
            char* end = nullptr;
            const long n = std::strtol(text.c_str(), &end, 10);
            if (end == text.c_str() || *end || n < lo || n > hi)
                return false;
            *out = (int)n;
            return true;
        };
        if (!adaptiveAllowance.empty() && !whole(adaptiveAllowance, 0, 63, &opt.adaptiveAllowance)) {
            std::cerr << "kajo_render: --adaptive-allowance must be a whole number in 0..63" << std::endl;
            return 1;
        }
        if (!adaptiveMinPasses.empty() && !whole(adaptiveMinPasses, 1, 0x7ffffffe, &opt.adaptiveMinPasses)) {
            std::cerr << "kajo_render: --adaptive-min-passes must be a whole number >= 1" << std::endl;
            return 1;
        }
        if (!adaptiveEvery.empty() && !whole(adaptiveEvery, 1, 65536, &opt.adaptiveEvery)) {
            std::cerr << "kajo_render: --adaptive-every must be a whole number in 1..65536" << std::endl;
            return 1;
        }
        opt.maxPasses = 1024;
    }
    if (noiseGiven || adaptiveGiven) {
        // (before any device is opened: the refusals of kajo_hip_noise, with the option's name)
        if (threeArg) {
            std::cerr << "kajo_render: the noise options need the backend's options (without --three-arg)" << std::endl;
            return 1;
        }
        opt.noise = true;
        if (!untilNoise.empty()) {
            if (!parseFloat(untilNoise, &opt.noiseTarget) || opt.noiseTarget < 0.0f) {
                std::cerr << "kajo_render: --until-noise must be a finite number >= 0" << std::endl;
                return 1;
            }
            // E = 0 is hip::Options' "no rule" (noiseTarget 0), and means "never": no estimate is <= 0, so a rule with that target would end
            // no run. The run then takes --max-passes like any pass budget (opt.passes below) and reports the estimate it ends with.
            opt.maxPasses = 1024;
        }
        if (!noiseQuantile.empty() && (!parseFloat(noiseQuantile, &opt.noiseQuantile) || opt.noiseQuantile <= 0.0f || opt.noiseQuantile > 1.0f)) {
            std::cerr << "kajo_render: --noise-quantile must be a quantile in (0, 1]" << std::endl;
            return 1;
        }
        if (!noiseFloor.empty() && (!parseFloat(noiseFloor, &opt.noiseFloor) || !(opt.noiseFloor > 0.0f))) {
            std::cerr << "kajo_render: --noise-floor must be a finite number > 0" << std::endl;
            return 1;
        }
        if (!maxPasses.empty()) {
            char* end = nullptr;
            const long n = std::strtol(maxPasses.c_str(), &end, 10);
            if ((untilNoise.empty() && !adaptiveGiven) || end == maxPasses.c_str() || *end || n < 1 || n > 0x7ffffffe) {
                std::cerr << "kajo_render: --max-passes must be a whole number >= 1, with --until-noise" << std::endl;
                return 1;
            }
            opt.maxPasses = (int)n;
        }
        if (!untilNoise.empty() || adaptiveGiven)
            opt.passes = opt.maxPasses; // (the preview's pass budget and the scheduler's: the rule ends the run before it, or it does)
    }
    const bool meterGiven = !meterExposure.empty() || !meterWhite.empty();
    if (meterGiven) {
        // (before any device is opened: the refusals of kajo_hip_meter and of kajo_hip_meter_tone, with the option's name)
        if (threeArg) {
            std::cerr << "kajo_render: the meter options need the backend's options (without --three-arg)" << std::endl;
            return 1;
        }
        if (toneAuto) {
            std::cerr << "kajo_render: --meter-exposure and --auto-exposure are two automatic exposures: give one" << std::endl;
            return 1;
        }
        if (!meterWhite.empty() && opt.tone.curve != KAJO_TONE_REINHARD) {
            std::cerr << "kajo_render: --meter-white sets the white point of --tonemap reinhard: give the two together" << std::endl;
            return 1;
        }
        opt.meterOn = true;
        kajo_hip_default_meter_params(&opt.meter);
        if (!meterExposure.empty() && (!parseFloat(meterExposure, &opt.meter.percentile) || opt.meter.percentile <= 0.0f || opt.meter.percentile > 1.0f)) {
            std::cerr << "kajo_render: --meter-exposure must be a percentile in (0, 1]" << std::endl;
            return 1;
        }
        if (!meterWhite.empty()) {
            if (!parseFloat(meterWhite, &opt.meter.whitePercentile) || opt.meter.whitePercentile <= 0.0f || opt.meter.whitePercentile > 1.0f) {
                std::cerr << "kajo_render: --meter-white must be a percentile in (0, 1]" << std::endl;
                return 1;
            }
            opt.meter.flags |= KAJO_METER_AUTO_WHITE;
        }
        opt.meter.key = opt.tone.key; // (--key, checked above; 0.18 without)
    }
    if (localContrast.empty() && (!localDetail.empty() || !localRange.empty() || !localIterations.empty() || !localPivot.empty())) {
        std::cerr << "kajo_render: --local-detail, --local-range, --local-iterations and --local-pivot shape the stage that --local-contrast turns on: give them with --local-contrast" << std::endl;
        return 1;
    }
    const bool localGiven = !localContrast.empty();
    if (localGiven) {
        // (before any device is opened: the refusals of kajo_hip_local, with the option's name)
        if (threeArg) {
            std::cerr << "kajo_render: the local tone mapping options need the backend's options (without --three-arg)" << std::endl;
            return 1;
        }
        opt.localOn = true;
        kajo_hip_default_local_params(&opt.local);
        if (!parseFloat(localContrast, &opt.local.compression) || opt.local.compression <= 0.0f || opt.local.compression > 1.0f) {
            std::cerr << "kajo_render: --local-contrast: local compression must be finite and in (0, 1]" << std::endl;
            return 1;
        }
        if (!localDetail.empty() && (!parseFloat(localDetail, &opt.local.detail) || opt.local.detail < 0.0f || opt.local.detail > 4.0f)) {
            std::cerr << "kajo_render: --local-detail: local detail must be finite and in [0, 4]" << std::endl;
            return 1;
        }
        if (!localRange.empty() && (!parseFloat(localRange, &opt.local.sigmaRange) || opt.local.sigmaRange <= 0.0f)) {
            std::cerr << "kajo_render: --local-range: local range sigma must be finite and positive" << std::endl;
            return 1;
        }
        if (!localIterations.empty()) {
            char* end = nullptr;
            const long n = std::strtol(localIterations.c_str(), &end, 10);
            if (*end != '\0' || n < 0 || n > 8) {
                std::cerr << "kajo_render: --local-iterations: local iterations must be in [0, 8]" << std::endl;
                return 1;
            }
            opt.local.iterations = (int32_t)n;
        }
        if (localPivot.compare(0, 7, "metered") == 0 && (localPivot.size() == 7 || localPivot[7] == ':')) {
            opt.local.flags |= KAJO_LOCAL_PIVOT_METERED;
            if (localPivot.size() > 7 && (!parseFloat(localPivot.substr(8), &opt.local.pivotPercentile) || opt.local.pivotPercentile <= 0.0f ||
                                          opt.local.pivotPercentile > 1.0f)) {
                std::cerr << "kajo_render: --local-pivot metered:Q: local pivot percentile must be finite and in (0, 1]" << std::endl;
                return 1;
            }
        } else if (!localPivot.empty() && (!parseFloat(localPivot, &opt.local.pivot) || opt.local.pivot < -16.0f || opt.local.pivot > 16.0f)) {
            std::cerr << "kajo_render: --local-pivot: local pivot must be finite and in [-16, 16], or metered[:Q]" << std::endl;
            return 1;
        }
    }
    const bool viewGiven = !outputSize.empty() || !viewRect.empty() || !viewFilter.empty() || !supersample.empty();
    // the encode: --png16 (RGBA16 words, a transfer) and --dither (ARGB8 words with dither for -o). Before any device is opened: the
    // refusals, with the option's name
    const bool encodeGiven = !png16Out.empty() || dither || !transferName.empty() || !peakNits.empty() || !ditherSeed.empty();
    const char* transferNames[] = {"gamma22", "srgb", "pq", "linear"};
    KajoEncodeParams encode16, encode8;
    kajo_hip_default_encode_params(&encode16);
    kajo_hip_default_encode_params(&encode8);
    if (encodeGiven) {
        if (threeArg) {
            std::cerr << "kajo_render: the encode options need the options constructor (without --three-arg)" << std::endl;
            return 1;
        }
        if (png16Out.empty() && (!transferName.empty() || !peakNits.empty())) {
            std::cerr << "kajo_render: --transfer and --peak-nits belong to --png16" << std::endl;
            return 1;
        }
        if (!dither && !ditherSeed.empty()) {
            std::cerr << "kajo_render: --dither-seed belongs to --dither" << std::endl;
            return 1;
        }
        if (toneAuto) {
            std::cerr << "kajo_render: --png16 and --dither take no --auto-exposure (its scale is formed inside the tone mapping they replace): "
                         "use --meter-exposure" << std::endl;
            return 1;
        }
        if (dither && viewGiven) {
            std::cerr << "kajo_render: --dither and a view option are not combined: the view resamples 8-bit words" << std::endl;
            return 1;
        }
        encode16.format = KAJO_ENCODE_RGBA16;
        if (!transferName.empty()) {
            if (transferName == "gamma22") encode16.transfer = KAJO_TRANSFER_GAMMA22;
            else if (transferName == "srgb") encode16.transfer = KAJO_TRANSFER_SRGB;
            else if (transferName == "pq") encode16.transfer = KAJO_TRANSFER_PQ;
            else {
                std::cerr << "kajo_render: --transfer must be gamma22, srgb or pq" << std::endl;
                return 1;
            }
        }
        if (!peakNits.empty()) {
            if (encode16.transfer != KAJO_TRANSFER_PQ) {
                std::cerr << "kajo_render: --peak-nits belongs to --transfer pq" << std::endl;
                return 1;
            }
            if (!parseFloat(peakNits, &encode16.peakNits) || !(encode16.peakNits > 0.0f && encode16.peakNits <= 10000.0f)) {
                std::cerr << "kajo_render: --peak-nits: encode peak luminance must be finite and in (0, 10000] nits" << std::endl;
                return 1;
            }
        }
        if (dither) {
            encode8.flags = KAJO_ENCODE_DITHER;
            if (!ditherSeed.empty()) {
                char* end = nullptr;
                const unsigned long long seed = std::strtoull(ditherSeed.c_str(), &end, 10);
                if (end == ditherSeed.c_str() || *end != '\0' || ditherSeed[0] == '-' || seed > 0xffffffffull) {
                    std::cerr << "kajo_render: --dither-seed N must be in 0..4294967295" << std::endl;
                    return 1;
                }
                encode8.ditherSeed = (uint32_t)seed;
            }
        }
    }
    const char* viewFilterNames[] = {"nearest", "area", "triangle", "lanczos3"};
    if (viewGiven) {
        // (before any device is opened: the refusals of the view, with the option's name)
        if (threeArg) {
            std::cerr << "kajo_render: the view options need the options constructor (without --three-arg)" << std::endl;
            return 1;
        }
        if (!supersample.empty() && !outputSize.empty()) {
            std::cerr << "kajo_render: --supersample and --output-size are two output sizes: give one" << std::endl;
            return 1;
        }
        opt.viewOn = true;
        kajo_hip_default_view_params(&opt.view);
        opt.view.outW = width;
        opt.view.outH = height;
        if (!supersample.empty()) {
            char* end = nullptr;
            const long k = std::strtol(supersample.c_str(), &end, 10);
            if (end == supersample.c_str() || *end != '\0' || k < 2 || k > 8) {
                std::cerr << "kajo_render: --supersample K must be in 2..8" << std::endl;
                return 1;
            }
            if (!viewFilter.empty() && viewFilter != "area") {
                std::cerr << "kajo_render: --supersample averages with the area filter: --view-filter must be area with it" << std::endl;
                return 1;
            }
            // (the frame, and everything written at the rendered size, is K times the size asked for; the aspect is unchanged)
            width *= (int)k;
            height *= (int)k;
        }
        if (!outputSize.empty()) {
            int w = 0, h = 0;
            char tail = 0;
            if (std::sscanf(outputSize.c_str(), "%dx%d%c", &w, &h, &tail) != 2 || w < 1 || h < 1 || w > KAJO_VIEW_MAX_OUT || h > KAJO_VIEW_MAX_OUT) {
                std::cerr << "kajo_render: --output-size WxH: view output size must be in [1, 16384]" << std::endl;
                return 1;
            }
            opt.view.outW = w;
            opt.view.outH = h;
        }
        if (!viewRect.empty()) {
            float r[4];
            char tail = 0;
            if (std::sscanf(viewRect.c_str(), "%f,%f,%f,%f%c", &r[0], &r[1], &r[2], &r[3], &tail) != 4 || !std::isfinite(r[0]) || !std::isfinite(r[1]) ||
                !std::isfinite(r[2]) || !std::isfinite(r[3]) || !(0.0f <= r[0] && r[0] < r[2] && r[2] <= (float)width) ||
                !(0.0f <= r[1] && r[1] < r[3] && r[3] <= (float)height)) {
                std::cerr << "kajo_render: --view X0,Y0,X1,Y1: view rectangle must satisfy 0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height" << std::endl;
                return 1;
            }
            opt.view.x0 = r[0], opt.view.y0 = r[1], opt.view.x1 = r[2], opt.view.y1 = r[3];
        }
        if (!viewFilter.empty()) {
            uint32_t f = 0;
            while (f < 4 && viewFilter != viewFilterNames[f])
                f++;
            if (f == 4) {
                std::cerr << "kajo_render: --view-filter must be nearest, area, triangle or lanczos3" << std::endl;
                return 1;
            }
            opt.view.filter = f;
        }
        const double sx = (viewRect.empty() ? (double)width : (double)opt.view.x1 - opt.view.x0) / opt.view.outW;
        const double sy = (viewRect.empty() ? (double)height : (double)opt.view.y1 - opt.view.y0) / opt.view.outH;
        if (sx > KAJO_VIEW_MAX_SCALE || sy > KAJO_VIEW_MAX_SCALE) {
            std::cerr << "kajo_render: view minification must be at most 64" << std::endl;
            return 1;
        }
    }
    if (lensAperture.empty() && (!lensFocus.empty() || !lensFocusAt.empty() || !lensMaxRadius.empty())) {
        std::cerr << "kajo_render: --lens-focus, --lens-focus-at and --lens-max-radius shape the stage that --lens-aperture turns on: give them with --lens-aperture" << std::endl;
        return 1;
    }
    const bool lensGiven = !lensAperture.empty();
    if (lensGiven) {
        // (before any device is opened: the refusals of kajo_hip_lens, with the option's name)
        if (!lensFocus.empty() && !lensFocusAt.empty()) {
            std::cerr << "kajo_render: --lens-focus and --lens-focus-at are two ways to focus: give one" << std::endl;
            return 1;
        }
        // (the stage reads the AOV buffers of the one handle: the same condition as --denoise)
        if ((opt.gpus != 1 && !aovTiled) || threeArg) {
            std::cerr << "kajo_render: --lens-aperture needs the whole frame on one GPU (--gpus 1, without --three-arg)" << std::endl;
            return 1;
        }
        opt.lensOn = true;
        kajo_hip_default_lens_params(&opt.lens);
        if (!parseFloat(lensAperture, &opt.lens.aperture) || opt.lens.aperture < 0.0f || opt.lens.aperture > 1.0f) {
            std::cerr << "kajo_render: --lens-aperture: lens aperture must be finite and in [0, 1]" << std::endl;
            return 1;
        }
        if (!lensFocus.empty() && (!parseFloat(lensFocus, &opt.lens.focusDistance) || opt.lens.focusDistance <= 0.0f)) {
            std::cerr << "kajo_render: --lens-focus: lens focus distance must be finite and positive" << std::endl;
            return 1;
        }
        if (!lensMaxRadius.empty()) {
            char* end = nullptr;
            const long n = std::strtol(lensMaxRadius.c_str(), &end, 10);
            if (end == lensMaxRadius.c_str() || *end != '\0' || n < 1 || n > KAJO_LENS_MAX_RADIUS) {
                std::cerr << "kajo_render: --lens-max-radius: lens max radius must be in [1, 16]" << std::endl;
                return 1;
            }
            opt.lens.maxRadius = (int32_t)n;
        }
        if (!lensFocusAt.empty()) {
            int fx = -1, fy = -1;
            char tail = 0;
            if (std::sscanf(lensFocusAt.c_str(), "%d,%d%c", &fx, &fy, &tail) != 2 || fx < 0 || fy < 0 || fx >= width || fy >= height) {
                std::cerr << "kajo_render: --lens-focus-at X,Y must be a pixel of the frame" << std::endl;
                return 1;
            }
            opt.lensFocusAt.x = fx;
            opt.lensFocusAt.y = fy;
        } else if (lensFocus.empty()) {
            opt.lensFocusAt.x = width / 2;
            opt.lensFocusAt.y = height / 2;
        }
        opt.aov = true;
    }
    const bool gradeGiven = !gradeSlope.empty() || !gradeOffset.empty() || !gradePower.empty() || !gradeSaturation.empty() || !whiteBalance.empty() ||
                            !whiteBalanceAt.empty() || !gradeRegions.empty();
    double whiteBalanceKelvin = 0, whiteBalanceTint = 0;
    if (gradeGiven) {
        // (before any device is opened: the refusals of kajo_hip_grade and of kajo_hip_grade_white_balance, in the library's own words -- text
        // that is no number becomes a NaN, which they refuse)
        if (threeArg) {
            std::cerr << "kajo_render: the grade options need the backend's options (without --three-arg)" << std::endl;
            return 1;
        }
        if (!whiteBalance.empty() && !whiteBalanceAt.empty()) {
            std::cerr << "kajo_render: --white-balance and --white-balance-at are two white balances: give one" << std::endl;
            return 1;
        }
        if (gradeRegions.size() > KAJO_GRADE_MAX_REGIONS) {
            std::cerr << "kajo_render: --grade-region can be given four times at the most" << std::endl;
            return 1;
        }
        opt.gradeOn = true;
        kajo_hip_default_grade_params(&opt.grade);
        if ((!gradeSlope.empty() && !parseTriple(gradeSlope, false, opt.grade.global.slope)) ||
            (!gradeOffset.empty() && !parseTriple(gradeOffset, false, opt.grade.global.offset)) ||
            (!gradePower.empty() && !parseTriple(gradePower, false, opt.grade.global.power))) {
            std::cerr << "kajo_render: --grade-slope, --grade-offset and --grade-power take three numbers R,G,B" << std::endl;
            return 1;
        }
        if (!gradeSaturation.empty() && !parseFloat(gradeSaturation, &opt.grade.global.saturation))
            opt.grade.global.saturation = NAN;
        for (const std::string& text : gradeRegions) {
            KajoGradeRegion& r = opt.grade.regions[opt.grade.nRegions++];
            if (!parseRegion(text, &r)) {
                std::cerr << "kajo_render: --grade-region IDS:key=v[:key=v...] takes a comma-separated list of at most 16 object ids (whole numbers >= 0), then "
                             "the keys slope, offset, power (one number or R,G,B), saturation and amount"
                          << std::endl;
                return 1;
            }
        }
        if (kajo_hip_grade_pixels(&opt.grade, nullptr, nullptr, 0, nullptr) != KAJO_OK) {
            std::cerr << "kajo_render: the grade options: " << kajo_hip_last_error() << std::endl;
            return 1;
        }
        if (!whiteBalance.empty()) {
            const size_t comma = whiteBalance.find(',');
            float kelvin = NAN, tint = 0.0f;
            if (!parseFloat(whiteBalance.substr(0, comma), &kelvin))
                kelvin = NAN;
            if (comma != std::string::npos && !parseFloat(whiteBalance.substr(comma + 1), &tint))
                tint = NAN;
            float gains[3];
            if (kajo_hip_grade_white_balance(kelvin, tint, gains) != KAJO_OK) {
                std::cerr << "kajo_render: --white-balance KELVIN[,TINT]: " << kajo_hip_last_error() << std::endl;
                return 1;
            }
            whiteBalanceKelvin = kelvin;
            whiteBalanceTint = tint;
            // (into the slope in binary64, rounded once; the product stays inside the slope's range or the library refuses it below)
            for (int c = 0; c < 3; c++)
                opt.grade.global.slope[c] = (float)((double)opt.grade.global.slope[c] * (double)gains[c]);
            if (kajo_hip_grade_pixels(&opt.grade, nullptr, nullptr, 0, nullptr) != KAJO_OK) {
                std::cerr << "kajo_render: the grade options: " << kajo_hip_last_error() << std::endl;
                return 1;
            }
        }
        if (!whiteBalanceAt.empty()) {
            int x = -1, y = -1;
            char tail = 0;
            if (std::sscanf(whiteBalanceAt.c_str(), "%d,%d%c", &x, &y, &tail) != 2 || x < 0 || y < 0 || x >= width || y >= height) {
                std::cerr << "kajo_render: --white-balance-at X,Y must be a pixel of the frame" << std::endl;
                return 1;
            }
            opt.gradeNeutralAt.x = x;
            opt.gradeNeutralAt.y = y;
        }
        if (opt.grade.nRegions > 0) {
            // (the regions read the coverage tables kept beside the AOV buffers of the one handle: the same condition as --matte-mask)
            if (opt.gpus != 1 && !aovTiled) {
                std::cerr << "kajo_render: --grade-region needs the whole frame's mattes: --gpus 1, or any --gpus with --aov-tiled" << std::endl;
                return 1;
            }
            opt.aov = true;
            opt.matte = true;
        }
    }
    const bool gradeRegionsGiven = gradeGiven && opt.grade.nRegions > 0;
    const bool matteGiven = !matteMaskOut.empty() || !matteIdsOut.empty();
    if (aovSpecular && aovPrefix.empty() && denoiseOut.empty() && !matteGiven && !lensGiven && !gradeRegionsGiven) {
        std::cerr << "kajo_render: --aov-specular changes the AOVs that --aov writes and --denoise is guided by: give it with --aov or --denoise" << std::endl;
        return 1;
    }
    opt.aovSpecular = aovSpecular;
    if (aovTiled && aovPrefix.empty() && denoiseOut.empty() && !matteGiven && !lensGiven && !gradeRegionsGiven) {
        std::cerr << "kajo_render: --aov-tiled changes where the AOVs of --aov, --matte-mask, --matte-ids and --denoise are kept: give it with one of them" << std::endl;
        return 1;
    }
    opt.aovTiled = aovTiled;
    if (!aovPrefix.empty()) {
        // (before any device is opened: the AOV buffers are whole-frame buffers of ONE handle, include/kajo_hip.h KAJO_FLAG_AOV, unless every
        // owner keeps its own tiles', --aov-tiled)
        if ((opt.gpus != 1 && !aovTiled) || threeArg) {
            std::cerr << "kajo_render: --aov needs the whole frame on one GPU (--gpus 1, without --three-arg)" << std::endl;
            return 1;
        }
        opt.aov = true;
    }
    if (matteObjectsGiven != !matteMaskOut.empty()) {
        std::cerr << "kajo_render: --matte-mask FILE writes the coverage of the objects --matte-objects LIST names: give the two together" << std::endl;
        return 1;
    }
    if (matteGiven) {
        // (the coverage tables are kept beside the AOV buffers of the one handle: the same condition as --aov, checked before any device is opened)
        if ((opt.gpus != 1 && !aovTiled) || threeArg) {
            std::cerr << "kajo_render: " << (matteMaskOut.empty() ? "--matte-ids" : "--matte-mask")
                      << " needs the whole frame on one GPU (--gpus 1, without --three-arg)" << std::endl;
            return 1;
        }
        if (matteObjectsGiven && !parseObjects(matteObjectsText, &matteObjects)) {
            std::cerr << "kajo_render: --matte-objects must be a comma-separated list of object ids (whole numbers >= 0)" << std::endl;
            return 1;
        }
        opt.aov = true;
        opt.matte = true;
    }
    if (!denoiseOut.empty()) {
        // (the denoiser reads the AOV buffers of the one handle: the same condition as --aov, checked before any device is opened)
        if ((opt.gpus != 1 && !aovTiled) || threeArg) {
            std::cerr << "kajo_render: --denoise needs the whole frame on one GPU (--gpus 1, without --three-arg)" << std::endl;
            return 1;
        }
        if (denoiseIterations < 0 || denoiseIterations > 8) {
            std::cerr << "kajo_render: --denoise-iterations must be in 0..8" << std::endl;
            return 1;
        }
        opt.aov = true;
    }
    if (denoiseNoiseGuided) {
        if (denoiseOut.empty()) {
            std::cerr << "kajo_render: --denoise-noise-guided needs --denoise: it steers that filter" << std::endl;
            return 1;
        }
        opt.denoiseNoiseGuided = true; // (the handles keep the noise estimate, as with --noise-map)
    }

    scene::Scene scene;
    if (!podPath.empty()) {
        // a parsed scene as the tests' fixtures hold it (tests/golden/scenes.npz): the records have scene::Scene's own layout
        std::ifstream f(podPath, std::ios::binary);
        int32_t counts[2] = {0, 0};
        f.read(reinterpret_cast<char*>(counts), sizeof counts);
        if (!f || counts[0] < 0 || counts[1] < 0 || counts[0] > (1 << 20) || counts[1] > (1 << 20)) {
            std::cerr << "Failed to read scene image " << podPath << std::endl;
            return 1;
        }
        static_assert(sizeof(scene::Sphere) == 39 * sizeof(float) && sizeof(scene::Plane) == 38 * sizeof(float), "records are packed floats");
        f.read(reinterpret_cast<char*>(&scene.backgroundColor), 16);
        f.read(reinterpret_cast<char*>(&scene.camera.transform), 64);
        f.read(reinterpret_cast<char*>(&scene.camera.projection), 64);
        scene.spheres.resize(counts[0]);
        scene.planes.resize(counts[1]);
        f.read(reinterpret_cast<char*>(scene.spheres.data()), (std::streamsize)(sizeof(scene::Sphere) * scene.spheres.size()));
        f.read(reinterpret_cast<char*>(scene.planes.data()), (std::streamsize)(sizeof(scene::Plane) * scene.planes.size()));
        if (!f) {
            std::cerr << "Failed to read scene image " << podPath << std::endl;
            return 1;
        }
    } else if (scenePath.empty())
        scene::buildTestScene(scene);
    else if (!scene::Parser::load(scene, scenePath, static_cast<float>(width) / height)) {
        std::cerr << "Failed to parse scene from " << scenePath << std::endl;
        return 1;
    }

    std::unique_ptr<Image> image(new Image(width, height));
    std::unique_ptr<Preview> preview(Preview::create(image.get(), true)); // as renderer/Main.cpp:132
    preview->setPassBudget(opt.passes, verbose);
    preview->closeAtEvent(closeAtEvent);
    std::unique_ptr<Scheduler> scheduler;
    hip::Scheduler* hipScheduler = nullptr;
    opt.counters = json;
    long long matteSamples = 0, matteDroppedPixels = 0; // --json with a matte option
    long long denoiseMeasuredPx = 0;                    // --json with --denoise-noise-guided
    KajoMeterResult metered = {};                       // --json with a meter option: of the image run() wrote
    float localPivotUsed = 0;                           // --json with --local-contrast: of the image run() wrote
    bool localRan = false;
    float lensFocusUsed = 0, lensMaxRadiusPx = 0; // --json with --lens-aperture: of the image -o holds
    bool lensRan = false;
    float gradeSlopeUsed[3] = {1, 1, 1}; // --json with a grade option: of the image -o holds
    bool gradeRan = false;
    std::unique_ptr<Image> viewed; // -o with a view option: the image at the view's size
    try {
        if (rendererName == "hip") {
            // (--three-arg: the statement integration/apply_to_kajo.sh adds to renderer/Main.cpp:135-142, word for word)
            Preview* pv = noPreview ? nullptr : preview.get();
            hipScheduler = threeArg ? new hip::Scheduler(scene, image.get(), pv) : new hip::Scheduler(scene, image.get(), pv, opt);
            scheduler.reset(hipScheduler);
        } else {
            std::cerr << "Unknown renderer: " << rendererName << std::endl;
            return 1;
        }
        scheduler->run();
        if (hipScheduler && meterGiven)
            metered = hipScheduler->lastMeter();
        if (hipScheduler && localGiven)
            localRan = hipScheduler->lastLocalPivot(&localPivotUsed);
        if (lensGiven || gradeGiven) {
            // (the image -o holds: the display chain with the stage in it, from the frame as run() left it; a focus pixel that is far is
            // refused here, after the render)
            hipScheduler->readPresented(nullptr, nullptr, nullptr, nullptr, image->pixels.get(), nullptr, nullptr);
            if (lensGiven)
                lensRan = hipScheduler->lastLens(&lensFocusUsed, &lensMaxRadiusPx);
            if (gradeGiven)
                gradeRan = hipScheduler->lastGrade(gradeSlopeUsed);
            if (meterGiven)
                metered = hipScheduler->lastMeter();
        }
        if (!rawOut.empty()) {
            std::vector<float> acc((size_t)width * height * 4);
            hipScheduler->readRadiance(acc.data());
            std::ofstream f(rawOut, std::ios::binary);
            f.write(reinterpret_cast<const char*>(acc.data()), (std::streamsize)(acc.size() * sizeof(float)));
        }
        if (!hdrOut.empty()) {
            // the estimate itself: sum / P in float32, RGB
            const size_t count = (size_t)width * height;
            std::vector<float> acc(count * 4), rgb(count * 3);
            hipScheduler->readRadiance(acc.data());
            const float passes = (float)hipScheduler->statistics().passes;
            for (size_t i = 0; i < count; i++)
                for (int k = 0; k < 3; k++)
                    rgb[3 * i + k] = acc[4 * i + k] / passes;
            if (!writePfm(hdrOut, width, height, 3, rgb.data()))
                return 3;
        }
        if (!noiseMapOut.empty()) {
            const size_t count = (size_t)width * height;
            std::vector<float> m(count), se(count), rel(count), rgb(count * 3);
            hipScheduler->readNoise(m.data(), se.data(), rel.data());
            for (size_t i = 0; i < count; i++) {
                rgb[3 * i] = m[i];
                rgb[3 * i + 1] = se[i];
                rgb[3 * i + 2] = rel[i];
            }
            if (!writePfm(noiseMapOut, width, height, 3, rgb.data()))
                return 3;
        }
        if (!sampleMapOut.empty()) {
            const size_t count = (size_t)width * height;
            std::vector<uint32_t> passesOf(count);
            std::vector<float> plane(count);
            hipScheduler->readSamplePasses(passesOf.data());
            for (size_t i = 0; i < count; i++)
                plane[i] = (float)passesOf[i];
            if (!writePfm(sampleMapOut, width, height, 1, plane.data()))
                return 3;
        }
        if (!aovPrefix.empty()) {
            // the means: albedo and normal over every sample, depth over the samples that hit (0 where none did)
            const size_t count = (size_t)width * height;
            std::vector<float> a(count * 4), b(count * 4), albedo(count * 3), normal(count * 3), depth(count);
            long long samples = 0;
            hipScheduler->readAov(a.data(), b.data(), &samples);
            const float s = samples > 0 ? (float)samples : 1.0f;
            for (size_t i = 0; i < count; i++) {
                for (int k = 0; k < 3; k++) {
                    albedo[3 * i + k] = a[4 * i + k] / s;
                    normal[3 * i + k] = b[4 * i + k] / s;
                }
                depth[i] = a[4 * i + 3] > 0.0f ? b[4 * i + 3] / a[4 * i + 3] : 0.0f;
            }
            if (!writePfm(aovPrefix + "_albedo.pfm", width, height, 3, albedo.data()) || !writePfm(aovPrefix + "_normal.pfm", width, height, 3, normal.data()) ||
                !writePfm(aovPrefix + "_depth.pfm", width, height, 1, depth.data()))
                return 3;
        }
        if (matteGiven) {
            const size_t count = (size_t)width * height;
            std::vector<float> mask(matteMaskOut.empty() ? 0 : count), dominant(matteIdsOut.empty() ? 0 : count);
            hipScheduler->readMatteMask(matteObjects.data(), (int)matteObjects.size(), matteMaskOut.empty() ? nullptr : mask.data(),
                                        matteIdsOut.empty() ? nullptr : dominant.data());
            if ((!matteMaskOut.empty() && !writePfm(matteMaskOut, width, height, 1, mask.data())) ||
                (!matteIdsOut.empty() && !writePfm(matteIdsOut, width, height, 1, dominant.data())))
                return 3;
            if (json) {
                // the samples a pixel's table could not hold: samples - the sum of its counts
                std::vector<uint32_t> counts(count * KAJO_MATTE_SLOTS);
                hipScheduler->readMatte(nullptr, counts.data(), &matteSamples);
                for (size_t i = 0; i < count; i++) {
                    long long held = 0;
                    for (int k = 0; k < KAJO_MATTE_SLOTS; k++)
                        held += counts[i * KAJO_MATTE_SLOTS + k];
                    matteDroppedPixels += held < matteSamples ? 1 : 0;
                }
            }
        }
        if (!denoiseOut.empty()) {
            KajoDenoiseParams p;
            kajo_hip_default_denoise_params(&p);
            p.iterations = denoiseIterations;
            Image denoised(width, height);
            if (despeckle || meterGiven || localGiven || lensGiven || gradeGiven)
                hipScheduler->readPresented(nullptr, &p, nullptr, nullptr, denoised.pixels.get(), nullptr, nullptr);
            else if (glareGiven)
                hipScheduler->readDisplayed(&p, nullptr, nullptr, denoised.pixels.get(), nullptr);
            else if (toneGiven)
                hipScheduler->readDenoisedTonemapped(&p, nullptr, denoised.pixels.get(), nullptr);
            else
                hipScheduler->readDenoised(&p, nullptr, denoised.pixels.get());
            if (!denoised.save(denoiseOut))
                return 3;
            if (denoiseNoiseGuided && json)
                denoiseMeasuredPx = hipScheduler->denoiseMeasuredPixels();
        }
        if (viewGiven && !out.empty()) {
            // (the image -o holds: the display chain as run() left the frame, through the view, at the view's size)
            viewed.reset(new Image(opt.view.outW, opt.view.outH));
            hipScheduler->readViewed(viewed->pixels.get());
            if (gradeGiven)
                gradeRan = hipScheduler->lastGrade(gradeSlopeUsed);
        }
        if (dither && !out.empty()) {
            // (the image -o holds: the whole chain as run() left the frame, through the encode's ARGB8 words with dither)
            hipScheduler->readEncoded(&encode8, image->pixels.get());
            if (gradeGiven)
                gradeRan = hipScheduler->lastGrade(gradeSlopeUsed);
        }
        if (!png16Out.empty()) {
            std::vector<uint16_t> words((size_t)width * height * 4);
            hipScheduler->readEncoded(&encode16, words.data());
            if (!writePng16(png16Out, width, height, words.data(), encode16.transfer == KAJO_TRANSFER_PQ))
                return 3;
        }
    } catch (const std::exception& e) {
        std::cerr << "kajo_render: " << e.what() << std::endl;
        return 2;
    }
    if (!out.empty() && !(viewed ? viewed->save(out) : image->save(out)))
        return 3;
    if (json) {
        const hip::Statistics& s = hipScheduler->statistics();
        std::printf("{\"width\": %d, \"height\": %d, \"passes\": %d, \"gpus\": %d, \"paths\": %llu, \"traversals\": %llu, "
                    "\"vertices\": %llu, \"wall_s\": %.6f, \"kernel_ms\": %.3f, \"msamples_per_s\": %.2f, \"batch_ms\": [",
                    width, height, s.passes, s.gpus, s.paths, s.traversals, s.vertices, s.wallSeconds, s.kernelMs,
                    s.paths / s.wallSeconds / 1e6);
        for (size_t i = 0; i < s.batchMs.size(); i++)
            std::printf("%s%.4f", i ? ", " : "", s.batchMs[i]);
        std::printf("], \"batch_passes\": [");
        for (size_t i = 0; i < s.batchPasses.size(); i++)
            std::printf("%s%d", i ? ", " : "", s.batchPasses[i]);
        // what the preview saw (renderer/Preview.cpp:79-98,216-234): every update() in call order, whether each came on the thread that
        // owns the window, and how often it was asked for events
        std::printf("], \"preview_updates\": [");
        bool onOwner = true;
        for (size_t i = 0; i < preview->updates().size(); i++) {
            std::printf("%s%d", i ? ", " : "", preview->updates()[i].pass);
            onOwner = onOwner && preview->updates()[i].onCreatingThread;
        }
        std::printf("], \"preview_updates_on_owning_thread\": %s, \"preview_event_calls\": %d", onOwner ? "true" : "false", preview->eventCalls());
        if (toneGiven)
            std::printf(", \"tone_scale\": %.9g", (double)s.toneScale);
        if (despeckle)
            std::printf(", \"despeckle_clamped\": %lld, \"despeckle_repaired\": %lld", s.clamped, s.repaired);
        if (meterGiven) {
            // (of the image -o holds: run()'s last refresh -- taken before --denoise metered its own frame)
            std::printf(", \"meter_exposure\": %.9g, \"meter_white\": %.9g, \"meter_anchor\": %.9g, \"meter_metered\": %lld, \"meter_under\": %lld, "
                        "\"meter_over\": %lld, \"meter_stops\": %.9g",
                        (double)metered.exposure, (double)metered.whiteL, (double)metered.anchorL, (long long)metered.metered, (long long)metered.under,
                        (long long)metered.over, metered.metered > 0 ? (metered.maxBin - metered.minBin + 1) / 16.0 : 0.0);
        }
        if (localGiven) {
            // (local_pivot: of the image -o holds; null where the parameters make the stage a copy and it did not run)
            std::printf(", \"local_compression\": %.9g, \"local_detail\": %.9g, \"local_range\": %.9g, \"local_iterations\": %d, "
                        "\"local_pivot_metered\": %s, \"local_pivot_percentile\": %.9g, \"local_pivot\": ",
                        (double)opt.local.compression, (double)opt.local.detail, (double)opt.local.sigmaRange, (int)opt.local.iterations,
                        (opt.local.flags & KAJO_LOCAL_PIVOT_METERED) ? "true" : "false", (double)opt.local.pivotPercentile);
            if (localRan)
                std::printf("%.9g", (double)localPivotUsed);
            else
                std::printf("null");
        }
        if (lensGiven && lensRan)
            std::printf(", \"lens_focus\": %.9g, \"lens_max_radius_px\": %.9g", (double)lensFocusUsed, (double)lensMaxRadiusPx);
        if (gradeGiven && gradeRan) {
            // (grade_slope: the slope the image -o holds was graded with, the white balance in it)
            const KajoGradeOp& g = opt.grade.global;
            std::printf(", \"grade_slope\": [%.9g, %.9g, %.9g], \"grade_offset\": [%.9g, %.9g, %.9g], \"grade_power\": [%.9g, %.9g, %.9g], "
                        "\"grade_saturation\": %.9g, \"grade_regions\": %d",
                        (double)gradeSlopeUsed[0], (double)gradeSlopeUsed[1], (double)gradeSlopeUsed[2], (double)g.offset[0], (double)g.offset[1],
                        (double)g.offset[2], (double)g.power[0], (double)g.power[1], (double)g.power[2], (double)g.saturation, (int)opt.grade.nRegions);
            if (!whiteBalance.empty())
                std::printf(", \"grade_white_balance_kelvin\": %.9g, \"grade_white_balance_tint\": %.9g", whiteBalanceKelvin, whiteBalanceTint);
        }
        if (viewGiven)
            std::printf(", \"view_out_w\": %d, \"view_out_h\": %d, \"view_filter\": \"%s\", \"view_scale_x\": %.9g, \"view_scale_y\": %.9g",
                        (int)opt.view.outW, (int)opt.view.outH, viewFilterNames[opt.view.filter],
                        (viewRect.empty() ? (double)width : (double)opt.view.x1 - opt.view.x0) / opt.view.outW,
                        (viewRect.empty() ? (double)height : (double)opt.view.y1 - opt.view.y0) / opt.view.outH);
        if (encodeGiven) {
            // (of --png16 where it is given, else of -o through --dither)
            const KajoEncodeParams& e = png16Out.empty() ? encode8 : encode16;
            std::printf(", \"encode_format\": \"%s\", \"encode_transfer\": \"%s\", \"encode_peak_nits\": ", png16Out.empty() ? "argb8" : "rgba16",
                        transferNames[e.transfer]);
            if (e.transfer == KAJO_TRANSFER_PQ)
                std::printf("%.9g", (double)e.peakNits);
            else
                std::printf("null");
            std::printf(", \"encode_dither\": %s", dither ? "true" : "false");
        }
        if (adaptiveGiven)
            std::printf(", \"adaptive_active_units\": %lld, \"adaptive_units\": %lld, \"adaptive_paths\": %lld, \"adaptive_stopped_at_pass\": %d",
                        s.adaptiveActiveUnits, s.adaptiveUnits, s.adaptivePaths, s.adaptiveStoppedAtPass);
        if (noiseGiven || adaptiveGiven)
            std::printf(", \"noise_quantile_value\": %.9g, \"noise_known_px\": %lld, \"noise_bad_px\": %lld, \"noise_stopped_at_pass\": %d",
                        (double)s.noiseQuantileValue, s.noiseKnownPx, s.noiseBadPx, s.noiseStoppedAtPass);
        if (aovTiled)
            std::printf(", \"aov_tiled\": true");
        if (denoiseNoiseGuided)
            std::printf(", \"denoise_noise_guided\": true, \"denoise_measured_px\": %lld", denoiseMeasuredPx);
        if (matteGiven)
            std::printf(", \"matte_samples\": %lld, \"matte_dropped_pixels\": %lld", matteSamples, matteDroppedPixels);
        std::printf("}\n");
    }
    return 0;
}
