// Main.cpp -- headless driver with the reference's command line (renderer/Main.cpp:97-146):
//   kajo_render [-w SIZE] [-h SIZE] [-r hip] [options] SCENE.json     (no SCENE: the built-in test scene)
// in three stages: the command line into Arguments (Arguments.cpp), the render, the files and the JSON line.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "Arguments.h"
#include "HipScheduler.h"
#include "Image.h"
#include "kajo_hip.h"
#include "Preview.h"
#include "scene/Scene.h"

namespace
{

// what the run measured, for the JSON line: each of the image the file named holds
struct RunFacts
{
    KajoMeterResult metered = {};                       // a meter option: of the image run() wrote
    float localPivotUsed = 0;                           // --local-contrast: of the image run() wrote
    bool localRan = false;
    float lensFocusUsed = 0, lensMaxRadiusPx = 0;       // --lens-aperture: of the image -o holds
    bool lensRan = false;
    float gradeSlopeUsed[3] = {1, 1, 1};                // a grade option: of the image -o holds
    bool gradeRan = false;
    long long matteSamples = 0, matteDroppedPixels = 0; // a matte option
    long long denoiseMeasuredPx = 0;                    // --denoise-noise-guided
};

int loadScene(const Arguments& a, scene::Scene& scene)
{
    if (!a.podPath.empty()) {
        // a parsed scene as the tests' fixtures hold it (tests/golden/scenes.npz): the records have scene::Scene's own layout
        std::ifstream f(a.podPath, std::ios::binary);
        int32_t counts[2] = {0, 0};
        f.read(reinterpret_cast<char*>(counts), sizeof counts);
        static_assert(sizeof(scene::Sphere) == 39 * sizeof(float) && sizeof(scene::Plane) == 38 * sizeof(float), "records are packed floats");
        if (f && counts[0] >= 0 && counts[1] >= 0 && counts[0] <= (1 << 20) && counts[1] <= (1 << 20)) {
            f.read(reinterpret_cast<char*>(&scene.backgroundColor), 16);
            f.read(reinterpret_cast<char*>(&scene.camera.transform), 64);
            f.read(reinterpret_cast<char*>(&scene.camera.projection), 64);
            scene.spheres.resize(counts[0]);
            scene.planes.resize(counts[1]);
            f.read(reinterpret_cast<char*>(scene.spheres.data()), (std::streamsize)(sizeof(scene::Sphere) * scene.spheres.size()));
            f.read(reinterpret_cast<char*>(scene.planes.data()), (std::streamsize)(sizeof(scene::Plane) * scene.planes.size()));
            if (f)
                return 0;
        }
        std::cerr << "Failed to read scene image " << a.podPath << std::endl;
        return 1;
    }
    if (a.scenePath.empty())
        scene::buildTestScene(scene);
    else if (!scene::Parser::load(scene, a.scenePath, static_cast<float>(a.width) / a.height)) {
        std::cerr << "Failed to parse scene from " << a.scenePath << std::endl;
        return 1;
    }
    return 0;
}

// run(), and what it and the image -o holds measured
void render(hip::Scheduler& s, const Arguments& a, Image& image, RunFacts& facts)
{
    s.run();
    if (a.meterGiven)
        facts.metered = s.lastMeter();
    if (a.localGiven)
        facts.localRan = s.lastLocalPivot(&facts.localPivotUsed);
    if (a.lensGiven || a.gradeGiven) {
        // (the image -o holds: the display chain with the stage in it, from the frame as run() left it; a focus pixel that is far is
        // refused here, after the render)
        s.readPresented(nullptr, nullptr, nullptr, nullptr, image.pixels.get(), nullptr, nullptr);
        if (a.lensGiven)
            facts.lensRan = s.lastLens(&facts.lensFocusUsed, &facts.lensMaxRadiusPx);
        if (a.gradeGiven)
            facts.gradeRan = s.lastGrade(facts.gradeSlopeUsed);
        if (a.meterGiven)
            facts.metered = s.lastMeter();
    }
}

// The writers: each true where its file was not asked for, or was written.

bool writeRaw(hip::Scheduler& s, const Arguments& a)
{
    if (a.rawOut.empty())
        return true;
    std::vector<float> acc((size_t)a.width * a.height * 4);
    s.readRadiance(acc.data());
    std::ofstream f(a.rawOut, std::ios::binary);
    f.write(reinterpret_cast<const char*>(acc.data()), (std::streamsize)(acc.size() * sizeof(float)));
    return true;
}

// the estimate itself: sum / P in float32, RGB
bool writeHdr(hip::Scheduler& s, const Arguments& a)
{
    if (a.hdrOut.empty())
        return true;
    const size_t count = (size_t)a.width * a.height;
    std::vector<float> acc(count * 4), rgb(count * 3);
    s.readRadiance(acc.data());
    const float passes = (float)s.statistics().passes;
    for (size_t i = 0; i < count; i++)
        for (int k = 0; k < 3; k++)
            rgb[3 * i + k] = acc[4 * i + k] / passes;
    return writePfm(a.hdrOut, a.width, a.height, 3, rgb.data());
}

bool writeNoiseMap(hip::Scheduler& s, const Arguments& a)
{
    if (a.noiseMapOut.empty())
        return true;
    const size_t count = (size_t)a.width * a.height;
    std::vector<float> m(count), se(count), rel(count), rgb(count * 3);
    s.readNoise(m.data(), se.data(), rel.data());
    for (size_t i = 0; i < count; i++) {
        rgb[3 * i] = m[i];
        rgb[3 * i + 1] = se[i];
        rgb[3 * i + 2] = rel[i];
    }
    return writePfm(a.noiseMapOut, a.width, a.height, 3, rgb.data());
}

bool writeSampleMap(hip::Scheduler& s, const Arguments& a)
{
    if (a.sampleMapOut.empty())
        return true;
    const size_t count = (size_t)a.width * a.height;
    std::vector<uint32_t> passesOf(count);
    std::vector<float> plane(count);
    s.readSamplePasses(passesOf.data());
    for (size_t i = 0; i < count; i++)
        plane[i] = (float)passesOf[i];
    return writePfm(a.sampleMapOut, a.width, a.height, 1, plane.data());
}

// the means: albedo and normal over every sample, depth over the samples that hit (0 where none did)
bool writeAovs(hip::Scheduler& s, const Arguments& a)
{
    if (a.aovPrefix.empty())
        return true;
    const size_t count = (size_t)a.width * a.height;
    std::vector<float> sumA(count * 4), sumB(count * 4), albedo(count * 3), normal(count * 3), depth(count);
    long long samples = 0;
    s.readAov(sumA.data(), sumB.data(), &samples);
    const float n = samples > 0 ? (float)samples : 1.0f;
    for (size_t i = 0; i < count; i++) {
        for (int k = 0; k < 3; k++) {
            albedo[3 * i + k] = sumA[4 * i + k] / n;
            normal[3 * i + k] = sumB[4 * i + k] / n;
        }
        depth[i] = sumA[4 * i + 3] > 0.0f ? sumB[4 * i + 3] / sumA[4 * i + 3] : 0.0f;
    }
    return writePfm(a.aovPrefix + "_albedo.pfm", a.width, a.height, 3, albedo.data()) &&
           writePfm(a.aovPrefix + "_normal.pfm", a.width, a.height, 3, normal.data()) && writePfm(a.aovPrefix + "_depth.pfm", a.width, a.height, 1, depth.data());
}

bool writeMattes(hip::Scheduler& s, const Arguments& a, RunFacts& facts)
{
    if (!a.matteGiven)
        return true;
    const size_t count = (size_t)a.width * a.height;
    std::vector<float> mask(a.matteMaskOut.empty() ? 0 : count), dominant(a.matteIdsOut.empty() ? 0 : count);
    s.readMatteMask(a.matteObjects.data(), (int)a.matteObjects.size(), a.matteMaskOut.empty() ? nullptr : mask.data(),
                    a.matteIdsOut.empty() ? nullptr : dominant.data());
    if ((!a.matteMaskOut.empty() && !writePfm(a.matteMaskOut, a.width, a.height, 1, mask.data())) ||
        (!a.matteIdsOut.empty() && !writePfm(a.matteIdsOut, a.width, a.height, 1, dominant.data())))
        return false;
    if (a.json) {
        // the samples a pixel's table could not hold: samples - the sum of its counts
        std::vector<uint32_t> counts(count * KAJO_MATTE_SLOTS);
        s.readMatte(nullptr, counts.data(), &facts.matteSamples);
        for (size_t i = 0; i < count; i++) {
            long long held = 0;
            for (int k = 0; k < KAJO_MATTE_SLOTS; k++)
                held += counts[i * KAJO_MATTE_SLOTS + k];
            facts.matteDroppedPixels += held < facts.matteSamples ? 1 : 0;
        }
    }
    return true;
}

// the denoised frame through the stages given: the shortest reader that holds them all
bool writeDenoised(hip::Scheduler& s, const Arguments& a, RunFacts& facts)
{
    if (a.denoiseOut.empty())
        return true;
    KajoDenoiseParams p;
    kajo_hip_default_denoise_params(&p);
    p.iterations = a.denoiseIterations;
    Image denoised(a.width, a.height);
    if (a.opt.despeckleOn || a.meterGiven || a.localGiven || a.lensGiven || a.gradeGiven)
        s.readPresented(nullptr, &p, nullptr, nullptr, denoised.pixels.get(), nullptr, nullptr);
    else if (a.glareGiven)
        s.readDisplayed(&p, nullptr, nullptr, denoised.pixels.get(), nullptr);
    else if (a.toneGiven)
        s.readDenoisedTonemapped(&p, nullptr, denoised.pixels.get(), nullptr);
    else
        s.readDenoised(&p, nullptr, denoised.pixels.get());
    if (!denoised.save(a.denoiseOut))
        return false;
    if (a.opt.denoiseNoiseGuided && a.json)
        facts.denoiseMeasuredPx = s.denoiseMeasuredPixels();
    return true;
}

// -o with a view option: the display chain as run() left the frame, through the view, at the view's size
void readViewedImage(hip::Scheduler& s, const Arguments& a, std::unique_ptr<Image>& viewed, RunFacts& facts)
{
    if (!a.viewGiven || a.out.empty())
        return;
    viewed.reset(new Image(a.opt.view.outW, a.opt.view.outH));
    if (a.dither && a.encodeView)
        return; // (readDitheredImage fills it, through the float view)
    s.readViewed(viewed->pixels.get());
    if (a.gradeGiven)
        facts.gradeRan = s.lastGrade(facts.gradeSlopeUsed);
}

// -o with --dither: the whole chain as run() left the frame, through the encode's ARGB8 words with dither
void readDitheredImage(hip::Scheduler& s, const Arguments& a, Image& image, RunFacts& facts)
{
    if (!a.dither || a.out.empty())
        return;
    if (a.encodeView)
        s.readEncodedViewed(&a.encode8, image.pixels.get());
    else
        s.readEncoded(&a.encode8, image.pixels.get());
    if (a.gradeGiven)
        facts.gradeRan = s.lastGrade(facts.gradeSlopeUsed);
}

bool writeEncoded16(hip::Scheduler& s, const Arguments& a)
{
    if (a.png16Out.empty())
        return true;
    // (--encode-view: at the view's output size, through the float view)
    const int w = a.encodeView ? a.opt.view.outW : a.width, h = a.encodeView ? a.opt.view.outH : a.height;
    std::vector<uint16_t> words((size_t)w * h * 4);
    if (a.encodeView)
        s.readEncodedViewed(&a.encode16, words.data());
    else
        s.readEncoded(&a.encode16, words.data());
    return writePng16(a.png16Out, w, h, words.data(), a.encode16.transfer == KAJO_TRANSFER_PQ);
}

void printJson(const Arguments& a, const hip::Statistics& s, const Preview& preview, const RunFacts& f)
{
    const hip::Options& opt = a.opt;
    std::printf("{\"width\": %d, \"height\": %d, \"passes\": %d, \"gpus\": %d, \"paths\": %llu, \"traversals\": %llu, "
                "\"vertices\": %llu, \"wall_s\": %.6f, \"kernel_ms\": %.3f, \"msamples_per_s\": %.2f, \"batch_ms\": [",
                a.width, a.height, s.passes, s.gpus, s.paths, s.traversals, s.vertices, s.wallSeconds, s.kernelMs, s.paths / s.wallSeconds / 1e6);
    for (size_t i = 0; i < s.batchMs.size(); i++)
        std::printf("%s%.4f", i ? ", " : "", s.batchMs[i]);
    std::printf("], \"batch_passes\": [");
    for (size_t i = 0; i < s.batchPasses.size(); i++)
        std::printf("%s%d", i ? ", " : "", s.batchPasses[i]);
    // what the preview saw (renderer/Preview.cpp:79-98,216-234): every update() in call order, whether each came on the thread that
    // owns the window, and how often it was asked for events
    std::printf("], \"preview_updates\": [");
    bool onOwner = true;
    for (size_t i = 0; i < preview.updates().size(); i++) {
        std::printf("%s%d", i ? ", " : "", preview.updates()[i].pass);
        onOwner = onOwner && preview.updates()[i].onCreatingThread;
    }
    std::printf("], \"preview_updates_on_owning_thread\": %s, \"preview_event_calls\": %d", onOwner ? "true" : "false", preview.eventCalls());
    if (a.toneGiven)
        std::printf(", \"tone_scale\": %.9g", (double)s.toneScale);
    if (opt.despeckleOn)
        std::printf(", \"despeckle_clamped\": %lld, \"despeckle_repaired\": %lld", s.clamped, s.repaired);
    if (a.meterGiven) {
        // (of the image -o holds: run()'s last refresh -- taken before --denoise metered its own frame)
        const KajoMeterResult& m = f.metered;
        std::printf(", \"meter_exposure\": %.9g, \"meter_white\": %.9g, \"meter_anchor\": %.9g, \"meter_metered\": %lld, \"meter_under\": %lld, "
                    "\"meter_over\": %lld, \"meter_stops\": %.9g",
                    (double)m.exposure, (double)m.whiteL, (double)m.anchorL, (long long)m.metered, (long long)m.under, (long long)m.over,
                    m.metered > 0 ? (m.maxBin - m.minBin + 1) / 16.0 : 0.0);
    }
    if (a.localGiven) {
        // (local_pivot: of the image -o holds; null where the parameters make the stage a copy and it did not run)
        std::printf(", \"local_compression\": %.9g, \"local_detail\": %.9g, \"local_range\": %.9g, \"local_iterations\": %d, "
                    "\"local_pivot_metered\": %s, \"local_pivot_percentile\": %.9g, \"local_pivot\": ",
                    (double)opt.local.compression, (double)opt.local.detail, (double)opt.local.sigmaRange, (int)opt.local.iterations,
                    (opt.local.flags & KAJO_LOCAL_PIVOT_METERED) ? "true" : "false", (double)opt.local.pivotPercentile);
        if (f.localRan)
            std::printf("%.9g", (double)f.localPivotUsed);
        else
            std::printf("null");
    }
    if (a.lensGiven && f.lensRan)
        std::printf(", \"lens_focus\": %.9g, \"lens_max_radius_px\": %.9g", (double)f.lensFocusUsed, (double)f.lensMaxRadiusPx);
    if (a.gradeGiven && f.gradeRan) {
        // (grade_slope: the slope the image -o holds was graded with, the white balance in it)
        const KajoGradeOp& g = opt.grade.global;
        std::printf(", \"grade_slope\": [%.9g, %.9g, %.9g], \"grade_offset\": [%.9g, %.9g, %.9g], \"grade_power\": [%.9g, %.9g, %.9g], "
                    "\"grade_saturation\": %.9g, \"grade_regions\": %d",
                    (double)f.gradeSlopeUsed[0], (double)f.gradeSlopeUsed[1], (double)f.gradeSlopeUsed[2], (double)g.offset[0], (double)g.offset[1],
                    (double)g.offset[2], (double)g.power[0], (double)g.power[1], (double)g.power[2], (double)g.saturation, (int)opt.grade.nRegions);
        if (a.whiteBalanceGiven)
            std::printf(", \"grade_white_balance_kelvin\": %.9g, \"grade_white_balance_tint\": %.9g", a.whiteBalanceKelvin, a.whiteBalanceTint);
    }
    if (a.viewGiven)
        std::printf(", \"view_out_w\": %d, \"view_out_h\": %d, \"view_filter\": \"%s\", \"view_scale_x\": %.9g, \"view_scale_y\": %.9g", (int)opt.view.outW,
                    (int)opt.view.outH, viewFilterNames[opt.view.filter], a.viewScaleX, a.viewScaleY);
    if (a.encodeGiven) {
        // (of --png16 where it is given, else of -o through --dither)
        const KajoEncodeParams& e = a.png16Out.empty() ? a.encode8 : a.encode16;
        std::printf(", \"encode_format\": \"%s\", \"encode_transfer\": \"%s\", \"encode_peak_nits\": ", a.png16Out.empty() ? "argb8" : "rgba16",
                    transferNames[e.transfer]);
        if (e.transfer == KAJO_TRANSFER_PQ)
            std::printf("%.9g", (double)e.peakNits);
        else
            std::printf("null");
        std::printf(", \"encode_dither\": %s", a.dither ? "true" : "false");
        if (a.encodeView)
            std::printf(", \"encode_view_out_w\": %d, \"encode_view_out_h\": %d", (int)opt.view.outW, (int)opt.view.outH);
    }
    if (a.adaptiveGiven)
        std::printf(", \"adaptive_active_units\": %lld, \"adaptive_units\": %lld, \"adaptive_paths\": %lld, \"adaptive_stopped_at_pass\": %d",
                    s.adaptiveActiveUnits, s.adaptiveUnits, s.adaptivePaths, s.adaptiveStoppedAtPass);
    if (a.noiseGiven || a.adaptiveGiven)
        std::printf(", \"noise_quantile_value\": %.9g, \"noise_known_px\": %lld, \"noise_bad_px\": %lld, \"noise_stopped_at_pass\": %d",
                    (double)s.noiseQuantileValue, s.noiseKnownPx, s.noiseBadPx, s.noiseStoppedAtPass);
    if (!opt.checkpointPath.empty() || !opt.resumePath.empty())
    {
        // (the one file name in the line: its quotes, backslashes and control characters escaped)
        std::string name;
        for (unsigned char c : opt.checkpointPath) {
            char u[8];
            if (c == '"' || c == '\\')
                name += '\\', name += (char)c;
            else if (c < 0x20)
                std::snprintf(u, sizeof u, "\\u%04x", c), name += u;
            else
                name += (char)c;
        }
        std::printf(", \"checkpoint_file\": \"%s\", \"checkpoint_passes\": %d, \"resumed_from_passes\": %d, \"frame_digest\": \"%016llx\"",
                    name.c_str(), s.checkpointPasses, s.resumedFromPasses, s.frameDigest);
    }
    if (opt.aovTiled)
        std::printf(", \"aov_tiled\": true");
    if (opt.denoiseNoiseGuided)
        std::printf(", \"denoise_noise_guided\": true, \"denoise_measured_px\": %lld", f.denoiseMeasuredPx);
    if (a.matteGiven)
        std::printf(", \"matte_samples\": %lld, \"matte_dropped_pixels\": %lld", f.matteSamples, f.matteDroppedPixels);
    std::printf("}\n");
}

} // namespace

int main(int argc, char** argv)
{
    Arguments a;
    if (int rc = parseArguments(argc, argv, &a))
        return rc;
    scene::Scene scene;
    if (int rc = loadScene(a, scene))
        return rc;

    std::unique_ptr<Image> image(new Image(a.width, a.height));
    std::unique_ptr<Preview> preview(Preview::create(image.get(), true)); // as renderer/Main.cpp:132
    preview->setPassBudget(a.opt.passes, a.verbose);
    preview->closeAtEvent(a.closeAtEvent);
    std::unique_ptr<hip::Scheduler> scheduler;
    RunFacts facts;
    std::unique_ptr<Image> viewed; // -o with a view option: the image at the view's size
    try {
        if (a.rendererName != "hip") {
            std::cerr << "Unknown renderer: " << a.rendererName << std::endl;
            return 1;
        }
        // (--three-arg: the statement integration/apply_to_kajo.sh adds to renderer/Main.cpp:135-142, word for word)
        Preview* pv = a.noPreview ? nullptr : preview.get();
        scheduler.reset(a.threeArg ? new hip::Scheduler(scene, image.get(), pv) : new hip::Scheduler(scene, image.get(), pv, a.opt));
        hip::Scheduler& s = *scheduler;
        render(s, a, *image, facts);
        // (in this order: lastMeter() above is taken before --denoise meters its own frame, lastGrade() after each image -o may hold)
        if (!writeRaw(s, a) || !writeHdr(s, a) || !writeNoiseMap(s, a) || !writeSampleMap(s, a) || !writeAovs(s, a) || !writeMattes(s, a, facts) ||
            !writeDenoised(s, a, facts))
            return 3;
        readViewedImage(s, a, viewed, facts);
        readDitheredImage(s, a, viewed && a.encodeView ? *viewed : *image, facts); // (--encode-view: -o at the view's size)
        if (!writeEncoded16(s, a))
            return 3;
    } catch (const std::exception& e) {
        std::cerr << "kajo_render: " << e.what() << std::endl;
        return 2;
    }
    if (!a.out.empty() && !(viewed ? viewed->save(a.out) : image->save(a.out)))
        return 3;
    if (a.json)
        printJson(a, scheduler->statistics(), *preview, facts);
    return 0;
}
