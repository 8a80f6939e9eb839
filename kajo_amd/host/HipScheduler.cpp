#include "HipScheduler.h"

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "Image.h"
#include "Preview.h"
#include "kajo_hip.h"
#include "scene/Scene.h"

namespace hip
{

namespace
{

// C ABI error codes become exceptions on this side of the boundary
void check(int rc, const char* what)
{
    if (rc != KAJO_OK)
        throw std::runtime_error(std::string(what) + ": " + kajo_hip_last_error());
}

void checkHip(hipError_t e, const char* what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

void checkNccl(ncclResult_t r, const char* what)
{
    if (r != ncclSuccess)
        throw std::runtime_error(std::string(what) + ": " + ncclGetErrorString(r));
}

// The first float of a 4x4 matrix or 4-vector member of scene::Scene, whatever its C++ type: this repo's stand-in
// (float[16] / four floats) or the reference's glm::mat4 / glm::vec4 -- both are 16 resp. 4 consecutive floats, column
// major. `make -C kajo_amd/host refcheck` compiles this file against the reference's own scene/Scene.h, Image.h and
// Scheduler.h where /root/reference exists.
template <class T, size_t N>
const float* floatsOf(const T& v)
{
    static_assert(sizeof(T) == N * sizeof(float), "matrix / vector member is not a packed float array");
    return reinterpret_cast<const float*>(&v);
}

void copyMaterial(const scene::Material& m, KajoMaterial& k)
{
    static_assert(sizeof(scene::Material) == sizeof(KajoMaterial), "scene::Material and KajoMaterial share one layout");
    std::memcpy(&k, &m, sizeof k);
}

} // namespace

struct Scheduler::Impl
{
    Image* image = nullptr;
    Preview* preview = nullptr;
    Options opt;
    std::vector<kajo_hip_t> handles;
    std::vector<int> devices;
    std::vector<hipStream_t> streams; // one per owner, shared with its handle
    std::vector<ncclComm_t> comms;
    void* gathered = nullptr;         // on device 0: gpus consecutive tile buffers
    void* argbDevice = nullptr;       // on device 0: the resolved image of a gathered frame, before it goes to Image::pixels
    void* encodedDevice = nullptr;    // on device 0: the encoded image of a gathered frame (readEncoded), grown on demand
    size_t encodedBytes = 0;
    size_t tileBytes = 0;
    // Options::aovTiled with a gather: on device 0, gpus consecutive AOV tile buffers and (Options::matte) matte tile buffers
    void* aovGathered = nullptr;
    void* matteGathered = nullptr;
    size_t aovTileBytes = 0, matteTileBytes = 0;
    bool aovComposed = false; // handle 0 holds the whole-frame AOVs of the passes rendered so far
    Statistics stats;
    float toneScale = 1; // Statistics::toneScale of the last image
    KajoMeterResult metered = {}; // lastMeter()

    // Options::tone is the identity (include/kajo_hip.h: s = 1 and the clamp, whatever white and key say): the plain resolve
    bool toneIsIdentity() const { return opt.tone.curve == KAJO_TONE_CLAMP && opt.tone.flags == 0 && opt.tone.exposure == 0.0f; }

    // Options::glare changes the frame (include/kajo_hip.h: with strength 0 or no level the output is the input)
    bool glareOn() const { return opt.glare.strength > 0.0f && opt.glare.levels > 0; }

    // Options::local changes the frame (include/kajo_hip.h: with compression 1 and detail 1 the output is the input)
    bool localActive() const { return opt.localOn && !(opt.local.compression == 1.0f && opt.local.detail == 1.0f); }

    // A stage's parameters where Options has it change the frame, else null: what run()'s refreshes and readEncoded hand the chain calls.
    // (readPresented and readViewed hand the glare &opt.glare whatever its strength, not glareOrNull(): the two look mergeable by the
    // header's "strength 0 makes the output the input", and are left as they are.)
    const KajoDespeckleParams* despeckleOrNull() const { return opt.despeckleOn ? &opt.despeckle : nullptr; }
    const KajoGlareParams* glareOrNull() const { return glareOn() ? &opt.glare : nullptr; }
    const KajoLocalParams* localOrNull() const { return localActive() ? &opt.local : nullptr; }
    const KajoMeterParams* meterOrNull() const { return opt.meterOn ? &opt.meter : nullptr; }
    // Options::noise / noiseTarget: the handles keep the batch moments (KAJO_FLAG_NOISE)
    bool noiseOn() const { return opt.noise || opt.noiseTarget > 0.0f || adaptiveOn() || opt.denoiseNoiseGuided; }
    // Options::denoiseNoiseGuided: the denoise parameters of a read with the flag set (*store); with several owners the whole frame's m and
    // se from all of them, as readNoise fills them, on the first handle
    std::vector<float> guideMean, guideSe;
    const KajoDenoiseParams* guided(const KajoDenoiseParams* in, KajoDenoiseParams* store)
    {
        if (!opt.denoiseNoiseGuided || !in)
            return in;
        *store = *in;
        store->flags |= KAJO_DENOISE_NOISE_GUIDED;
        if (handles.size() > 1 && store->iterations >= 1) {
            const size_t n = (size_t)image->width * image->height;
            guideMean.assign(n, 0.0f);
            guideSe.assign(n, -1.0f);
            const KajoNoiseParams p = noiseParams();
            for (kajo_hip_t h : handles)
                check(kajo_hip_noise(h, &p, guideMean.data(), guideSe.data(), nullptr, nullptr, nullptr, nullptr), "kajo_hip_noise");
            check(kajo_hip_denoise_guide_planes(handles[0], guideMean.data(), guideSe.data()), "kajo_hip_denoise_guide_planes");
        }
        return store;
    }
    // Options::adaptiveTarget: the handles retire converged units (KAJO_FLAG_ADAPTIVE)
    bool adaptiveOn() const { return opt.adaptiveTarget > 0.0f; }
    KajoAdaptState adaptState{}; // the owners' states added, at the last refresh

    void measureAdaptive()
    {
        adaptState = KajoAdaptState{};
        for (kajo_hip_t h : handles) {
            KajoAdaptState s;
            check(kajo_hip_adapt_state(h, &s), "kajo_hip_adapt_state");
            adaptState.units += s.units;
            adaptState.activeUnits += s.activeUnits;
            adaptState.pixels += s.pixels;
            adaptState.activePixels += s.activePixels;
            adaptState.paths += s.paths;
            adaptState.lastDecisionPass = std::max(adaptState.lastDecisionPass, s.lastDecisionPass);
        }
    }
    KajoNoiseParams noiseParams() const { return KajoNoiseParams{opt.noiseFloor, opt.noiseQuantile}; }
    float noiseValue = -1; // Statistics::noise* of the last refresh
    long long noiseKnown = 0, noiseUnknown = 0, noiseBad = 0;
    // the owners' histograms added word by word, evaluated
    void measureNoise()
    {
        const KajoNoiseParams p = noiseParams();
        uint32_t sum[KAJO_NOISE_HIST_WORDS] = {}, own[KAJO_NOISE_HIST_WORDS];
        for (kajo_hip_t h : handles) {
            check(kajo_hip_noise(h, &p, nullptr, nullptr, nullptr, nullptr, own, nullptr), "kajo_hip_noise");
            for (int i = 0; i < KAJO_NOISE_HIST_WORDS; i++)
                sum[i] += own[i];
        }
        noiseKnown = 0;
        for (int i = 0; i < KAJO_METER_BINS; i++)
            noiseKnown += sum[i];
        noiseUnknown = sum[KAJO_METER_BINS];
        noiseBad = sum[KAJO_METER_BINS + 1];
        check(kajo_hip_noise_evaluate(sum, p.quantile, &noiseValue), "kajo_hip_noise_evaluate");
    }
    bool localRan = false; // lastLocalPivot()
    float localPivot = 0;
    void notePivot()
    {
        check(kajo_hip_local_pivot(handles[0], &localPivot), "kajo_hip_local_pivot");
        localRan = true;
    }

    bool lensRan = false; // lastLens()
    float lensFocus = 0, lensMaxRadiusPx = 0;
    std::vector<float> lensRadius;
    bool gradeRan = false; // lastGrade()
    float gradeSlope[3] = {1, 1, 1};
    std::vector<float> gradeFrame;

    ~Impl()
    {
        for (kajo_hip_t h : handles)
            kajo_hip_destroy(h);
        for (ncclComm_t c : comms)
            ncclCommDestroy(c);
        for (size_t i = 0; i < streams.size(); i++) {
            (void)hipSetDevice(devices[i]);
            (void)hipStreamDestroy(streams[i]);
        }
        if (gathered) {
            (void)hipSetDevice(devices.empty() ? 0 : devices[0]);
            (void)hipFree(gathered);
        }
        if (argbDevice)
            (void)hipFree(argbDevice);
        if (encodedDevice)
            (void)hipFree(encodedDevice);
        if (aovGathered)
            (void)hipFree(aovGathered);
        if (matteGathered)
            (void)hipFree(matteGathered);
    }

    void create(const scene::Scene& s)
    {
        // scene::Scene -> flat POD (valid only during this call, like the reference's const&)
        std::vector<KajoSphere> spheres(s.spheres.size());
        std::vector<KajoPlane> planes(s.planes.size());
        for (size_t i = 0; i < s.spheres.size(); i++) {
            std::memcpy(spheres[i].transform, floatsOf<decltype(s.spheres[i].transform), 16>(s.spheres[i].transform), 64);
            copyMaterial(s.spheres[i].material, spheres[i].material);
            spheres[i].radius = s.spheres[i].radius;
        }
        for (size_t i = 0; i < s.planes.size(); i++) {
            std::memcpy(planes[i].transform, floatsOf<decltype(s.planes[i].transform), 16>(s.planes[i].transform), 64);
            copyMaterial(s.planes[i].material, planes[i].material);
        }
        KajoScene pod;
        std::memcpy(pod.backgroundColor, floatsOf<decltype(s.backgroundColor), 4>(s.backgroundColor), 16);
        std::memcpy(pod.camera.transform, floatsOf<decltype(s.camera.transform), 16>(s.camera.transform), 64);
        std::memcpy(pod.camera.projection, floatsOf<decltype(s.camera.projection), 16>(s.camera.projection), 64);
        pod.nSpheres = (int32_t)spheres.size();
        pod.nPlanes = (int32_t)planes.size();
        pod.spheres = spheres.data();
        pod.planes = planes.data();

        if (opt.gpus == 0) {
            // The reference's driver has no flag for it (renderer/Main.cpp:104-120): the backend takes the node as it finds it,
            // as cpu::Scheduler takes every core (renderer/cpu/Scheduler.cpp:17-24). KAJO_HIP_GPUS caps it.
            int visible = 0;
            checkHip(hipGetDeviceCount(&visible), "hipGetDeviceCount");
            opt.gpus = visible;
            if (const char* e = std::getenv("KAJO_HIP_GPUS")) {
                const int want = std::atoi(e);
                if (want < 1 || want > visible)
                    throw std::runtime_error("hip::Scheduler: KAJO_HIP_GPUS must be between 1 and the number of visible GPUs");
                opt.gpus = want;
            }
        }
        if (opt.gpus < 1)
            throw std::runtime_error("hip::Scheduler: no GPU visible (this backend has no CPU path)");
        if (opt.lensOn && !opt.aov)
            throw std::runtime_error("hip::Scheduler: lensOn needs the depth AOV (aov = true)");
        if (opt.lensOn && opt.gpus != 1 && !opt.aovTiled)
            throw std::runtime_error("hip::Scheduler: lensOn with more than one GPU needs aovTiled");
        if (opt.gradeOn && opt.grade.nRegions > 0 && !(opt.aov && opt.matte))
            throw std::runtime_error("hip::Scheduler: grade regions need the coverage mattes (aov = true, matte = true)");
        if (opt.gradeOn && opt.grade.nRegions > 0 && opt.gpus != 1 && !opt.aovTiled)
            throw std::runtime_error("hip::Scheduler: grade regions with more than one GPU need aovTiled");
        if (opt.denoiseNoiseGuided && !opt.aov)
            throw std::runtime_error("hip::Scheduler: denoiseNoiseGuided steers the denoiser, which needs the AOVs (aov = true)");
        if (opt.aov && opt.gpus != 1 && !opt.aovTiled)
            throw std::runtime_error("hip::Scheduler: first-hit AOVs need the whole frame on one GPU (gpus = 1)");
        if (opt.sameDevice && opt.gather != Options::Copy)
            throw std::runtime_error("hip::Scheduler: sameDevice needs gather = Copy (RCCL wants one rank per device)");
        Options::Numerics numerics = opt.strict ? Options::Strict : opt.numerics;
        if (opt.numericsFromEnvironment && std::getenv("KAJO_HIP_FORCE_GATHER"))
            opt.forceGather = true; // (testing: the three-argument form's N > 1 code -- communicator, gather, resolve from the gathered buffers -- on a one-GPU box)
        if (opt.numericsFromEnvironment) {
            if (const char* e = std::getenv("KAJO_HIP_NUMERICS")) {
                const std::string v(e);
                if (v == "exact") numerics = Options::Exact;
                else if (v == "fast") numerics = Options::Fast;
                else if (v == "strict") numerics = Options::Strict;
                else throw std::runtime_error("hip::Scheduler: KAJO_HIP_NUMERICS must be exact, fast or strict");
            }
        }
        for (int g = 0; g < opt.gpus; g++) {
            KajoParams p;
            kajo_hip_default_params(&p);
            p.samplesPerPass = opt.samplesPerPass;
            p.depthLimit = opt.depthLimit;
            p.seed = opt.seed;
            p.flags = (numerics == Options::Strict ? KAJO_FLAG_STRICT : numerics == Options::Exact ? KAJO_FLAG_EXACT : 0u) | (opt.counters ? KAJO_FLAG_COUNTERS : 0u) |
                      (opt.aov ? KAJO_FLAG_AOV | (opt.aovSpecular ? KAJO_FLAG_AOV_SPECULAR : 0u) | (opt.matte ? KAJO_FLAG_AOV_MATTE : 0u) |
                                 (opt.aovTiled ? KAJO_FLAG_AOV_TILED : 0u)
                               : 0u) |
                      (noiseOn() ? KAJO_FLAG_NOISE : 0u) | (adaptiveOn() ? KAJO_FLAG_ADAPTIVE : 0u);
            p.device = opt.sameDevice ? 0 : g;
            p.tileIndex = g;
            p.tileCount = opt.gpus;
            p.passesPerLaunch = opt.passesPerUpdate > 0 ? opt.passesPerUpdate : 16;
            kajo_hip_t h = nullptr;
            check(kajo_hip_create(&pod, image->width, image->height, &p, &h), "kajo_hip_create");
            handles.push_back(h);
            devices.push_back(p.device);
            if (adaptiveOn()) {
                KajoAdaptParams a;
                kajo_hip_default_adapt_params(&a);
                a.target = opt.adaptiveTarget;
                a.floor = opt.noiseFloor;
                a.allowance = opt.adaptiveAllowance;
                if (opt.adaptiveMinPasses > 0)
                    a.minPasses = opt.adaptiveMinPasses;
                if (opt.adaptiveEvery > 0)
                    a.checkEvery = opt.adaptiveEvery;
                check(kajo_hip_set_adaptive(h, &a), "kajo_hip_set_adaptive");
            }
        }
        if (opt.gpus > 1 || opt.forceGather) {
            void* ptr = nullptr;
            check(kajo_hip_tile_buffer(handles[0], &ptr, &tileBytes), "kajo_hip_tile_buffer");
            checkHip(hipSetDevice(devices[0]), "hipSetDevice");
            checkHip(hipMalloc(&gathered, tileBytes * opt.gpus), "hipMalloc(gather buffer)");
            checkHip(hipMalloc(&argbDevice, (size_t)image->width * image->height * 4), "hipMalloc(image)");
            // one stream per owner carries both its render kernels and its share of the gather
            for (int g = 0; g < opt.gpus; g++) {
                checkHip(hipSetDevice(devices[g]), "hipSetDevice");
                hipStream_t st;
                checkHip(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
                streams.push_back(st);
                check(kajo_hip_set_stream(handles[g], st), "kajo_hip_set_stream");
            }
            if (opt.gather == Options::Rccl) {
                comms.resize(opt.gpus);
                checkNccl(ncclCommInitAll(comms.data(), opt.gpus, devices.data()), "ncclCommInitAll");
            }
            if (opt.aov && opt.aovTiled) {
                void *a = nullptr, *m = nullptr;
                check(kajo_hip_aov_tile_buffers(handles[0], &a, &aovTileBytes, &m, &matteTileBytes), "kajo_hip_aov_tile_buffers");
                checkHip(hipSetDevice(devices[0]), "hipSetDevice");
                checkHip(hipMalloc(&aovGathered, aovTileBytes * opt.gpus), "hipMalloc(AOV gather buffer)");
                if (matteTileBytes)
                    checkHip(hipMalloc(&matteGathered, matteTileBytes * opt.gpus), "hipMalloc(matte gather buffer)");
            }
        }
    }

    // the grade's parameters for an image: Options::grade, with the gains of Options::gradeNeutralAt -- from the chain's frame in front of
    // the grade (kajo_hip_grade with the identity returns it) -- multiplied into the global slope in binary64 and rounded once
    void gradeParams(const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, KajoGradeParams* out)
    {
        *out = opt.grade;
        if (opt.gradeNeutralAt.x >= 0) {
            KajoGradeParams identity;
            kajo_hip_default_grade_params(&identity);
            gradeFrame.resize((size_t)image->width * image->height * 4);
            check(kajo_hip_grade(handles[0], despeckle, denoise, &identity, gradeFrame.data()), "kajo_hip_grade");
            const float* px = &gradeFrame[((size_t)opt.gradeNeutralAt.y * image->width + opt.gradeNeutralAt.x) * 4];
            float gains[3];
            if (kajo_hip_grade_neutral(px, gains) != KAJO_OK)
                throw std::runtime_error("hip::Scheduler: the pixel that should be grey (" + std::to_string(opt.gradeNeutralAt.x) + ", " +
                                         std::to_string(opt.gradeNeutralAt.y) + ") has a channel that is not finite and positive: no neutral there");
            for (int c = 0; c < 3; c++)
                out->global.slope[c] = (float)((double)out->global.slope[c] * (double)gains[c]);
        }
        std::memcpy(gradeSlope, out->global.slope, sizeof gradeSlope);
        gradeRan = true;
    }

    // Options::lensFocusAt into the parameters: the depth under that pixel
    void focusLens(KajoLensParams* lens)
    {
        if (opt.lensFocusAt.x < 0)
            return;
        float z = 0;
        check(kajo_hip_lens_depth_at(handles[0], opt.lensFocusAt.x, opt.lensFocusAt.y, &z), "kajo_hip_lens_depth_at");
        if (!std::isfinite(z))
            throw std::runtime_error("hip::Scheduler: the pixel to focus on (" + std::to_string(opt.lensFocusAt.x) + ", " +
                                     std::to_string(opt.lensFocusAt.y) + ") is far (a miss, or no finite depth): nothing to focus on");
        lens->focusDistance = z;
    }

    // Options switches on a stage of the display chain that changes the frame in front of the tone curves
    bool chainOn() const { return localActive() || opt.meterOn || opt.despeckleOn || glareOn(); }

    // The whole display chain on handle 0's own frame (include/kajo_hip.h: every smaller chain call is this one with stages NULL): the
    // stages given, Options' local tone mapping and metering where they are on, tone NULL = Options::tone
    void present(const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade, const KajoLensParams* lens,
                 const KajoGlareParams* glare, const KajoToneParams* tone, const KajoViewParams* view, uint32_t* argb8)
    {
        check(kajo_hip_present_grade_argb8(handles[0], despeckle, denoise, grade, lens, glare, localOrNull(), meterOrNull(), tone ? tone : &opt.tone,
                                           view, argb8, &metered),
              "kajo_hip_present_grade_argb8");
        if (localActive())
            notePivot();
    }

    // lastLens() of an image made with `lens`
    void noteLens(const KajoLensParams& lens)
    {
        lensRadius.resize((size_t)image->width * image->height);
        check(kajo_hip_lens_coc(handles[0], &lens, lensRadius.data(), nullptr), "kajo_hip_lens_coc");
        lensFocus = lens.focusDistance;
        lensMaxRadiusPx = 0;
        for (float r : lensRadius)
            lensMaxRadiusPx = std::max(lensMaxRadiusPx, r);
        lensRan = true;
    }

    // One buffer of the owner-to-GPU-0 exchange: on device 0, `gpus` consecutive parts of `bytes` each, owner g's at g * bytes
    // (type: of the RCCL exchange, four-byte elements; copyName: of the copy, for its error)
    struct GatherBuffer
    {
        void* onDevice0;
        size_t bytes;
        ncclDataType_t type;
        const char* copyName;
    };
    // Every owner's part of each buffer -> GPU 0; sourcesOf(g, src) names owner g's part of each. RCCL: per owner
    // and buffer a send on the owner's communicator and stream and a receive on those of GPU 0, ALL inside one group. Copy: per owner a
    // wait for its stream, then the copies on GPU 0's.
    template <class SourcesOf>
    void gatherToDevice0(const std::vector<GatherBuffer>& buffers, SourcesOf sourcesOf)
    {
        const bool rccl = opt.gather == Options::Rccl;
        if (rccl)
            checkNccl(ncclGroupStart(), "ncclGroupStart");
        for (int g = 0; g < opt.gpus; g++) {
            void* src[2] = {nullptr, nullptr};
            sourcesOf(g, src);
            if (!rccl) {
                check(kajo_hip_wait(handles[g]), "kajo_hip_wait");
                checkHip(hipSetDevice(devices[0]), "hipSetDevice");
            }
            for (size_t i = 0; i < buffers.size(); i++) {
                const GatherBuffer& b = buffers[i];
                char* dst = static_cast<char*>(b.onDevice0) + (size_t)g * b.bytes;
                if (rccl) {
                    checkNccl(ncclSend(src[i], b.bytes / 4, b.type, 0, comms[g], streams[g]), "ncclSend");
                    checkNccl(ncclRecv(dst, b.bytes / 4, b.type, g, comms[0], streams[0]), "ncclRecv");
                } else
                    checkHip(hipMemcpyAsync(dst, src[i], b.bytes, hipMemcpyDefault, streams[0]), b.copyName);
            }
        }
        if (rccl)
            checkNccl(ncclGroupEnd(), "ncclGroupEnd");
    }

    // several owners (or the forced gather): the whole float frame on handle 0, from the last gather
    void composeFrame()
    {
        if (gathered && !composed) {
            check(kajo_hip_compose(handles[0], gathered), "kajo_hip_compose");
            composed = true;
        }
    }

    // Options::aovTiled: the whole-frame AOVs (and the float frame the denoiser filters) on handle 0, for the readers that need them. One
    // exchange of the AOV and the matte buffers by the frame's own mechanism, then the two compose kernels; nothing where they are at hand
    // already.
    void composeAov()
    {
        if (!opt.aov || !opt.aovTiled || aovComposed)
            return;
        if (gathered) {
            std::vector<GatherBuffer> buffers = {{aovGathered, aovTileBytes, ncclFloat, "hipMemcpyAsync(AOV gather)"}};
            if (matteGathered)
                buffers.push_back({matteGathered, matteTileBytes, ncclUint32, "hipMemcpyAsync(matte gather)"});
            gatherToDevice0(buffers, [&](int g, void** src) {
                check(kajo_hip_aov_tile_buffers(handles[g], &src[0], nullptr, &src[1], nullptr), "kajo_hip_aov_tile_buffers");
            });
            composeFrame();
        }
        // (a single owner: from its own tile buffers, aovGathered and matteGathered null)
        check(kajo_hip_compose_aov(handles[0], aovGathered, matteGathered), "kajo_hip_compose_aov");
        aovComposed = true;
    }

    // What a chain call on handle 0's whole frame takes for the denoiser, the grade and the lens: the parameters, or null without the stage
    struct ChainStages
    {
        const KajoDenoiseParams* denoise = nullptr;
        const KajoGradeParams* grade = nullptr;
        const KajoLensParams* lens = nullptr;
        KajoDenoiseParams denoiseStore;
        KajoGradeParams gradeStore;
        KajoLensParams lensStore;
    };

    // Before readPresented's, readViewed's and readEncoded's chain call on the whole frame: the frame composed, the AOVs where a stage reads
    // them, then the parameters. gradeBeforeLens: readPresented forms the grade's (kajo_hip_grade) before it focuses the lens
    // (kajo_hip_lens_depth_at), the other two after; both calls only read the frame, and each reader keeps its order.
    void prepareChain(const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, bool gradeBeforeLens, ChainStages& c)
    {
        composeFrame();
        if (denoise || opt.lensOn || (opt.gradeOn && opt.grade.nRegions > 0))
            composeAov();
        c.denoise = guided(denoise, &c.denoiseStore);
        if (opt.gradeOn && gradeBeforeLens)
            gradeParams(despeckle, c.denoise, &c.gradeStore);
        if (opt.lensOn) {
            c.lensStore = opt.lens;
            focusLens(&c.lensStore);
            c.lens = &c.lensStore;
        }
        if (opt.gradeOn && !gradeBeforeLens)
            gradeParams(despeckle, c.denoise, &c.gradeStore);
        c.grade = opt.gradeOn ? &c.gradeStore : nullptr;
    }

    // One exchange per displayed frame: every owner's tile buffer -> GPU 0; then the image straight
    // from the gathered buffers into Image::pixels (the float frame is composed only when readRadiance() asks for it).
    // The image of a refresh: the chain where Options turns a stage of it on, else the plain resolve or the tone mapping alone. From handle
    // 0's own tile buffer into host words, or from the gathered buffers into device words.
    void resolveInto(bool fromGathered, void* dst)
    {
        uint32_t* words = static_cast<uint32_t*>(dst);
        if (chainOn()) {
            if (!fromGathered)
                return present(despeckleOrNull(), nullptr, nullptr, nullptr, glareOrNull(), nullptr, nullptr, words);
            check(kajo_hip_present_grade_gathered_argb8_device(handles[0], gathered, despeckleOrNull(), nullptr, glareOrNull(), localOrNull(),
                                                               meterOrNull(), &opt.tone, nullptr, dst, &metered),
                  "kajo_hip_present_grade_gathered_argb8_device");
            if (localActive())
                notePivot();
        } else if (toneIsIdentity()) {
            if (fromGathered)
                check(kajo_hip_resolve_gathered_argb8_device(handles[0], gathered, dst), "kajo_hip_resolve_gathered_argb8_device");
            else
                check(kajo_hip_resolve_argb8(handles[0], words), "kajo_hip_resolve_argb8");
        } else if (fromGathered)
            check(kajo_hip_tonemap_gathered_argb8_device(handles[0], gathered, &opt.tone, dst), "kajo_hip_tonemap_gathered_argb8_device");
        else
            check(kajo_hip_tonemap_argb8(handles[0], &opt.tone, nullptr, words, &toneScale), "kajo_hip_tonemap_argb8");
    }

    void gatherAndResolve()
    {
        if (opt.gpus == 1 && !opt.forceGather) {
            // single owner: the library resolves from its own tile buffer
            resolveInto(false, image->pixels.get());
            if (chainOn())
                check(kajo_hip_tone_scale(handles[0], &toneScale), "kajo_hip_tone_scale");
            return;
        }
        // (every owner's tile buffer has the size of the first's, tileBytes: the tile map gives each the same number of slots)
        gatherToDevice0({{gathered, tileBytes, ncclFloat, "hipMemcpyAsync(gather)"}}, [&](int g, void** src) {
            size_t bytes = 0;
            check(kajo_hip_tile_buffer(handles[g], &src[0], &bytes), "kajo_hip_tile_buffer");
        });
        composed = false;
        resolveInto(true, argbDevice);
        checkHip(hipSetDevice(devices[0]), "hipSetDevice");
        checkHip(hipMemcpyAsync(image->pixels.get(), argbDevice, (size_t)image->width * image->height * 4, hipMemcpyDeviceToHost, streams[0]),
                 "hipMemcpyAsync(image)");
        checkHip(hipStreamSynchronize(streams[0]), "hipStreamSynchronize");
        if (chainOn() || !toneIsIdentity())
            check(kajo_hip_tone_scale(handles[0], &toneScale), "kajo_hip_tone_scale"); // (the stream is drained: no wait left)
    }
    bool composed = false;
};

namespace
{
Options optionsOfTheThreeArgumentForm()
{
    Options o; // every visible GPU (gpus = 0), reference constants, EXACT numerics unless KAJO_HIP_NUMERICS says otherwise
    o.numericsFromEnvironment = true;
    return o;
}
} // namespace

Scheduler::Scheduler(const scene::Scene& scene, Image* image, Preview* preview): Scheduler(scene, image, preview, optionsOfTheThreeArgumentForm())
{
}

Scheduler::Scheduler(const scene::Scene& scene, Image* image, Preview* preview, const Options& options): m_impl(new Impl)
{
    m_impl->image = image;
    m_impl->preview = preview;
    m_impl->opt = options;
    m_impl->create(scene);
}

Scheduler::~Scheduler() {}

const Statistics& Scheduler::statistics() const
{
    return m_impl->stats;
}

const KajoMeterResult& Scheduler::lastMeter() const
{
    return m_impl->metered;
}

bool Scheduler::lastLocalPivot(float* pivot) const
{
    if (m_impl->localRan && pivot)
        *pivot = m_impl->localPivot;
    return m_impl->localRan;
}

bool Scheduler::lastGrade(float slope[3]) const
{
    if (m_impl->gradeRan && slope)
        std::memcpy(slope, m_impl->gradeSlope, sizeof m_impl->gradeSlope);
    return m_impl->gradeRan;
}

bool Scheduler::lastLens(float* focusDistance, float* maxRadiusPx) const
{
    if (m_impl->lensRan && focusDistance)
        *focusDistance = m_impl->lensFocus;
    if (m_impl->lensRan && maxRadiusPx)
        *maxRadiusPx = m_impl->lensMaxRadiusPx;
    return m_impl->lensRan;
}

void Scheduler::readRadiance(float* dst)
{
    Impl& d = *m_impl;
    d.composeFrame();
    check(kajo_hip_read_radiance(d.handles[0], dst), "kajo_hip_read_radiance");
}

void Scheduler::readAov(float* albedoHits, float* normalDepth, long long* samples)
{
    Impl& d = *m_impl;
    d.composeAov();
    int64_t n = 0;
    check(kajo_hip_read_aov(d.handles[0], albedoHits, normalDepth, &n), "kajo_hip_read_aov");
    if (samples)
        *samples = (long long)n;
}

void Scheduler::readMatte(int32_t* ids, uint32_t* counts, long long* samples)
{
    Impl& d = *m_impl;
    d.composeAov();
    int64_t n = 0;
    check(kajo_hip_read_matte(d.handles[0], ids, counts, &n), "kajo_hip_read_matte");
    if (samples)
        *samples = (long long)n;
}

void Scheduler::readMatteMask(const int32_t* objects, int n, float* mask, float* dominant)
{
    Impl& d = *m_impl;
    d.composeAov();
    check(kajo_hip_matte_mask(d.handles[0], objects, n, mask, dominant), "kajo_hip_matte_mask");
}

void Scheduler::readDenoised(const KajoDenoiseParams* params, float* radiance, uint32_t* argb8)
{
    Impl& d = *m_impl;
    KajoDenoiseParams p, g;
    kajo_hip_default_denoise_params(&p);
    d.composeAov();
    check(kajo_hip_denoise(d.handles[0], d.guided(params ? params : &p, &g), radiance, argb8), "kajo_hip_denoise");
}

void Scheduler::readDenoisedTonemapped(const KajoDenoiseParams* params, const KajoToneParams* tone, uint32_t* argb8, float* scale)
{
    Impl& d = *m_impl;
    KajoDenoiseParams p, g;
    kajo_hip_default_denoise_params(&p);
    d.composeAov();
    check(kajo_hip_tonemap_argb8(d.handles[0], tone ? tone : &d.opt.tone, d.guided(params ? params : &p, &g), argb8, scale), "kajo_hip_tonemap_argb8");
}

void Scheduler::readDisplayed(const KajoDenoiseParams* denoise, const KajoGlareParams* glare, const KajoToneParams* tone, uint32_t* argb8, float* scale)
{
    Impl& d = *m_impl;
    d.composeFrame();
    KajoDenoiseParams g;
    if (denoise) {
        d.composeAov();
        denoise = d.guided(denoise, &g);
    }
    check(kajo_hip_display_argb8(d.handles[0], denoise, glare ? glare : &d.opt.glare, tone ? tone : &d.opt.tone, argb8, scale), "kajo_hip_display_argb8");
}

void Scheduler::readPresented(const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* glare,
                              const KajoToneParams* tone, uint32_t* argb8, float* scale, long long counts[2])
{
    Impl& d = *m_impl;
    if (!despeckle)
        despeckle = d.despeckleOrNull();
    if (counts)
        counts[0] = counts[1] = 0;
    if (!despeckle && !d.opt.meterOn && !d.localActive() && !d.opt.lensOn && !d.opt.gradeOn)
        return readDisplayed(denoise, glare, tone, argb8, scale);
    Impl::ChainStages c;
    d.prepareChain(despeckle, denoise, true, c);
    d.present(despeckle, c.denoise, c.grade, c.lens, glare ? glare : &d.opt.glare, tone, nullptr, argb8);
    if (scale)
        check(kajo_hip_tone_scale(d.handles[0], scale), "kajo_hip_tone_scale");
    if (c.lens)
        d.noteLens(*c.lens);
    if (despeckle && counts) {
        int64_t c[2] = {0, 0};
        check(kajo_hip_despeckle_counts(d.handles[0], c), "kajo_hip_despeckle_counts");
        counts[0] = c[0];
        counts[1] = c[1];
    }
}

void Scheduler::readViewed(uint32_t* dst)
{
    Impl& d = *m_impl;
    if (!d.opt.viewOn)
        throw std::runtime_error("hip::Scheduler: readViewed needs Options::viewOn");
    Impl::ChainStages c;
    d.prepareChain(d.despeckleOrNull(), nullptr, false, c);
    // (no noteLens here, unlike readPresented and readEncoded: lastLens() has never been of a viewed image)
    d.present(d.despeckleOrNull(), nullptr, c.grade, c.lens, &d.opt.glare, nullptr, &d.opt.view, dst);
}

void Scheduler::readEncoded(const KajoEncodeParams* encode, void* dst)
{
    readEncodedThrough(encode, nullptr, dst);
}

void Scheduler::readEncodedViewed(const KajoEncodeParams* encode, void* dst)
{
    if (!m_impl->opt.viewOn)
        throw std::runtime_error("hip::Scheduler: readEncodedViewed needs Options::viewOn");
    readEncodedThrough(encode, &m_impl->opt.view, dst);
}

// readEncoded (view null: the calls it has always made) and readEncodedViewed
void Scheduler::readEncodedThrough(const KajoEncodeParams* encode, const KajoViewParams* view, void* dst)
{
    Impl& d = *m_impl;
    const KajoDespeckleParams* despeckle = d.despeckleOrNull();
    const KajoLocalParams* local = d.localOrNull();
    const bool wholeFrame = d.opt.lensOn || (d.opt.gradeOn && (d.opt.grade.nRegions > 0 || d.opt.gradeNeutralAt.x >= 0));
    KajoGradeParams grade;
    if (d.gathered && !wholeFrame) {
        // several owners: straight from the gathered tile buffers, as run()'s refreshes
        size_t bytes = 0;
        check(kajo_hip_encode_bytes(encode, view ? view->outW : d.image->width, view ? view->outH : d.image->height, &bytes), "kajo_hip_encode_bytes");
        checkHip(hipSetDevice(d.devices[0]), "hipSetDevice");
        if (d.encodedBytes < bytes) {
            if (d.encodedDevice)
                checkHip(hipFree(d.encodedDevice), "hipFree(encoded image)");
            d.encodedDevice = nullptr;
            d.encodedBytes = 0;
            checkHip(hipMalloc(&d.encodedDevice, bytes), "hipMalloc(encoded image)");
            d.encodedBytes = bytes;
        }
        if (d.opt.gradeOn)
            d.gradeParams(despeckle, nullptr, &grade);
        if (view)
            check(kajo_hip_encode_view_present_gathered_device(d.handles[0], d.gathered, despeckle, d.opt.gradeOn ? &grade : nullptr, d.glareOrNull(),
                                                               local, d.meterOrNull(), &d.opt.tone, view, encode, d.encodedDevice, &d.metered),
                  "kajo_hip_encode_view_present_gathered_device");
        else
            check(kajo_hip_encode_present_gathered_device(d.handles[0], d.gathered, despeckle, d.opt.gradeOn ? &grade : nullptr, d.glareOrNull(), local,
                                                          d.meterOrNull(), &d.opt.tone, encode, d.encodedDevice, &d.metered),
                  "kajo_hip_encode_present_gathered_device");
        if (local)
            d.notePivot();
        checkHip(hipMemcpyAsync(dst, d.encodedDevice, bytes, hipMemcpyDeviceToHost, d.streams[0]), "hipMemcpyAsync(encoded image)");
        checkHip(hipStreamSynchronize(d.streams[0]), "hipStreamSynchronize");
        return;
    }
    Impl::ChainStages c;
    d.prepareChain(despeckle, nullptr, false, c);
    if (view)
        check(kajo_hip_encode_view_present(d.handles[0], despeckle, nullptr, c.grade, c.lens, d.glareOrNull(), local, d.meterOrNull(), &d.opt.tone, view,
                                           encode, dst, &d.metered),
              "kajo_hip_encode_view_present");
    else
        check(kajo_hip_encode_present(d.handles[0], despeckle, nullptr, c.grade, c.lens, d.glareOrNull(), local, d.meterOrNull(), &d.opt.tone, encode, dst,
                                      &d.metered),
              "kajo_hip_encode_present");
    if (local)
        d.notePivot();
    if (c.lens)
        d.noteLens(*c.lens);
}

void Scheduler::readNoise(float* mean, float* stderror, float* relative)
{
    Impl& d = *m_impl;
    if (!d.noiseOn())
        throw std::runtime_error("hip::Scheduler: readNoise needs Options::noise or Options::noiseTarget");
    const KajoNoiseParams p = d.noiseParams();
    for (kajo_hip_t h : d.handles)
        check(kajo_hip_noise(h, &p, mean, stderror, relative, nullptr, nullptr, nullptr), "kajo_hip_noise");
}

long long Scheduler::denoiseMeasuredPixels()
{
    Impl& d = *m_impl;
    if (!d.opt.denoiseNoiseGuided)
        throw std::runtime_error("hip::Scheduler: denoiseMeasuredPixels needs Options::denoiseNoiseGuided");
    const size_t n = (size_t)d.image->width * d.image->height;
    std::vector<float> m(n, 0.0f), se(n, -1.0f);
    readNoise(m.data(), se.data(), nullptr);
    long long measured = 0;
    for (size_t i = 0; i < n; i++)
        measured += se[i] >= 0.0f && m[i] > 0.0f ? 1 : 0;
    return measured;
}

void Scheduler::readSamplePasses(uint32_t* plane)
{
    Impl& d = *m_impl;
    if (!d.adaptiveOn())
        throw std::runtime_error("hip::Scheduler: readSamplePasses needs Options::adaptiveTarget");
    for (kajo_hip_t h : d.handles)
        check(kajo_hip_adapt_passes(h, plane), "kajo_hip_adapt_passes");
}

namespace
{

// The checkpoint file: "KAJOCKPF", a version word, the number of sections, their sizes (64-bit), then the sections as
// kajo_hip_checkpoint_save wrote them, each from a multiple of 16. Little-endian, as the sections are.
const char kFileMagic[8] = {'K', 'A', 'J', 'O', 'C', 'K', 'P', 'F'};

void writeCheckpointFile(const std::string& path, const std::vector<std::vector<unsigned char>>& sections)
{
    const std::string tmp = path + ".tmp";
    {
        std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
        const uint32_t head[2] = {1u, (uint32_t)sections.size()};
        f.write(kFileMagic, 8);
        f.write(reinterpret_cast<const char*>(head), sizeof head);
        uint64_t at = 16 + 8 * (uint64_t)sections.size();
        for (const auto& s : sections) {
            const uint64_t n = s.size();
            f.write(reinterpret_cast<const char*>(&n), 8);
        }
        const char zeros[16] = {};
        for (const auto& s : sections) {
            f.write(zeros, (std::streamsize)((16 - at % 16) % 16));
            at += (16 - at % 16) % 16;
            f.write(reinterpret_cast<const char*>(s.data()), (std::streamsize)s.size());
            at += s.size();
        }
        f.flush();
        if (!f)
            throw std::runtime_error("hip::Scheduler: cannot write the checkpoint " + tmp);
    }
    if (std::rename(tmp.c_str(), path.c_str()) != 0)
        throw std::runtime_error("hip::Scheduler: cannot rename " + tmp + " to " + path);
}

std::vector<std::vector<unsigned char>> readCheckpointFile(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    std::vector<unsigned char> all((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (!f && all.empty())
        throw std::runtime_error("hip::Scheduler: cannot read the checkpoint " + path);
    uint32_t head[2] = {0, 0};
    if (all.size() < 16 || std::memcmp(all.data(), kFileMagic, 8) != 0)
        throw std::runtime_error("hip::Scheduler: " + path + " is not a checkpoint file");
    std::memcpy(head, all.data() + 8, sizeof head);
    if (head[0] != 1u || head[1] < 1 || head[1] > 4096 || all.size() < 16 + 8 * (size_t)head[1])
        throw std::runtime_error("hip::Scheduler: " + path + ": unknown version or truncated table of sections");
    std::vector<std::vector<unsigned char>> sections;
    uint64_t at = 16 + 8 * (uint64_t)head[1];
    for (uint32_t i = 0; i < head[1]; i++) {
        uint64_t n;
        std::memcpy(&n, all.data() + 16 + 8 * (size_t)i, 8);
        at += (16 - at % 16) % 16;
        if (n > all.size() || at > all.size() - n)
            throw std::runtime_error("hip::Scheduler: " + path + ": truncated inside section " + std::to_string(i));
        sections.emplace_back(all.begin() + (std::ptrdiff_t)at, all.begin() + (std::ptrdiff_t)(at + n));
        at += n;
    }
    return sections;
}

} // namespace

void Scheduler::run()
{
    Impl& d = *m_impl;
    const Options& o = d.opt;
    const bool adaptive = d.adaptiveOn();
    const bool stopRule = o.noiseTarget > 0.0f || adaptive; // (either rule: refreshes of whole batches, maxPasses the budget)
    int adaptiveStoppedAt = 0;
    const int budget = stopRule && o.maxPasses > 0 ? o.maxPasses : o.passes > 0 ? o.passes : (d.preview ? 0 : 16);
    int stoppedAt = 0;
    const std::thread::id self = std::this_thread::get_id();
    const auto t0 = std::chrono::steady_clock::now();
    int done = 0, resumedFrom = 0, checkpointed = 0;
    // Options::checkpointPath: every owner's section into one file
    const auto checkpoint = [&]() {
        std::vector<std::vector<unsigned char>> sections;
        for (kajo_hip_t h : d.handles) {
            size_t bytes = 0, written = 0;
            check(kajo_hip_checkpoint_bytes(h, &bytes), "kajo_hip_checkpoint_bytes");
            sections.emplace_back(bytes);
            check(kajo_hip_checkpoint_save(h, sections.back().data(), bytes, &written), "kajo_hip_checkpoint_save");
            sections.back().resize(written);
        }
        writeCheckpointFile(o.checkpointPath, sections);
        checkpointed = done;
    };
    if (!o.resumePath.empty()) {
        // the file's sections as they are where they are the handles' own (same number of owners: restore refuses another layout), else
        // merged into one whole-frame section of which every handle takes its pixels
        std::vector<std::vector<unsigned char>> sections = readCheckpointFile(o.resumePath);
        KajoCheckpointInfo info;
        check(kajo_hip_checkpoint_info(sections[0].data(), sections[0].size(), &info), "kajo_hip_checkpoint_info");
        if (sections.size() != d.handles.size() || info.header.tileCount != (int)d.handles.size()) {
            for (uint32_t i = 0; i < info.header.nPlanes; i++)
                if (info.planes[i].kind == KAJO_CKPT_ADAPT)
                    throw std::runtime_error("hip::Scheduler: " + o.resumePath + " is an adaptive session of " + std::to_string(sections.size()) +
                                             " GPU(s): it resumes with that many only (units are launch blocks)");
            std::vector<const void*> ptrs;
            std::vector<size_t> sizes;
            for (const auto& s : sections) {
                ptrs.push_back(s.data());
                sizes.push_back(s.size());
            }
            size_t bytes = 0;
            check(kajo_hip_checkpoint_merge(ptrs.data(), sizes.data(), (int)ptrs.size(), nullptr, 0, &bytes), "kajo_hip_checkpoint_merge");
            std::vector<unsigned char> merged(bytes);
            check(kajo_hip_checkpoint_merge(ptrs.data(), sizes.data(), (int)ptrs.size(), merged.data(), merged.size(), &bytes), "kajo_hip_checkpoint_merge");
            sections.assign(d.handles.size(), merged);
        } else {
            // (in the order of the tile indices, whatever order the file has them in)
            std::vector<std::vector<unsigned char>> byIndex(sections.size());
            for (auto& s : sections) {
                check(kajo_hip_checkpoint_info(s.data(), s.size(), &info), "kajo_hip_checkpoint_info");
                if (info.header.tileCount != (int)sections.size())
                    throw std::runtime_error("hip::Scheduler: " + o.resumePath + ": a section of " + std::to_string(info.header.tileCount) +
                                             " owners in a file of " + std::to_string(sections.size()) + " sections");
                if (!byIndex[(size_t)info.header.tileIndex].empty())
                    throw std::runtime_error("hip::Scheduler: " + o.resumePath + ": owner " + std::to_string(info.header.tileIndex) + " is there twice");
                byIndex[(size_t)info.header.tileIndex].swap(s);
            }
            sections.swap(byIndex);
        }
        for (size_t g = 0; g < d.handles.size(); g++)
            check(kajo_hip_checkpoint_restore(d.handles[g], sections[g].data(), sections[g].size()), "kajo_hip_checkpoint_restore");
        done = resumedFrom = info.header.passesDone;
        d.aovComposed = false;
        if (done > 0 && budget != 0 && done >= budget)
            d.gatherAndResolve(); // (nothing left to render: the image of the restored frame)
    }
    std::vector<double> batchMs;
    std::vector<int> batchPasses;
    // Passes between two refreshes. Fusing passes into one launch evens out the lanes' trip counts (38 G paths/s at
    // 16 per launch against 30 at one, profiles/HISTORY.md section 6), so headless runs take all that is left and a live preview
    // gets as many as fit a 30 Hz refresh, from the measured time per pass.
    // A launch cannot be interrupted (the reference's workers look at their stop flag once per row, cpu/Renderer.cpp:77-78): the
    // bound on how long run() can overshoot a closed window -- or a caller waits for the first image -- is the length of one
    // launch. With a preview: a 30 Hz refresh. Headless: half a second (the 1000-sphere scene at 4K takes 37 ms per pass: 13
    // passes per launch instead of 16, where round 4 launched 16 regardless -- 0.6 s -- and 32 in the tools: 1.2 s).
    double msPerPass = 0.0;
    int samples = 0; // batches measured so far
    auto autoBatch = [&]() {
        if (o.passesPerUpdate > 0)
            return o.passesPerUpdate;
        if (msPerPass <= 0.0)
            return d.preview ? 1 : 2; // nothing measured yet
        const int fit = (int)((d.preview ? 33.0 : 500.0) / msPerPass);
        if (fit >= 8) {
            // launches of 8 or 16 passes that begin with a group of four (include/kajo_hip.h kajo_hip_render): the FAST / EXACT kernels then
            // render the cheapest blocks of a large frame as one workgroup per group (KajoCounters.tailGroups: +2 % at 1920x1080); a shorter
            // batch first if the passes done so far end inside a group. Scheduling only: the frame does not depend on the batches.
            const int over = done % 4;
            return over ? 4 - over : (fit >= 16 ? 16 : 8);
        }
        return fit < 1 ? 1 : fit;
    };

    // The SDL calls of the preview stay on this (the main) thread, as the reference requires
    // (cpu/Scheduler.cpp:64-81 marshals worker progress through a queue for the same reason).
    while ((!d.preview || d.preview->processEvents()) && (budget == 0 || done < budget) && !stoppedAt && !adaptiveStoppedAt) {
        int batch = autoBatch();
        if (stopRule) // a refresh of the stop rule ends on a batch boundary of the estimate: whole batches, four passes at the least
            batch = done % KAJO_NOISE_BATCH_PASSES ? KAJO_NOISE_BATCH_PASSES - done % KAJO_NOISE_BATCH_PASSES
                                                   : std::max(batch / KAJO_NOISE_BATCH_PASSES, 1) * KAJO_NOISE_BATCH_PASSES;
        const int now = budget == 0 ? batch : (budget - done < batch ? budget - done : batch);
        const auto tb = std::chrono::steady_clock::now();
        for (kajo_hip_t h : d.handles)
            check(kajo_hip_render(h, now), "kajo_hip_render"); // asynchronous, one stream per GPU
        for (kajo_hip_t h : d.handles)
            check(kajo_hip_wait(h), "kajo_hip_wait");
        done += now;
        d.aovComposed = false;
        d.gatherAndResolve();
        if (d.noiseOn()) {
            d.measureNoise();
            if (o.noiseTarget > 0.0f && d.noiseUnknown == 0 && d.noiseKnown > 0 && d.noiseValue <= o.noiseTarget)
                stoppedAt = done;
        }
        if (adaptive) {
            d.measureAdaptive();
            if (d.adaptState.activeUnits == 0)
                adaptiveStoppedAt = done;
        }
        const double batchWall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
        batchMs.push_back(batchWall);
        batchPasses.push_back(now);
        // (the first batch pays for the cold start -- module load, the blocks' cost measurement and its order: it sizes the second batch and
        // is then forgotten)
        const double ms = batchWall / now;
        msPerPass = samples < 2 ? ms : 0.75 * msPerPass + 0.25 * ms;
        samples++;
        if (d.preview)
            for (int p = done - now + 1; p <= done; p++)
                d.preview->update(self, p, o.samplesPerPass, 0, 0, d.image->width, d.image->height);
        if (!o.checkpointPath.empty() && o.checkpointEvery > 0 && done / o.checkpointEvery > (done - now) / o.checkpointEvery)
            checkpoint();
    }
    if (!o.checkpointPath.empty() && checkpointed != done)
        checkpoint();

    d.stats = Statistics();
    d.stats.passes = done;
    d.stats.gpus = o.gpus;
    d.stats.batchMs = batchMs;
    d.stats.batchPasses = batchPasses;
    d.stats.toneScale = d.toneScale;
    if (d.noiseOn() && done > 0) {
        d.stats.noiseQuantileValue = d.noiseValue;
        d.stats.noiseKnownPx = d.noiseKnown;
        d.stats.noiseUnknownPx = d.noiseUnknown;
        d.stats.noiseBadPx = d.noiseBad;
        d.stats.noiseStoppedAtPass = stoppedAt;
    }
    if (adaptive && done > 0) {
        d.stats.adaptiveUnits = d.adaptState.units;
        d.stats.adaptiveActiveUnits = d.adaptState.activeUnits;
        d.stats.adaptivePaths = d.adaptState.paths;
        d.stats.adaptiveStoppedAtPass = adaptiveStoppedAt;
    }
    if (o.despeckleOn && done > 0) {
        int64_t c[2] = {0, 0};
        check(kajo_hip_despeckle_counts(d.handles[0], c), "kajo_hip_despeckle_counts");
        d.stats.clamped = c[0];
        d.stats.repaired = c[1];
    }
    d.stats.checkpointPasses = checkpointed;
    d.stats.resumedFromPasses = resumedFrom;
    if (!o.checkpointPath.empty() || !o.resumePath.empty())
        for (kajo_hip_t h : d.handles) { // (digests add over owners)
            KajoDigest dg;
            check(kajo_hip_digest(h, &dg), "kajo_hip_digest");
            d.stats.frameDigest += dg.plane[KAJO_CKPT_SUM];
        }
    d.stats.wallSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (kajo_hip_t h : d.handles) {
        KajoCounters c;
        check(kajo_hip_counters(h, &c), "kajo_hip_counters");
        d.stats.paths += c.paths;
        d.stats.traversals += c.traversals;
        d.stats.vertices += c.vertices;
        d.stats.laneSlots += c.laneSlots;
        if (c.kernelMs > d.stats.kernelMs)
            d.stats.kernelMs = c.kernelMs;
    }
}

} // namespace hip
