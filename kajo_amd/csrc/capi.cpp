// capi.cpp -- libkajo_hip.so: the C ABI of include/kajo_hip.h over the HIP runtime.
//
// One KajoHip handle = one GPU's share of a frame: the staged scene in device memory, the
// compact tile accumulation buffer, a stream, and (on demand) the composed whole frame and
// its ARGB8 image. There is NO CPU rendering path in this library: without a usable HIP
// device kajo_hip_create fails with KAJO_E_NO_DEVICE.
#include "handle.h"

// launchers of the units only this file drives (noise.hip, adapt_kernels.cpp)
extern "C" {
int kajo_noise_update_launch(const void* tiles, void* baseline, void* records, uint32_t slots, void* stream);
int kajo_noise_map_launch(const void* records, const TileMap* map, int tileIndex, double floorL, void* mean, void* stdError, void* relative,
                          void* batches, void* hist, void* stream);
int kajo_adapt_step_launch(void* tiles, void* baseline, void* records, const void* state, uint32_t slots, uint32_t unitShift, int boundary, int P,
                           void* stream);
int kajo_adapt_select_launch(const void* records, void* state, const AdaptGeom* geom, const AdaptRule* rule, uint32_t units, uint32_t unitThreads,
                             void* stream);
int kajo_adapt_passes_launch(const void* records, const void* state, const TileMap* map, int tileIndex, uint32_t unitShift, uint32_t P, void* plane,
                             void* stream);
}

// kajo_hip_aov_kernel's names in the order of render_args.h KajoAovInstance: the five scene classes, with _spec, with _matte, with both
#define AOV_CLASSES(p) p, p "_big", p "_big_lg", p "_biglist", p "_biglist_lg"
#define AOV_NAMES(p) {AOV_CLASSES(p), AOV_CLASSES(p "_spec"), AOV_CLASSES(p "_matte"), AOV_CLASSES(p "_spec_matte")}
const KernelSet kFastKernels = {kajo_render_fast_launch, kajo_render_fast_split_launch, kajo_render_fast_set_lds, kajo_resolve_fast_launch,
                                kajo_resolve_tiles_fast_launch, kajo_tone_fast_launch, kajo_aov_fast_launch, kajo_aov_fast_set_lds,
                                kajo_kat_trace_fast_launch, kajo_kat_shade_fast_launch, AOV_NAMES("kajo_aov_fast")};
const KernelSet kStrictKernels = {kajo_render_strict_launch, kajo_render_strict_split_launch, kajo_render_strict_set_lds, kajo_resolve_strict_launch,
                                  kajo_resolve_tiles_strict_launch, kajo_tone_strict_launch, kajo_aov_strict_launch, kajo_aov_strict_set_lds,
                                  kajo_kat_trace_strict_launch, kajo_kat_shade_strict_launch, AOV_NAMES("kajo_aov_strict")};
// The oracle's arithmetic in everything that decides (STRICT and EXACT): which walk, which hold policy, whose resolve. EXACT has render
// and shading kernels of its own; the STRICT instances serve it for the rest (EXACT's camera rays, walk and normals are STRICT's arithmetic).
const KernelSet kExactKernels = [] {
    KernelSet k = kStrictKernels;
    k.render = kajo_render_exact_launch;
    k.split = kajo_render_exact_split_launch;
    k.setLds = kajo_render_exact_set_lds;
    k.katShade = kajo_kat_shade_exact_launch;
    return k;
}();

thread_local std::string g_error;

namespace
{

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
    if (h->encodeUploaded)
        (void)hipEventDestroy(h->encodeUploaded);
    if (h->encodeStaging)
        (void)hipHostFree(h->encodeStaging);
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

// the whole-frame AOV sums: float4 [2][W * H]
size_t aovFrameBytes(const KajoHip* h)
{
    return 2 * (size_t)h->W * h->H * 16;
}

// the coverage tables of a handle: ids and counts, a word each per slot
size_t matteTableBytes(const KajoHip* h)
{
    return (size_t)h->W * h->H * KAJO_MATTE_SLOTS * 8;
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

constexpr size_t kCounterBytes = 32 * sizeof(unsigned long long);

// the batch moments of the noise estimate: KajoNoiseMoments [slotsPerOwner]
size_t momentBytes(const KajoHip* h)
{
    return 2 * h->tileBytes;
}

// the state words of an adaptive handle's units, on the device and on the host
size_t adaptStateBytes(const KajoHip* h)
{
    return (size_t)(h->gridBlocks ? h->gridBlocks : 1) * sizeof(uint32_t);
}

// Everything that sums passes, zeroed on the handle's stream: the buffers the handle has, each with its size. sums == false: only what
// is estimated from the sums (the moments and the units' state), which kajo_hip_set_pass_count starts over beside a buffer it keeps.
int clearAccumulators(KajoHip* h, bool sums)
{
    const auto zero = [h](const DeviceBuffer& b, size_t bytes) { return b ? hipMemsetAsync(b.p, 0, bytes, h->stream) : hipSuccess; };
    if (sums) {
        HIP_TRY(zero(h->tiles, h->tileBytes));
        HIP_TRY(zero(h->counters, kCounterBytes));
        HIP_TRY(zero(h->aov, aovFrameBytes(h)));
        HIP_TRY(zero(h->matte, matteTableBytes(h)));
        HIP_TRY(zero(h->aovTiles, aovTileBytes(h)));
        HIP_TRY(zero(h->matteTiles, matteTileBytes(h)));
        HIP_TRY(zero(h->noiseBase, h->tileBytes));
    }
    HIP_TRY(zero(h->noiseMoments, momentBytes(h)));
    HIP_TRY(zero(h->adaptStateDev, adaptStateBytes(h)));
    return KAJO_OK;
}

// f(index of the pixel in the row-major frame, its slot) for every pixel of the frame this owner has
template <class F> void forOwnedPixels(const KajoHip* h, F f)
{
    for (int y = 0; y < h->H; y++)
        for (int x = 0; x < h->W; x++) {
            int owner;
            uint32_t slot;
            kajoTileSlot(h->map, x, y, &owner, &slot);
            if (owner == h->params.tileIndex)
                f((size_t)y * h->W + x, slot);
        }
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

// ---- kajo_hip_create's steps -------------------------------------------------------------------------------------------------------

// The scene staged by the flags, in device memory, and the view of it the kernels read; the LDS plan of the scene
int uploadScene(KajoHip* h, const KajoScene& scene)
{
    const uint32_t flags = h->params.flags;
    kajo::stageScene(scene, h->staged, (flags & KAJO_FLAG_NO_GRID) ? 0 : 48, !(flags & KAJO_FLAG_NO_SHADOW_LISTS));
    const kajo::StagedScene& st = h->staged;
    DSceneView& v = h->view;
    HIP_TRY(upload(st.planeRow, &v.planeRow, h->sceneBuffers));
    HIP_TRY(upload(st.planeDet, &v.planeDet, h->sceneBuffers));
    HIP_TRY(upload(st.planeFrame, &v.planeFrame, h->sceneBuffers));
    HIP_TRY(upload(st.sphereHot, &v.sphereHot, h->sceneBuffers));
    HIP_TRY(upload(st.sphereHotOffset, &v.sphereHotOffset, h->sceneBuffers));
    HIP_TRY(upload(st.sphereCold, &v.sphereCold, h->sceneBuffers));
    HIP_TRY(upload(st.material, &v.material, h->sceneBuffers));
    HIP_TRY(upload(st.light, &v.light, h->sceneBuffers));
    HIP_TRY(upload(st.gridCellStart, &v.grid.cellStart, h->sceneBuffers));
    HIP_TRY(upload(st.gridItems, &v.grid.items, h->sceneBuffers));
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
    HIP_TRY(upload(st.shadowRowBase, &v.shadow.rowBase, h->sceneBuffers));
    HIP_TRY(upload(st.shadowOff16, &v.shadow.off16, h->sceneBuffers));
    HIP_TRY(upload(st.shadowPacked, &v.shadow.items, h->sceneBuffers));
    HIP_TRY(upload(st.shadowInvKeyScale, &v.shadow.invKeyScale, h->sceneBuffers));
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
    h->lds = kajoLdsPlan(st, h->numerics);
    v.grid.inLds = h->lds.gridInLds ? 1 : 0;
    if (!h->lds.fits)
        return fail(KAJO_E_INVALID, "scene exceeds the LDS staging limit: scene records + the waves' mailboxes must fit 160 KiB");
    return KAJO_OK;
}

// The frame plan (the handle's base) and what follows from it before anything is allocated: its refusals, the large-LDS opt-ins, the
// AOV kernel of the scene's class
int planFrame(KajoHip* h)
{
    const KajoParams& p = h->params;
    static_cast<KajoFramePlan&>(*h) = kajoFramePlan(h->W, h->H, p, h->lds, h->numerics);
    if (h->tooManyBlocks)
        return fail(KAJO_E_INVALID, "frame too large: 2^28 pixel blocks per handle at most");
    if ((p.flags & KAJO_FLAG_ADAPTIVE) && !h->unitShift)
        return fail(KAJO_E_INVALID, "adaptive sampling: a unit is 64, 128 or 256 slots");
    h->noise = (p.flags & KAJO_FLAG_NOISE) != 0;
    h->adaptive = (p.flags & KAJO_FLAG_ADAPTIVE) != 0;
    if (h->lds.ldsTotal() > 48 * 1024)
        HIP_TRY((hipError_t)h->k->setLds(h->lds.coldInLds, h->lds.ldsTotal()));
    if (p.flags & KAJO_FLAG_AOV) {
        // the AOV kernel of the scene's class -- small scenes: everything in LDS; large ones: the hot records (and the grid's cell lists where
        // create() put them in LDS), per home of the cell lists and with or without visibility lists, as launch.inc.hip picks the render kernel
        if (h->lds.coldInLds)
            h->aovInstance = KAJO_AOV_SMALL;
        else if (h->view.shadow.enabled)
            h->aovInstance = h->view.grid.inLds ? KAJO_AOV_BIGLIST_LG : KAJO_AOV_BIGLIST;
        else
            h->aovInstance = h->view.grid.inLds ? KAJO_AOV_BIG_LG : KAJO_AOV_BIG;
        if (p.flags & KAJO_FLAG_AOV_SPECULAR) // the same scene class, with the chain to the first non-delta hit
            h->aovInstance += KAJO_AOV_SPEC_SMALL;
        if (p.flags & KAJO_FLAG_AOV_MATTE) // ... with the coverage tables beside the sums
            h->aovInstance += KAJO_AOV_MATTE_SMALL;
        h->aovLds = h->lds.coldInLds ? h->lds.ldsBytes : h->lds.hotBytes;
        if (h->aovLds > 48 * 1024)
            HIP_TRY((hipError_t)h->k->aovSetLds(h->aovInstance, h->aovLds));
        h->aovTiled = (p.flags & KAJO_FLAG_AOV_TILED) != 0;
    }
    return KAJO_OK;
}

// Every buffer that sums passes (clearAccumulators has the list), and the launch-order feedback
int allocAccumulators(KajoHip* h)
{
    const uint32_t flags = h->params.flags;
    HIP_TRY(h->tiles.alloc(h->tileBytes));
    if (flags & KAJO_FLAG_COUNTERS)
        HIP_TRY(h->counters.alloc(kCounterBytes));
    if (h->gridBlocks && !(flags & KAJO_FLAG_NO_REORDER)) {
        HIP_TRY(h->waveTrips.alloc((size_t)h->gridBlocks * h->lds.wavesPerBlock * sizeof(uint32_t)));
        HIP_TRY(h->blockOrder.alloc((size_t)h->gridBlocks * sizeof(uint32_t)));
    }
    if (flags & KAJO_FLAG_AOV) {
        // tiled: the sums of the handle's own tiles only (the whole-frame buffers: kajo_hip_compose_aov, on the handle it is called on)
        HIP_TRY(h->aovTiled ? h->aovTiles.alloc(aovTileBytes(h)) : h->aov.alloc(aovFrameBytes(h)));
        if (flags & KAJO_FLAG_AOV_MATTE)
            HIP_TRY(h->aovTiled ? h->matteTiles.alloc(matteTileBytes(h)) : h->matte.alloc(matteTableBytes(h)));
    }
    if (h->noise) {
        HIP_TRY(h->noiseBase.alloc(h->tileBytes));
        HIP_TRY(h->noiseMoments.alloc(momentBytes(h)));
    }
    if (h->adaptive)
        HIP_TRY(h->adaptStateDev.alloc(adaptStateBytes(h)));
    return clearAccumulators(h, true);
}

// An adaptive handle's orders, its pinned copy of the state words and the in-image pixels of every unit
int setupAdaptive(KajoHip* h)
{
    if (!h->adaptive)
        return KAJO_OK;
    const unsigned w = h->lds.wavesPerBlock;
    HIP_TRY(h->adaptUnits.alloc(adaptStateBytes(h)));
    HIP_TRY(h->adaptBlocks.alloc(adaptStateBytes(h) * w));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->adaptStateHost), adaptStateBytes(h), hipHostMallocDefault));
    std::memset(h->adaptStateHost, 0, adaptStateBytes(h));
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
    return KAJO_OK;
}

// What every launch's arguments have in common (kajo_hip_render sets the passes, the order and the carry; launchAov the passes)
void fillLaunchArgs(KajoHip* h)
{
    const KajoParams& p = h->params;
    const KajoLdsPlan& lds = h->lds;
    RenderArgs& a = h->renderArgs;
    std::memset(&a, 0, sizeof a);
    a.scene = h->view;
    a.tiles = h->tiles.p;
    a.W = h->W;
    a.H = h->H;
    a.n = h->n;
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
    lds.fillWaveLds(a, a.mailboxOffset, true);
    if (!(p.flags & KAJO_FLAG_AOV))
        return;
    AovArgs& g = h->aovArgs;
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
    g.seed = a.seed;
    if (p.flags & KAJO_FLAG_AOV_MATTE)
        g.matteIds = h->aovTiled ? h->matteTiles.p : h->matte.p;
    unsigned long long blocks = (unsigned long long)((h->W + 7) / 8) * ((h->H + 7) / 8);
    if (h->aovTiled) {
        // one wave per 8x8 block of the handle's own tiles, in the tile buffer's order (an owner without a tile launches nothing)
        blocks = (unsigned long long)h->nTilesOwned * (p.tileW / 8) * (p.tileH / 8);
        g.tiledBlocks = (int32_t)blocks;
        g.tileWaves = (uint32_t)(p.tileW / 8) | ((uint32_t)(p.tileH / 8) << 16);
        g.tileIndex = p.tileIndex;
        g.tileCount = p.tileCount;
    }
    h->aovGrid = (unsigned)((blocks + 3) / 4);
}

// ---- kajo_hip_render's steps -------------------------------------------------------------------------------------------------------

// What the next launch covers and in which order. Adaptive sampling: once a unit has retired the launches cover the active units only,
// in the handle's order without the others; a decision may have brought a new cost order in between, so the order is looked up launch
// by launch. The trips are measured by whole launches only; until a unit retires, as on any other handle.
struct LaunchOrder
{
    bool shortGrid;        // some unit has retired
    unsigned activeUnits;  // workgroups of an unsplit launch; 0: every unit retired, the passes are counted and nothing is rendered
    const uint32_t* units; // the order words of an unsplit launch, or null: image order
    const uint32_t* pixelBlocks; // the SPLIT kernels': null (one round or two: the launch order does not matter), or the active units' pixel blocks
    uint32_t* trips;       // where this launch records its waves' trips, or null
};

LaunchOrder launchOrder(const KajoHip* h, uint32_t* trips)
{
    LaunchOrder o;
    o.shortGrid = h->adaptive && h->adaptRetired > 0;
    o.activeUnits = (unsigned)h->gridBlocks - (h->adaptive ? h->adaptRetired : 0u);
    o.units = o.shortGrid ? h->adaptUnits.as<const uint32_t>() : h->orderValid ? h->blockOrder.as<const uint32_t>() : nullptr;
    o.pixelBlocks = o.shortGrid ? h->adaptBlocks.as<const uint32_t>() : nullptr;
    o.trips = o.shortGrid ? nullptr : trips;
    return o;
}

// One launch of the render kernel -- one of three arms by its shape -- between a pair of timing events (KajoCounters.kernelMs)
int launchRender(KajoHip* h, const RenderArgs& a, const KajoLaunchShape& s, const LaunchOrder& o, int now)
{
    const KajoLdsPlan& lds = h->lds;
    const unsigned block = 64 * lds.wavesPerBlock, grid = (unsigned)h->gridBlocks;
    h->lastTailGroups = 0;
    if (o.activeUnits == 0)
        return KAJO_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const auto between = [&]() -> int {
        hipError_t le;
        int rc;
        HIP_TRY(hipEventRecord(e0, h->stream));
        if (s.chunks > 1 || s.split > 1) {
            // the waves of a block divide the samples of every pass (behind the [pass][sample][pixel] table) or the passes (behind the
            // [pass][pixel] term table); one round or two: the launch order does not matter
            RenderArgs b = a;
            b.blockOrder = o.pixelBlocks;
            b.waveTrips = nullptr;
            if (s.chunks > 1)
                b.sampleChunks = (int32_t)s.chunks;
            const unsigned waves = s.chunks > 1 ? (unsigned)now * s.chunks : s.split;
            lds.fillWaveLds(b, a.mailboxOffset + (size_t)now * (s.chunks > 1 ? a.n * a.n : 1) * 64 * 16, false);
            b.thrL = 1; // (short waves: holding a vertex only lengthens their tail -- configs[0] 18.9 against 16.5 G paths/s; 1-3 % on
                        // split frames below 720p)
            le = (hipError_t)h->k->split(&b, o.shortGrid ? o.activeUnits * lds.wavesPerBlock : (unsigned)h->pixelBlocks, 64 * waves,
                                         b.perWaveOffset + (size_t)waves * b.perWaveBytes, h->stream);
        } else if (s.parted && !o.shortGrid) { // (a noise handle's launches are of one group at the most: never parted)
            // the launch tail: the cheapest blocks as one workgroup per group of the launch (partTheTail)
            if ((rc = partedOrderFor(h, s.launchGroups)))
                return rc;
            h->lastTailGroups = h->nParted * (unsigned)(s.launchGroups - 1);
            RenderArgs b = a;
            b.blockOrder = h->partedOrder[s.launchGroups].as<const uint32_t>();
            b.side = h->side.p;
            b.sideStride = h->nParted * block;
            b.partedFirst = grid - h->nParted;
            le = (hipError_t)h->k->render(&b, h->home, grid + h->lastTailGroups, block, lds.ldsTotal(), h->stream);
            if (le == hipSuccess)
                le = (hipError_t)kajo_fold_parts_launch(h->tiles.p, h->side.p, b.sideStride, h->partedBlocks.as<const uint32_t>(), h->nParted, block,
                                                        s.launchGroups, h->stream);
        } else {
            le = (hipError_t)h->k->render(&a, h->home, o.activeUnits, block, lds.ldsTotal(), h->stream);
        }
        if (le != hipSuccess)
            return failHip(le, "render kernel launch");
        HIP_TRY(hipEventRecord(e1, h->stream));
        return KAJO_OK;
    };
    int rc = getEvent(h, &e0);
    if (!rc && !(rc = getEvent(h, &e1)))
        rc = between();
    if (rc) { // the one place a pair goes back to the pool unused
        for (hipEvent_t e : {e0, e1})
            if (e)
                h->eventPool.push_back(e);
        return rc;
    }
    h->pending.emplace_back(e0, e1);
    return KAJO_OK;
}

// The first-hit AOVs of the same passes, behind the render launch and outside its timing events (KajoCounters.kernelMs)
int launchAov(KajoHip* h, int now)
{
    AovArgs g = h->aovArgs;
    g.firstPass = h->passesDone + 1;
    g.nPasses = now;
    HIP_TRY((hipError_t)h->k->aov(&g, h->aovInstance, h->aovGrid, h->aovLds, h->stream));
    h->aovPasses += now;
    return KAJO_OK;
}

// Behind every launch and outside the timing events: what the noise estimate and adaptive sampling do with the new passes
int afterLaunch(KajoHip* h, int now, bool shortGrid)
{
    const int after = h->passesDone + now, boundary = after % KAJO_NOISE_BATCH_PASSES == 0;
    const uint32_t slots = (uint32_t)((size_t)h->nTilesOwned * h->map.tileW * h->map.tileH);
    if (shortGrid) {
        // adaptive sampling: the retired slots extended to the new pass count and, at a batch boundary, the batch into the moments of the
        // active ones (a handle that retires has rendered every pass: no rebase)
        HIP_TRY((hipError_t)kajo_adapt_step_launch(h->tiles.p, h->noiseBase.p, h->noiseMoments.p, h->adaptStateDev.p, slots, h->unitShift, boundary,
                                                   after, h->stream));
    } else if (h->noise && boundary) {
        // a batch boundary, behind the launch (and its fold): the batch into the moments -- or, where this handle did not render all of
        // it, only the baseline
        if (h->noiseRebase)
            HIP_TRY(hipMemcpyAsync(h->noiseBase.p, h->tiles.p, h->tileBytes, hipMemcpyDeviceToDevice, h->stream));
        else
            HIP_TRY((hipError_t)kajo_noise_update_launch(h->tiles.p, h->noiseBase.p, h->noiseMoments.p, slots, h->stream));
        h->noiseRebase = false;
    }
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
    return "kajo-hip 0.1 (gfx950; aov-matte; local; aov-tiled; lens, view, grade, denoise-guided, encode, encode-view)";
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
    KajoParams p = *params;
    char msg[256];
    if (const char* refusal = kajoCheckCreate(*scene, width, height, &p, msg))
        return fail(KAJO_E_INVALID, refusal);

    int nDev = 0;
    hipError_t e = hipGetDeviceCount(&nDev);
    if (e != hipSuccess || nDev <= 0)
        return fail(KAJO_E_NO_DEVICE, "no HIP device available; this backend has no CPU path");
    if (p.device < 0 || p.device >= nDev)
        return fail(KAJO_E_INVALID, "device ordinal out of range");

    // (whatever fails from here on: destroy() frees what the handle has so far)
    std::unique_ptr<KajoHip, void (*)(KajoHip*)> h(new (std::nothrow) KajoHip, destroy);
    if (!h)
        return fail(KAJO_E_INVALID, "out of host memory");
    h->device = p.device;
    h->params = p;
    h->W = width;
    h->H = height;
    h->numerics = kajoNumerics(p.flags);
    h->sceneHash = kajoCkptSceneHash(*scene); // (the checkpoints' fingerprint: the handle does not keep the scene it was given)
    h->k = h->numerics == Numerics::Strict ? &kStrictKernels : h->numerics == Numerics::Exact ? &kExactKernels : &kFastKernels;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->ownStream = true;
    int rc;
    if ((rc = uploadScene(h.get(), *scene)) || (rc = planFrame(h.get())) || (rc = allocAccumulators(h.get())) || (rc = setupAdaptive(h.get())))
        return rc;
    fillLaunchArgs(h.get());
    HIP_TRY(hipStreamSynchronize(h->stream));
    *out = h.release();
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
    RenderArgs a = h->renderArgs;
    uint32_t* trips = (h->waveTrips && !h->orderValid) ? h->waveTrips.as<uint32_t>() : nullptr; // measure once, on the first launch
    // (the noise estimate: a baseline owed since kajo_hip_set_pass_count to a multiple of four is the buffer as it stands now)
    if (h->noise && h->noiseRebase && h->passesDone % KAJO_NOISE_BATCH_PASSES == 0) {
        HIP_TRY(hipMemcpyAsync(h->noiseBase.p, h->tiles.p, h->tileBytes, hipMemcpyDeviceToDevice, h->stream));
        h->noiseRebase = false;
    }
    for (int left = passes, now; left > 0; left -= now) {
        // cut, order, shape
        now = kajoLaunchPasses(left, h->params.passesPerLaunch, h->noise, h->passesDone);
        const LaunchOrder o = launchOrder(h, trips);
        const KajoLaunchShape s = kajoLaunchShape(*h, h->lds, h->params.flags, now, h->passesDone, h->orderValid, h->nParted);
        a.firstPass = h->passesDone + 1;
        a.nPasses = now;
        a.blockOrder = o.units;
        a.waveTrips = o.trips;
        if (s.startsInside || s.endsInside)
            HIP_TRY(h->carry.ensure(2 * h->tileBytes));
        a.carry = h->carry.p;
        // (a group whose first passes this handle did not render -- kajo_hip_set_pass_count to the middle of one -- continues from the
        // buffer as it stands: the restored sum counts as complete groups)
        a.carryIn = s.startsInside && h->carryValid;
        a.carryOut = s.endsInside;
        // launch, AOV, after-launch
        if ((rc = launchRender(h, a, s, o, now)) || ((h->params.flags & KAJO_FLAG_AOV) && (rc = launchAov(h, now))) ||
            (rc = afterLaunch(h, now, o.shortGrid)))
            return rc;
        // bookkeeping
        if (o.trips && s.split == 1 && s.chunks == 1) {
            h->tripsPending = true;
            trips = nullptr; // later launches of this call keep the first measurement
        }
        if (o.activeUnits > 0)
            h->launches++;
        h->passesDone += now;
        h->carryValid = s.endsInside;
        if (h->adaptive) {
            h->adaptPaths += h->adaptActivePixels * h->n * h->n * now;
            if (h->adaptSet && o.activeUnits > 0 && !h->noiseRebase && h->passesDone >= h->adaptParams.minPasses &&
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
    if (rc || (rc = clearAccumulators(h, true)))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    adaptReactivate(h);
    h->noiseRebase = false;
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
    if (h->noise) {
        // the moments start over (an adaptive handle, to pass 0: and so do the units); the baseline is the buffer at the first batch
        // boundary from here on (kajo_hip_render)
        if ((rc = clearAccumulators(h, false)))
            return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        adaptReactivate(h);
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
    HIP_TRY(h->aov.ensure(aovFrameBytes(h)));
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
        forOwnedPixels(h, [&](size_t at, uint32_t) {
            for (int k = 0; k < 4; k++)
                if (dst[k])
                    static_cast<uint32_t*>(dst[k])[at] = h->noiseStaged[k * pixels + at];
        });
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
    forOwnedPixels(h, [&](size_t at, uint32_t slot) { records[at] = own[slot]; });
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
    hipError_t le = (hipError_t)kajo_adapt_passes_launch(h->noiseMoments.p, h->adaptStateDev.p, &h->map, h->params.tileIndex, h->unitShift,
                                                         (uint32_t)h->passesDone, h->adaptOut.p, h->stream);
    if (le != hipSuccess)
        return failHip(le, "adaptive pass plane kernel launch");
    HIP_TRY(hipMemcpyAsync(part ? h->adaptStaged.data() : plane, h->adaptOut.p, pixels * 4, hipMemcpyDeviceToHost, h->stream));
    if ((rc = kajo_hip_wait(h)))
        return rc;
    if (part)
        forOwnedPixels(h, [&](size_t at, uint32_t) { plane[at] = h->adaptStaged[at]; });
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

extern "C" {

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

// checkpoints: kajo_hip_checkpoint_*, kajo_hip_digest
#include "checkpoint.cpp"
