// checkpoint.cpp -- checkpoints (include/kajo_hip.h "Checkpoints"): a handle's accumulated state as a self-describing section in canonical
// order, its restore, the planes' digests of a live handle; info and merge, pure host, are checkpoint_host.h's. The kernels are
// checkpoint_kernels.cpp's, the arithmetic checkpoint_math.h's. save, restore and digest wait for the handle's stream.
// Part of capi.cpp's translation unit, which includes this file at its end (the handle is private to capi.cpp and present.cpp).

namespace
{

// A per-pixel plane where the handle keeps it: `parts` consecutive arrays of `elems` pieces of `vecs` 16-byte vectors, in the tile layout
// (a pixel's piece at kajoTileSlot's slot) or row-major over the whole frame
struct PlaneSource
{
    uint32_t kind;
    void* base;
    uint32_t parts, vecs, elems;
    int tiled;
};

constexpr unsigned kSumWords = 16; // digests in front of the partial sums in ckptSums

// the per-pixel planes the handle keeps now, in the order of their kinds. carry: with the CARRY plane (restore: the section's; else the
// handle's own carryValid)
std::vector<PlaneSource> planeSources(const KajoHip* h, bool carry)
{
    const uint32_t flags = h->params.flags;
    const uint32_t slots = (uint32_t)h->map.slotsPerOwner, frame = (uint32_t)((size_t)h->W * h->H);
    std::vector<PlaneSource> v;
    v.push_back({KAJO_CKPT_SUM, h->tiles.p, 1, 1, slots, 1});
    if (carry)
        v.push_back({KAJO_CKPT_CARRY, h->carry.p, 2, 1, slots, 1});
    if (flags & KAJO_FLAG_AOV)
        v.push_back(h->aovTiled ? PlaneSource{KAJO_CKPT_AOV, h->aovTiles.p, 2, 1, slots, 1} : PlaneSource{KAJO_CKPT_AOV, h->aov.p, 2, 1, frame, 0});
    if (flags & KAJO_FLAG_AOV_MATTE)
        v.push_back(h->aovTiled ? PlaneSource{KAJO_CKPT_MATTE, h->matteTiles.p, 2, 2, slots, 1}
                                : PlaneSource{KAJO_CKPT_MATTE, h->matte.p, 2, 2, frame, 0});
    if (h->noise) {
        v.push_back({KAJO_CKPT_NOISE_BASE, h->noiseBase.p, 1, 1, slots, 1});
        v.push_back({KAJO_CKPT_NOISE_MOMENTS, h->noiseMoments.p, 1, 2, slots, 1});
    }
    return v;
}

// the kinds the handle keeps whatever its pass count (CARRY comes and goes with it)
uint32_t steadyKinds(const KajoHip* h)
{
    uint32_t set = 0;
    for (const PlaneSource& s : planeSources(h, false))
        set |= 1u << s.kind;
    if (h->adaptive)
        set |= 1u << KAJO_CKPT_ADAPT;
    if (h->counters)
        set |= 1u << KAJO_CKPT_COUNTERS;
    return set;
}

KajoCkptGeom geomOf(const KajoHip* h)
{
    return kajoCkptGeom(h->map, h->params.tileIndex);
}

uint64_t pixelsOf(const KajoHip* h)
{
    return h->ckptPrefixHost.back();
}

// The staging buffer, the prefix table and the sums, on the first call
int ensureBuffers(KajoHip* h)
{
    if (h->ckptPrefixHost.empty()) {
        const KajoCkptGeom g = geomOf(h);
        std::vector<uint32_t> prefix((size_t)g.tilesY + 1);
        kajoCkptPrefix(g, prefix.data());
        HIP_TRY(h->ckptPrefix.alloc(prefix.size() * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(h->ckptPrefix.p, prefix.data(), prefix.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        h->ckptPrefixHost.swap(prefix);
    }
    // the widest plane the handle can keep: the tables' 16 words per pixel, else 8 (the carry, the AOVs, the moments)
    const size_t widest = (h->params.flags & KAJO_FLAG_AOV_MATTE) ? 64 : 32;
    HIP_TRY(h->ckptStaging.ensure((size_t)pixelsOf(h) * widest));
    HIP_TRY(h->ckptSums.ensure((kSumWords + 1024) * sizeof(uint64_t)));
    return KAJO_OK;
}

// the ADAPT block of the handle
std::vector<uint32_t> adaptBlock(const KajoHip* h)
{
    std::vector<uint32_t> w(KAJO_CKPT_ADAPT_WORDS + (size_t)h->gridBlocks, 0u);
    std::memcpy(w.data(), &h->adaptParams, sizeof h->adaptParams); // words 0 .. 7
    w[8] = h->adaptSet ? 1u : 0u;
    w[9] = h->adaptRetired;
    w[10] = (uint32_t)h->adaptLastDecision;
    w[11] = (uint32_t)h->gridBlocks;
    w[12] = 64u * h->lds.wavesPerBlock;
    const uint64_t paths = (uint64_t)h->adaptPaths;
    w[14] = (uint32_t)paths;
    w[15] = (uint32_t)(paths >> 32);
    if (h->gridBlocks)
        std::memcpy(w.data() + KAJO_CKPT_ADAPT_WORDS, h->adaptStateHost, (size_t)h->gridBlocks * sizeof(uint32_t));
    return w;
}

// The header and the planes' table of the handle's section as it stands (sizes and offsets; no digests yet): the section's size returned
uint64_t describe(const KajoHip* h, KajoCheckpointHeader* header, KajoCheckpointPlane* planes)
{
    KajoCheckpointHeader& hd = *header;
    std::memset(&hd, 0, sizeof hd);
    std::memcpy(hd.magic, kCkptMagic, 8);
    hd.version = KAJO_CKPT_VERSION;
    hd.width = h->W;
    hd.height = h->H;
    hd.tileW = h->params.tileW;
    hd.tileH = h->params.tileH;
    hd.tileIndex = h->params.tileIndex;
    hd.tileCount = h->params.tileCount;
    hd.flags = h->params.flags;
    hd.samplesPerPass = h->params.samplesPerPass;
    hd.depthLimit = h->params.depthLimit;
    hd.passesDone = h->passesDone;
    hd.seed = h->params.seed;
    hd.fingerprint = kajoCkptFingerprint(h->sceneHash, h->W, h->H, h->params);
    hd.pixels = pixelsOf(h);
    hd.aovPasses = h->aovPasses;
    hd.noiseRebase = h->noiseRebase ? 1 : 0;
    uint32_t n = 0;
    std::memset(planes, 0, KAJO_CKPT_KINDS * sizeof *planes);
    for (const PlaneSource& s : planeSources(h, h->carryValid)) {
        planes[n].kind = s.kind;
        planes[n].wordsPerPixel = s.parts * s.vecs * 4;
        planes[n].bytes = hd.pixels * planes[n].wordsPerPixel * 4u;
        n++;
    }
    if (h->adaptive) {
        planes[n].kind = KAJO_CKPT_ADAPT;
        planes[n].bytes = (KAJO_CKPT_ADAPT_WORDS + (uint64_t)h->gridBlocks) * 4u;
        n++;
    }
    if (h->counters) {
        planes[n].kind = KAJO_CKPT_COUNTERS;
        planes[n].bytes = 32;
        n++;
    }
    hd.nPlanes = n;
    hd.bytes = kajoCkptLayout(planes, n) + sizeof(KajoCheckpointTrailer);
    return hd.bytes;
}

// Pack the planes one by one and take their digests (sums[i] on the device, in the planes' order); with `blob`, each plane's records
// go to blob + offsets[i] behind its digest kernel. Enqueued on the handle's stream; the caller synchronises.
int packPlanes(KajoHip* h, const std::vector<PlaneSource>& sources, unsigned char* blob, const KajoCheckpointPlane* planes)
{
    const KajoCkptGeom g = geomOf(h);
    const uint32_t pixels = (uint32_t)pixelsOf(h);
    uint64_t* sums = h->ckptSums.as<uint64_t>();
    for (size_t i = 0; i < sources.size(); i++) {
        const PlaneSource& s = sources[i];
        hipError_t le = (hipError_t)kajo_ckpt_pack_launch(s.base, &g, h->ckptPrefix.p, pixels, s.parts, s.vecs, s.elems, s.tiled, h->ckptStaging.p, h->stream);
        if (le == hipSuccess)
            le = (hipError_t)kajo_ckpt_digest_launch(h->ckptStaging.p, &g, h->ckptPrefix.p, pixels, s.parts * s.vecs, sums + kSumWords, sums + i, h->stream);
        if (le != hipSuccess)
            return failHip(le, "checkpoint kernel launch");
        if (blob && planes[i].bytes)
            HIP_TRY(hipMemcpyAsync(blob + planes[i].offset, h->ckptStaging.p, (size_t)planes[i].bytes, hipMemcpyDeviceToHost, h->stream));
    }
    return KAJO_OK;
}

// the preamble of the entry points on a handle: the device, the stream drained, the buffers
int ready(KajoHip* h)
{
    int rc = kajo_hip_wait(h);
    if (rc)
        return rc;
    return ensureBuffers(h);
}

} // namespace

extern "C" {

int kajo_hip_checkpoint_bytes(kajo_hip_t h, size_t* bytes)
{
    if (!h || !bytes)
        return fail(KAJO_E_INVALID, "null argument");
    int rc = ready(h);
    if (rc)
        return rc;
    KajoCheckpointHeader header;
    KajoCheckpointPlane planes[KAJO_CKPT_KINDS];
    *bytes = (size_t)describe(h, &header, planes);
    return KAJO_OK;
}

int kajo_hip_checkpoint_save(kajo_hip_t h, void* blob, size_t capacity, size_t* written)
{
    if (!h || !blob || !written)
        return fail(KAJO_E_INVALID, "null argument");
    *written = 0;
    int rc = ready(h);
    if (rc)
        return rc;
    KajoCheckpointHeader header;
    KajoCheckpointPlane planes[KAJO_CKPT_KINDS];
    const uint64_t total = describe(h, &header, planes);
    if (capacity < total)
        return fail(KAJO_E_INVALID, "checkpoint: the blob is smaller than kajo_hip_checkpoint_bytes says");
    unsigned char* out = static_cast<unsigned char*>(blob);
    std::memset(out, 0, (size_t)total); // (the padding between the planes: the blob is a function of the state)
    const std::vector<PlaneSource> sources = planeSources(h, h->carryValid);
    if ((rc = packPlanes(h, sources, out, planes)))
        return rc;
    uint64_t sums[kSumWords] = {};
    HIP_TRY(hipMemcpyAsync(sums, h->ckptSums.p, sizeof sums, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    uint32_t i = 0;
    for (; i < sources.size(); i++)
        planes[i].digest = sums[i];
    if (h->adaptive) {
        const std::vector<uint32_t> block = adaptBlock(h);
        std::memcpy(out + planes[i].offset, block.data(), block.size() * sizeof(uint32_t));
        planes[i].digest = kajoCkptDigestWords(block.data(), block.size());
        i++;
    }
    if (h->counters) {
        uint32_t words[8];
        HIP_TRY(hipMemcpy(words, h->counters.p, sizeof words, hipMemcpyDeviceToHost));
        std::memcpy(out + planes[i].offset, words, sizeof words);
        planes[i].digest = kajoCkptDigestWords(words, 8);
        i++;
    }
    const KajoCheckpointTrailer trailer{h->kernelMs, h->launches};
    std::memcpy(out, &header, sizeof header);
    std::memcpy(out + sizeof header, planes, (size_t)header.nPlanes * sizeof(KajoCheckpointPlane));
    std::memcpy(out + total - sizeof trailer, &trailer, sizeof trailer);
    *written = (size_t)total;
    return KAJO_OK;
}

int kajo_hip_digest(kajo_hip_t h, KajoDigest* out)
{
    if (!h || !out)
        return fail(KAJO_E_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    int rc = ready(h);
    if (rc)
        return rc;
    const std::vector<PlaneSource> sources = planeSources(h, h->carryValid);
    if ((rc = packPlanes(h, sources, nullptr, nullptr)))
        return rc;
    uint64_t sums[kSumWords] = {};
    HIP_TRY(hipMemcpyAsync(sums, h->ckptSums.p, sizeof sums, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < sources.size(); i++) {
        out->plane[sources[i].kind] = sums[i];
        out->present |= 1u << sources[i].kind;
    }
    if (h->adaptive) {
        const std::vector<uint32_t> block = adaptBlock(h);
        out->plane[KAJO_CKPT_ADAPT] = kajoCkptDigestWords(block.data(), block.size());
        out->present |= 1u << KAJO_CKPT_ADAPT;
    }
    if (h->counters) {
        uint32_t words[8];
        HIP_TRY(hipMemcpy(words, h->counters.p, sizeof words, hipMemcpyDeviceToHost));
        out->plane[KAJO_CKPT_COUNTERS] = kajoCkptDigestWords(words, 8);
        out->present |= 1u << KAJO_CKPT_COUNTERS;
    }
    return KAJO_OK;
}

int kajo_hip_checkpoint_info(const void* blob, size_t bytes, KajoCheckpointInfo* out)
{
    if (!blob || !out)
        return fail(KAJO_E_INVALID, "null argument");
    std::string why;
    if (!kajoCkptInfo(blob, bytes, out, &why))
        return fail(KAJO_E_INVALID, why);
    return KAJO_OK;
}

int kajo_hip_checkpoint_merge(const void* const* blobs, const size_t* bytes, int n, void* out, size_t capacity, size_t* written)
{
    if (!blobs || !bytes || !written || n < 1)
        return fail(KAJO_E_INVALID, "null argument");
    *written = 0;
    for (int i = 0; i < n; i++)
        if (!blobs[i])
            return fail(KAJO_E_INVALID, "null section");
    std::vector<unsigned char> merged;
    std::string why;
    if (!kajoCkptMerge(blobs, bytes, n, merged, &why))
        return fail(KAJO_E_INVALID, why);
    *written = merged.size(); // (with out == NULL: the size to come back with)
    if (!out)
        return KAJO_OK;
    if (capacity < merged.size())
        return fail(KAJO_E_INVALID, "checkpoint merge: the output is smaller than the merged section");
    std::memcpy(out, merged.data(), merged.size());
    return KAJO_OK;
}

int kajo_hip_checkpoint_restore(kajo_hip_t h, const void* blob, size_t bytes)
{
    if (!h || !blob)
        return fail(KAJO_E_INVALID, "null argument");
    // 1. the blob by itself
    KajoCheckpointInfo info;
    std::string why;
    if (!kajoCkptInfo(blob, bytes, &info, &why))
        return fail(KAJO_E_INVALID, why);
    const KajoCheckpointHeader& hd = info.header;
    // 2. against the handle, which is not touched before all of it holds
    // (field by field as well: the fingerprint is the blob's own word, and the sizes below are computed from the handle's frame)
    if (hd.width != h->W || hd.height != h->H || hd.samplesPerPass != h->params.samplesPerPass || hd.depthLimit != h->params.depthLimit ||
        hd.seed != h->params.seed || hd.fingerprint != kajoCkptFingerprint(h->sceneHash, h->W, h->H, h->params))
        return fail(KAJO_E_INVALID, "checkpoint: the section is of another scene or of other parameters than the handle (fingerprint)");
    const uint32_t kinds = kajoCkptKinds(info), carryBit = 1u << KAJO_CKPT_CARRY;
    if ((kinds & ~carryBit) != steadyKinds(h))
        return fail(KAJO_E_INVALID, "checkpoint: the section's planes are not the ones the handle keeps (its flags)");
    if ((kinds & carryBit) && !h->grouped)
        return fail(KAJO_E_INVALID, "checkpoint: plane CARRY in a section for a handle that adds pass by pass");
    const bool sameLayout = hd.tileW == h->params.tileW && hd.tileH == h->params.tileH && hd.tileIndex == h->params.tileIndex &&
                            hd.tileCount == h->params.tileCount;
    if (!sameLayout && hd.tileCount != 1)
        return fail(KAJO_E_INVALID, "checkpoint: the section is neither of the handle's tile layout nor a whole-frame section (kajo_hip_checkpoint_merge)");
    const unsigned char* b = static_cast<const unsigned char*>(blob);
    std::vector<uint32_t> adapt;
    if (const KajoCheckpointPlane* p = kajoCkptFind(info, KAJO_CKPT_ADAPT)) {
        if (!sameLayout)
            return fail(KAJO_E_INVALID, "checkpoint: a section with an ADAPT block restores into its own tile layout only (units are launch blocks)");
        adapt.resize((size_t)(p->bytes / 4));
        std::memcpy(adapt.data(), b + p->offset, (size_t)p->bytes);
        if (adapt.size() != KAJO_CKPT_ADAPT_WORDS + (size_t)h->gridBlocks || adapt[11] != (uint32_t)h->gridBlocks || adapt[12] != 64u * h->lds.wavesPerBlock)
            return fail(KAJO_E_INVALID, "checkpoint: plane ADAPT is not of the handle's units");
    }
    int rc = ready(h);
    if (rc)
        return rc;
    const KajoCkptGeom g = geomOf(h);
    const uint64_t pixels = pixelsOf(h);
    if (hd.pixels != (sameLayout ? pixels : (uint64_t)h->W * (uint64_t)h->H))
        return fail(KAJO_E_INVALID, "checkpoint: the section's pixel count is not the handle's");
    const bool carry = (kinds & carryBit) != 0 && pixels > 0;
    // 3. the planes: the handle's own pixels of each (a whole-frame section: picked out here), to the staging buffer, to their places
    if (carry)
        HIP_TRY(h->carry.ensure(2 * h->tileBytes));
    std::vector<uint32_t> own;
    for (const PlaneSource& s : planeSources(h, carry)) {
        const KajoCheckpointPlane* p = kajoCkptFind(info, s.kind);
        const uint32_t w = p->wordsPerPixel;
        const void* from = b + p->offset;
        if (!sameLayout) {
            own.resize((size_t)pixels * w);
            for (uint64_t r = 0; r < pixels; r++) {
                int x, y;
                kajoCkptPixel(g, h->ckptPrefixHost.data(), (uint32_t)r, &x, &y);
                std::memcpy(&own[(size_t)r * w], b + p->offset + ((size_t)y * h->W + x) * w * 4u, (size_t)w * 4u);
            }
            from = own.data();
        }
        if (pixels)
            HIP_TRY(hipMemcpyAsync(h->ckptStaging.p, from, (size_t)pixels * w * 4u, hipMemcpyHostToDevice, h->stream));
        HIP_TRY((hipError_t)kajo_ckpt_unpack_launch(h->ckptStaging.p, &g, h->ckptPrefix.p, s.parts, s.vecs, s.elems, s.tiled, s.base, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream)); // (`own` and the staging buffer serve the next plane)
    }
    if (const KajoCheckpointPlane* p = kajoCkptFind(info, KAJO_CKPT_COUNTERS))
        HIP_TRY(hipMemcpy(h->counters.p, b + p->offset, 32, hipMemcpyHostToDevice));
    // 4. the host's state
    h->passesDone = hd.passesDone;
    h->aovPasses = hd.aovPasses;
    h->carryValid = carry;
    h->noiseRebase = hd.noiseRebase != 0;
    h->frameValid = false;
    h->aovComposed = h->matteComposed = false;
    h->orderValid = false; // (the launch order is measured again)
    h->tripsPending = false;
    h->guideStamp = -1;
    std::memcpy(&h->kernelMs, b + hd.bytes - sizeof(KajoCheckpointTrailer), sizeof(double));
    std::memcpy(&h->launches, b + hd.bytes - sizeof(uint64_t), sizeof(uint64_t));
    h->lastTailGroups = 0;
    if (h->adaptive) {
        std::memcpy(&h->adaptParams, adapt.data(), sizeof h->adaptParams);
        h->adaptSet = adapt[8] != 0;
        h->adaptLastDecision = (int)adapt[10];
        h->adaptPaths = (long long)((uint64_t)adapt[14] | (uint64_t)adapt[15] << 32);
        unsigned retired = 0;
        long long active = 0;
        for (unsigned u = 0; u < h->gridBlocks; u++) {
            h->adaptStateHost[u] = adapt[KAJO_CKPT_ADAPT_WORDS + u];
            if (h->adaptStateHost[u] != KAJO_ADAPT_ACTIVE)
                retired++;
            else
                active += h->adaptUnitPixels[u];
        }
        h->adaptRetired = retired;
        h->adaptActivePixels = active;
        if (h->gridBlocks)
            HIP_TRY(hipMemcpy(h->adaptStateDev.p, h->adaptStateHost, (size_t)h->gridBlocks * sizeof(uint32_t), hipMemcpyHostToDevice));
        if ((rc = adaptUploadOrder(h)))
            return rc;
    }
    return KAJO_OK;
}

} // extern "C"
