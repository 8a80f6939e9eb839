// checkpoint_host.h -- the host half of checkpoints (include/kajo_hip.h "Checkpoints") without HIP: the fingerprint, the layout of a section,
// the checks of kajo_hip_checkpoint_info and the whole of kajo_hip_checkpoint_merge. checkpoint.cpp wraps them into the C ABI; the
// stand-alone program of tests/test_checkpoint_cpu.py runs the same lines under the sanitizers. Static functions: no symbols of
// libkajo_hip.so's. A refusal is its sentence in *why.
#ifndef KAJO_CHECKPOINT_HOST_H
#define KAJO_CHECKPOINT_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "kajo_hip.h"

#include "checkpoint_math.h"

static_assert(sizeof(KajoCheckpointHeader) == 104 && sizeof(KajoCheckpointPlane) == 32 && sizeof(KajoCheckpointTrailer) == 16 &&
                  sizeof(KajoCheckpointInfo) == 408 && sizeof(KajoDigest) == 80,
              "include/kajo_hip.h states the sizes");

static const char kCkptMagic[8] = {'K', 'A', 'J', 'O', 'C', 'K', 'P', 'T'};

// the flags that choose what is computed (the others say which planes exist, or how the same bits are scheduled)
constexpr uint32_t kCkptFingerprintFlags =
    KAJO_FLAG_STRICT | KAJO_FLAG_EXACT | KAJO_FLAG_NO_GRID | KAJO_FLAG_NO_SHADOW_LISTS | KAJO_FLAG_NO_ONE_LIGHT | KAJO_FLAG_AOV_SPECULAR;

static inline uint64_t kajoCkptHashWords(uint64_t h, const void* data, size_t bytes)
{
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i + 4 <= bytes; i += 4) {
        uint32_t w;
        memcpy(&w, p + i, 4);
        h = kajoCkptMix(h ^ (uint64_t)w);
    }
    return h;
}

// the KajoScene POD's bytes: the fields in front of the two pointers, the spheres, the planes
static inline uint64_t kajoCkptSceneHash(const KajoScene& scene)
{
    uint64_t h = kajoCkptHashWords(0, &scene, offsetof(KajoScene, spheres));
    if (scene.nSpheres > 0 && scene.spheres)
        h = kajoCkptHashWords(h, scene.spheres, (size_t)scene.nSpheres * sizeof(KajoSphere));
    if (scene.nPlanes > 0 && scene.planes)
        h = kajoCkptHashWords(h, scene.planes, (size_t)scene.nPlanes * sizeof(KajoPlane));
    return h;
}

static inline uint64_t kajoCkptFingerprint(uint64_t sceneHash, int W, int H, const KajoParams& p)
{
    const uint32_t words[8] = {(uint32_t)W, (uint32_t)H, (uint32_t)p.samplesPerPass, (uint32_t)p.depthLimit, (uint32_t)p.seed, (uint32_t)(p.seed >> 32),
                               p.flags & kCkptFingerprintFlags, KAJO_CKPT_VERSION};
    return kajoCkptHashWords(sceneHash, words, sizeof words);
}

static inline const char* kajoCkptKindName(uint32_t kind)
{
    static const char* const names[KAJO_CKPT_KINDS] = {"?", "SUM", "CARRY", "AOV", "MATTE", "NOISE_BASE", "NOISE_MOMENTS", "ADAPT", "COUNTERS"};
    return kind < KAJO_CKPT_KINDS ? names[kind] : "?";
}

// words per pixel of a kind; 0: not per pixel
static inline uint32_t kajoCkptKindWords(uint32_t kind)
{
    static const uint32_t words[KAJO_CKPT_KINDS] = {0, 4, 8, 8, 16, 4, 8, 0, 0};
    return kind < KAJO_CKPT_KINDS ? words[kind] : 0;
}

static inline uint64_t kajoCkptAlign(uint64_t v)
{
    return (v + 15u) & ~(uint64_t)15u;
}

// The layout of a section from its planes' kinds and sizes: the offsets into planes[], the trailer's offset returned; the section is 16
// bytes longer
static inline uint64_t kajoCkptLayout(KajoCheckpointPlane* planes, uint32_t nPlanes)
{
    uint64_t at = kajoCkptAlign(sizeof(KajoCheckpointHeader) + (uint64_t)nPlanes * sizeof(KajoCheckpointPlane));
    for (uint32_t i = 0; i < nPlanes; i++) {
        planes[i].offset = at;
        at = kajoCkptAlign(at + planes[i].bytes);
    }
    return at;
}

static inline KajoCkptGeom kajoCkptGeomOf(const KajoCheckpointHeader& h)
{
    KajoCkptGeom g;
    g.W = h.width;
    g.H = h.height;
    g.tileW = h.tileW;
    g.tileH = h.tileH;
    g.tilesX = (int32_t)(((long long)h.width + h.tileW - 1) / h.tileW);
    g.tilesY = (int32_t)(((long long)h.height + h.tileH - 1) / h.tileH);
    g.tileIndex = h.tileIndex;
    g.tileCount = h.tileCount;
    return g;
}

// kajo_hip_checkpoint_info: everything about a blob that needs no handle. digests: recompute them (restore and merge always do).
static inline bool kajoCkptInfo(const void* blob, size_t bytes, KajoCheckpointInfo* out, std::string* why, bool digests = true)
{
    const unsigned char* b = static_cast<const unsigned char*>(blob);
    KajoCheckpointInfo info;
    memset(&info, 0, sizeof info);
    if (!blob || bytes < sizeof(KajoCheckpointHeader))
        return *why = "checkpoint: truncated inside the header", false;
    memcpy(&info.header, b, sizeof info.header);
    const KajoCheckpointHeader& h = info.header;
    if (memcmp(h.magic, kCkptMagic, 8) != 0)
        return *why = "checkpoint: bad magic, not a checkpoint section", false;
    if (h.version != KAJO_CKPT_VERSION)
        return *why = "checkpoint: version " + std::to_string(h.version) + " is not this library's (" + std::to_string(KAJO_CKPT_VERSION) + ")", false;
    if (h.nPlanes < 1 || h.nPlanes >= KAJO_CKPT_KINDS)
        return *why = "checkpoint: plane count out of range", false;
    if (bytes < sizeof(KajoCheckpointHeader) + (size_t)h.nPlanes * sizeof(KajoCheckpointPlane))
        return *why = "checkpoint: truncated inside the plane table", false;
    memcpy(info.planes, b + sizeof(KajoCheckpointHeader), (size_t)h.nPlanes * sizeof(KajoCheckpointPlane));
    if (h.width <= 0 || h.height <= 0 || (long long)h.width * h.height > (1ll << 31) - 1 || h.tileW < 8 || h.tileH < 8 || (h.tileW & 7) ||
        (h.tileH & 7) || ((long long)h.tileW * h.tileH) % 256 || h.tileCount < 1 || h.tileIndex < 0 || h.tileIndex >= h.tileCount ||
        h.passesDone < 0 || h.aovPasses < 0 || h.reserved != 0 || (h.noiseRebase != 0 && h.noiseRebase != 1))
        return *why = "checkpoint: header fields out of range", false;
    // (the cheap checks first: nothing is allocated or walked for a frame the blob cannot be of -- SUM alone is 16 bytes a pixel, and the
    // table of tile rows may take four times the blob and a MiB: an owner of a few pixels of a frame of millions of tile rows is refused)
    const KajoCkptGeom g = kajoCkptGeomOf(h);
    if (h.pixels > bytes / 16u)
        return *why = "checkpoint: plane SUM: truncated", false;
    if (((uint64_t)g.tilesY + 1) * 4u > 4u * (uint64_t)bytes + (1u << 20))
        return *why = "checkpoint: header fields out of range: more tile rows than a section of this size describes", false;
    if (kajoCkptPrefix(g, nullptr) != h.pixels)
        return *why = "checkpoint: the pixel count is not that of the owner's share of the frame", false;
    std::vector<uint32_t> prefix((size_t)g.tilesY + 1);
    kajoCkptPrefix(g, prefix.data());
    // the planes: ascending kinds from SUM, each of its kind's size, at the offsets of kajoCkptLayout
    KajoCheckpointPlane want[KAJO_CKPT_KINDS];
    for (uint32_t i = 0; i < h.nPlanes; i++) {
        const KajoCheckpointPlane& p = info.planes[i];
        const std::string name = std::string("checkpoint: plane ") + kajoCkptKindName(p.kind);
        if (p.kind < 1 || p.kind >= KAJO_CKPT_KINDS || (i == 0 ? p.kind != KAJO_CKPT_SUM : p.kind <= info.planes[i - 1].kind))
            return *why = "checkpoint: plane table entry " + std::to_string(i) + ": kinds ascend from SUM, each once", false;
        if (p.wordsPerPixel != kajoCkptKindWords(p.kind))
            return *why = name + ": wrong words per pixel", false;
        const bool sized = p.wordsPerPixel ? p.bytes == h.pixels * p.wordsPerPixel * 4u
                           : p.kind == KAJO_CKPT_COUNTERS ? p.bytes == 32u
                                                          : (p.bytes >= KAJO_CKPT_ADAPT_WORDS * 4u && p.bytes % 4u == 0 && p.bytes < (1ull << 32));
        if (!sized)
            return *why = name + ": wrong size", false;
        want[i] = p;
    }
    const uint64_t trailer = kajoCkptLayout(want, h.nPlanes);
    for (uint32_t i = 0; i < h.nPlanes; i++) {
        const std::string name = std::string("checkpoint: plane ") + kajoCkptKindName(info.planes[i].kind);
        if (info.planes[i].offset != want[i].offset)
            return *why = name + ": wrong offset", false;
        if (want[i].offset + want[i].bytes > bytes)
            return *why = name + ": truncated", false;
    }
    if (trailer + sizeof(KajoCheckpointTrailer) > bytes)
        return *why = "checkpoint: truncated inside the trailer", false;
    if (h.bytes != trailer + sizeof(KajoCheckpointTrailer) || bytes != h.bytes)
        return *why = "checkpoint: the section's size is not the one its header states", false;
    memcpy(&info.trailer, b + trailer, sizeof info.trailer);
    if (digests)
        for (uint32_t i = 0; i < h.nPlanes; i++) {
            const KajoCheckpointPlane& p = info.planes[i];
            // (the planes sit at multiples of 16 of a blob the caller may have put anywhere: through a copy that is aligned)
            std::vector<uint32_t> words((size_t)(p.bytes / 4));
            if (p.bytes)
                memcpy(words.data(), b + p.offset, (size_t)p.bytes);
            const uint64_t d = p.wordsPerPixel ? kajoCkptDigestHost(g, prefix.data(), words.data(), h.pixels, p.wordsPerPixel)
                                               : kajoCkptDigestWords(words.data(), words.size());
            if (d != p.digest)
                return *why = std::string("checkpoint: plane ") + kajoCkptKindName(p.kind) + ": the digest does not match the contents", false;
        }
    if (out)
        *out = info;
    return true;
}

static inline const KajoCheckpointPlane* kajoCkptFind(const KajoCheckpointInfo& info, uint32_t kind)
{
    for (uint32_t i = 0; i < info.header.nPlanes; i++)
        if (info.planes[i].kind == kind)
            return &info.planes[i];
    return nullptr;
}

// the kinds of a section as a bit set
static inline uint32_t kajoCkptKinds(const KajoCheckpointInfo& info)
{
    uint32_t set = 0;
    for (uint32_t i = 0; i < info.header.nPlanes; i++)
        set |= 1u << info.planes[i].kind;
    return set;
}

// A section written from a header (nPlanes, pixels, the scalars), the planes' kinds and sizes, and their contents: the layout, the
// digests where `digests` gives none, the trailer. contents[i]: the plane's bytes. The blob is resized to the section.
static inline void kajoCkptWrite(KajoCheckpointHeader h, KajoCheckpointPlane* planes, const void* const* contents, const uint64_t* digests,
                                 const KajoCheckpointTrailer& trailer, std::vector<unsigned char>& blob)
{
    const uint64_t end = kajoCkptLayout(planes, h.nPlanes);
    memcpy(h.magic, kCkptMagic, 8);
    h.version = KAJO_CKPT_VERSION;
    h.reserved = 0;
    h.bytes = end + sizeof trailer;
    blob.assign((size_t)h.bytes, 0);
    const KajoCkptGeom g = kajoCkptGeomOf(h);
    std::vector<uint32_t> prefix((size_t)g.tilesY + 1);
    kajoCkptPrefix(g, prefix.data());
    for (uint32_t i = 0; i < h.nPlanes; i++) {
        KajoCheckpointPlane& p = planes[i];
        if (p.bytes)
            memcpy(blob.data() + p.offset, contents[i], (size_t)p.bytes);
        if (digests)
            p.digest = digests[i];
        else {
            std::vector<uint32_t> words((size_t)(p.bytes / 4));
            if (p.bytes)
                memcpy(words.data(), contents[i], (size_t)p.bytes);
            p.digest = p.wordsPerPixel ? kajoCkptDigestHost(g, prefix.data(), words.data(), h.pixels, p.wordsPerPixel)
                                       : kajoCkptDigestWords(words.data(), words.size());
        }
    }
    memcpy(blob.data(), &h, sizeof h);
    memcpy(blob.data() + sizeof h, planes, (size_t)h.nPlanes * sizeof(KajoCheckpointPlane));
    memcpy(blob.data() + end, &trailer, sizeof trailer);
}

// kajo_hip_checkpoint_merge: the n sections of one frame's owners into one whole-frame section
static inline bool kajoCkptMerge(const void* const* blobs, const size_t* bytes, int n, std::vector<unsigned char>& out, std::string* why)
{
    if (!blobs || !bytes || n < 1)
        return *why = "checkpoint merge: no sections", false;
    std::vector<KajoCheckpointInfo> infos((size_t)n);
    for (int i = 0; i < n; i++)
        if (!kajoCkptInfo(blobs[i], bytes[i], &infos[(size_t)i], why)) {
            *why = "section " + std::to_string(i) + ": " + *why;
            return false;
        }
    const KajoCheckpointHeader& first = infos[0].header;
    if (first.tileCount != n)
        return *why = "checkpoint merge: the frame has " + std::to_string(first.tileCount) + " owners, " + std::to_string(n) + " sections were given", false;
    std::vector<int> at((size_t)n, -1); // the section of every tile index
    uint32_t kinds = 0;                 // the planes of an owner with pixels
    for (int i = 0; i < n; i++) {
        const KajoCheckpointHeader& h = infos[(size_t)i].header;
        if (h.fingerprint != first.fingerprint || h.width != first.width || h.height != first.height || h.samplesPerPass != first.samplesPerPass ||
            h.depthLimit != first.depthLimit || h.seed != first.seed || h.flags != first.flags)
            return *why = "checkpoint merge: section " + std::to_string(i) + " is of another scene or other parameters (fingerprint)", false;
        if (h.tileW != first.tileW || h.tileH != first.tileH || h.tileCount != first.tileCount)
            return *why = "checkpoint merge: section " + std::to_string(i) + " is of another tile layout", false;
        if (h.passesDone != first.passesDone || h.aovPasses != first.aovPasses || h.noiseRebase != first.noiseRebase)
            return *why = "checkpoint merge: section " + std::to_string(i) + " is of another pass count", false;
        if (at[(size_t)h.tileIndex] >= 0)
            return *why = "checkpoint merge: owner " + std::to_string(h.tileIndex) + " is there twice, another is missing: the sections do not cover the frame exactly",
                   false;
        at[(size_t)h.tileIndex] = i;
        if (kajoCkptKinds(infos[(size_t)i]) & (1u << KAJO_CKPT_ADAPT))
            return *why = "checkpoint merge: section " + std::to_string(i) + " has an ADAPT block: an adaptive session resumes in its own layout only", false;
        if (h.pixels)
            kinds |= kajoCkptKinds(infos[(size_t)i]);
    }
    if (!kinds)
        kinds = kajoCkptKinds(infos[0]);
    for (int i = 0; i < n; i++) {
        const uint32_t own = kajoCkptKinds(infos[(size_t)i]);
        // (an owner without a pixel renders nothing and never stands inside a group: it may lack CARRY)
        const uint32_t carry = 1u << KAJO_CKPT_CARRY;
        if ((own & (1u << KAJO_CKPT_COUNTERS)) != (kinds & (1u << KAJO_CKPT_COUNTERS)))
            return *why = "checkpoint merge: section " + std::to_string(i) + ": plane COUNTERS is kept by some owners only, the counters cannot be added", false;
        if (infos[(size_t)i].header.pixels ? own != kinds : (own & ~carry) != (kinds & ~carry))
            return *why = "checkpoint merge: section " + std::to_string(i) + " keeps other planes than the rest", false;
    }
    // the whole-frame section
    KajoCheckpointHeader h = first;
    h.tileIndex = 0;
    h.tileCount = 1;
    h.pixels = (uint64_t)first.width * (uint64_t)first.height;
    KajoCheckpointPlane planes[KAJO_CKPT_KINDS];
    std::vector<std::vector<uint32_t>> contents;
    uint64_t digests[KAJO_CKPT_KINDS];
    h.nPlanes = 0;
    for (uint32_t kind = 1; kind < KAJO_CKPT_KINDS; kind++) {
        if (!(kinds & (1u << kind)))
            continue;
        const uint32_t w = kajoCkptKindWords(kind);
        KajoCheckpointPlane& p = planes[h.nPlanes];
        memset(&p, 0, sizeof p);
        p.kind = kind;
        p.wordsPerPixel = w;
        p.bytes = w ? h.pixels * w * 4u : 32u;
        contents.emplace_back((size_t)(p.bytes / 4), 0u);
        std::vector<uint32_t>& dst = contents.back();
        uint64_t digest = 0;
        for (int i = 0; i < n; i++) {
            const KajoCheckpointInfo& info = infos[(size_t)i];
            const KajoCheckpointPlane* src = kajoCkptFind(info, kind);
            if (!src)
                continue;
            const unsigned char* from = static_cast<const unsigned char*>(blobs[i]) + src->offset;
            if (!w) { // COUNTERS: four 64-bit sums
                for (int c = 0; c < 4; c++) {
                    uint64_t a, b;
                    memcpy(&a, &dst[2 * (size_t)c], 8);
                    memcpy(&b, from + 8 * c, 8);
                    a += b;
                    memcpy(&dst[2 * (size_t)c], &a, 8);
                }
                continue;
            }
            digest += src->digest;
            const KajoCkptGeom g = kajoCkptGeomOf(info.header);
            std::vector<uint32_t> prefix((size_t)g.tilesY + 1);
            kajoCkptPrefix(g, prefix.data());
            for (uint64_t r = 0; r < info.header.pixels; r++) {
                int x, y;
                kajoCkptPixel(g, prefix.data(), (uint32_t)r, &x, &y);
                memcpy(&dst[((size_t)y * (size_t)h.width + (size_t)x) * w], from + r * w * 4u, (size_t)w * 4u);
            }
        }
        digests[h.nPlanes] = w ? digest : kajoCkptDigestWords(dst.data(), dst.size());
        h.nPlanes++;
    }
    KajoCheckpointTrailer trailer{0.0, 0};
    for (int i = 0; i < n; i++) {
        trailer.kernelMs += infos[(size_t)i].trailer.kernelMs;
        trailer.launches += infos[(size_t)i].trailer.launches;
    }
    const void* ptrs[KAJO_CKPT_KINDS];
    for (uint32_t i = 0; i < h.nPlanes; i++)
        ptrs[i] = contents[i].data();
    kajoCkptWrite(h, planes, ptrs, digests, trailer, out);
    // the sums of the sections' digests are the merged planes' own
    std::string inner;
    if (!kajoCkptInfo(out.data(), out.size(), nullptr, &inner))
        return *why = "checkpoint merge: the merged section does not pass its own check (" + inner + ")", false;
    return true;
}

#endif
