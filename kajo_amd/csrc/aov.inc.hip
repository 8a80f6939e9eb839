// aov.inc.hip -- first-hit AOVs for denoisers (KAJO_FLAG_AOV, include/kajo_hip.h kajo_hip_read_aov), included by kernel_strict.hip and
// kernel_fast.hip behind integrator.inc.hip: the SAME device functions (stageToLds, trace, hitNormal) on the beauty render's own camera
// samples. The STRICT instance serves STRICT and EXACT handles: EXACT's camera rays, walk and normals are STRICT's arithmetic.
//
// Shape: one wave per 8x8 pixel block and one lane per pixel, as in the render kernels, so that a wave's camera rays stay coherent (the
// blocks of the whole frame, or with AovArgs::tiledBlocks those of the handle's own tiles: aovBody). A lane
// reads its pixel's two float4 sums, adds its samples one at a time -- pass order, then stratum sy * n + sx -- and writes them back: the
// sequential loop is what fixes the summation order, so the buffers do not depend on how the passes were cut into launches.
// Per sample: hit = id != 0; albedo = clamp((diffuse + specular) + transparency, 0, 1) of the hit object's material (the three lobe colours
// of Shader.cpp:129-131), the background colour on a miss (Shader.cpp:116-117); the world normal hitNormal gives (no flip), 0 on a miss;
// depth = the ray's maxDistance, 0 on a miss.
//
// FOLLOW (KAJO_FLAG_AOV_SPECULAR, the _spec instances): the sample is taken at the first NON-DELTA hit instead. While the hit's material
// would send the beauty path through a delta lobe more likely than not -- ideal transmission (pT >= 0.5) or the ideal reflector
// (exponent 0, pD < 0.5) -- the ray is continued in that lobe's one direction, exactly as the integrator forms its extension ray
// (transmissionDirection / reflect on the integrator's own hit point and normal, origin moved kEps along the new direction), at most
// KAJO_AOV_MAX_FOLLOW times. T, the product of the followed surfaces' clamped specular colours, scales the final albedo (or the
// background); the depth is the length of the whole chain. The definition is in include/kajo_hip.h; no random number is drawn.
//
// MATTE (KAJO_FLAG_AOV_MATTE, the _matte instances): beside the two sums a lane keeps its pixel's coverage table -- eight slots (id, count)
// in registers, read before the sample loop and written after it as A and B are -- and counts the id of the hit the sample is taken at
// (the final hit of the chain with FOLLOW) by the first-come rule of include/kajo_hip.h. Integers only: the same table in every build that
// walks to the same hits.
#define KAJO_AOV_MAX_FOLLOW 8
#define KAJO_AOV_CAT2(a, b) a##b
#define KAJO_AOV_CAT(a, b) KAJO_AOV_CAT2(a, b)

namespace
{

// The camera block of renderBody (integrator.inc.hip, MODE_NEW; Renderer.cpp:51-64), restated: the stream key of (pixel, stratum, pass),
// one generator step, the jittered point on the image plane and the normalised direction. Same operations on the same operands in the
// same order, so the same bits in the STRICT build (tests/test_hip_aov.py replays them against the oracle).
KDEV void aovCameraRay(const AovArgs& args, const LdsScene& lds, int spx, int spy, int sampleX, int sampleY, int pass, F3& O, F3& d)
{
    const float curPixX = spx * args.pixelWidth, curPixY = (args.H - spy) * args.pixelHeight;
    uint32_t a = (uint32_t)(spy * args.W + spx) ^ 0x61707865u, c = ((uint32_t)args.seed ^ 0x79622d32u) ^ ((uint32_t)pass >> 16),
             dd = (uint32_t)(args.seed >> 32) ^ 0x6b206574u;
    uint32_t b = ((uint32_t)(sampleY * args.n + sampleX) | ((uint32_t)pass << 16)) ^ 0x3320646eu;
    KAJO_QUARTER_ROUND(a, b, c, dd);
    KAJO_QUARTER_ROUND(a, b, c, dd);
    KAJO_QUARTER_ROUND(a, b, c, dd);
    Rng fresh;
    fresh.lo = (uint64_t)a | ((uint64_t)b << 32);
    fresh.hi = (uint64_t)c | ((uint64_t)dd << 32);
    rngStep(fresh);
    const float offX = unitBits((uint32_t)fresh.lo);
    const float offY = unitBits((uint32_t)(fresh.lo >> 32));
    const float sx = curPixX + sampleX * args.sampleWidth + offX * args.sampleWidth;
    const float sy = curPixY + sampleY * args.sampleHeight + offY * args.sampleHeight;
    const DFloat4 c0 = lds.camera[0], c1 = lds.camera[1], c2 = lds.camera[2], c3 = lds.camera[3];
    O = f3(c3.x, c3.y, c3.z);
    d = normalize(f3(c0.x, c0.y, c0.z) + f3(c1.x, c1.y, c1.z) * sx + f3(c2.x, c2.y, c2.z) * sy - O);
}

// One step of a camera sample's chain: if the hit's material is one the rule follows, moves the ray (O, d) on to the extension ray of
// its delta lobe, takes the surface's colour into T and its distance into D, and returns true. Per step one material is read: the
// coins and the exponent, and for a followed hit the specular colour + ior.
template <bool LISTS>
KDEV bool aovFollowStep(const DSceneView& sc, const LdsScene& lds, const Hit& h, F3& O, F3& d, F3& T, float& D)
{
    if (h.id == 0)
        return false;
    const DFloat4* mq = reinterpret_cast<const DFloat4*>(lds.material + (h.id - 1));
    const float pT = mq[0].y, pD = mq[0].z, exponent = mq[3].w;
    // (comparisons with a NaN coin are false: a material with no lobe at all is not followed)
    const bool transmit = pT >= 0.5f;
    if (!(transmit || (exponent == 0.0f && pD < 0.5f)))
        return false;
    const DFloat4 m2 = mq[2];
    const F3 N = hitNormal<LISTS>(sc, lds, h, O, d);
    const F3 nd = transmit ? transmissionDirection(d, N, m2.w) : reflect(d, N);
    if (nd.x == 0.0f && nd.y == 0.0f && nd.z == 0.0f)
        return false;
    // both delta lobes carry the SPECULAR colour (Shader.cpp:137-139)
    T = T * f3(fminf(fmaxf(m2.x, 0.0f), 1.0f), fminf(fmaxf(m2.y, 0.0f), 1.0f), fminf(fmaxf(m2.z, 0.0f), 1.0f));
    D = D + h.t;
    O = (O + d * h.t) + nd * kEps; // the hit point of Raytracer.cpp:134-135, the extension ray of Shader.cpp:197-198
    d = nd;
    return true;
}

// The chain behind the camera ray's hit `h`: returns the hit the sample is taken at and leaves the ray that found it in (O, d), the
// followed surfaces' colour in T and their distances in D. A wave's lanes run chains of different lengths, so this is ONE loop around
// ONE trace call: every lane still in a chain takes part in the trip, the others pass hasRay = false as lanes outside the frame do, and
// the wave leaves when no lane has a ray -- a wave that sees no mirror and no glass never enters it. The camera ray's own walk stays
// the caller's, in the first-hit kernels' form: FAST's contracted arithmetic depends on what the compiler knows about the ray (the
// camera origin is the same for every lane), and a scene without delta materials has to give the first-hit buffers bit for bit.
// The _biglist walks carry no general sphere record and no far-origin fallback because stage.cpp only builds visibility lists for a
// closed room of (centre, radius) spheres: a chain ray starts on a surface inside that room, like every extension ray of the integrator,
// so that guarantee covers it (tests/test_hip_aov_specular.py: the grid scenes with glass and mirror balls).
template <bool COLD_LDS, bool LISTS, int GHOME>
KDEV Hit aovFollow(const DSceneView& sc, const LdsScene& lds, Hit h, F3& O, F3& d, bool hasRay, F3& T, float& D)
{
    int follows = 0;
    bool chain = hasRay && aovFollowStep<LISTS>(sc, lds, h, O, d, T, D);
    while (__ballot(chain) != 0ull) { // (wave-uniform trip count: the longest chain among the wave's lanes)
        const Hit next = trace<!COLD_LDS, GHOME, LISTS>(sc, lds, O, d, chain);
        if (chain) {
            h = next;
            follows++;
            chain = follows < KAJO_AOV_MAX_FOLLOW && aovFollowStep<LISTS>(sc, lds, h, O, d, T, D);
        }
    }
    return h;
}

// One sample into a pixel's table: the slot that holds `id` counts it, else the first empty slot takes it with count 1, else it is
// dropped. Slots are only ever taken in order, so the filled ones are a prefix and one pass over the eight decides: a compare / select
// chain on named registers (an indexed array would live in scratch).
KDEV void matteSlot(uint32_t& slotId, uint32_t& slotCount, uint32_t id, bool& done)
{
    const bool take = !done && (slotCount == 0u || slotId == id);
    slotId = take ? id : slotId;
    slotCount += take ? 1u : 0u;
    done = done || take;
}

KDEV void matteAdd(uint4& i0, uint4& i1, uint4& c0, uint4& c1, uint32_t id)
{
    bool done = false;
    matteSlot(i0.x, c0.x, id, done);
    matteSlot(i0.y, c0.y, id, done);
    matteSlot(i0.z, c0.z, id, done);
    matteSlot(i0.w, c0.w, id, done);
    matteSlot(i1.x, c1.x, id, done);
    matteSlot(i1.y, c1.y, id, done);
    matteSlot(i1.z, c1.z, id, done);
    matteSlot(i1.w, c1.w, id, done);
}

// COLD_LDS, LISTS, GHOME: as renderBody's (the instance of the scene class; capi.cpp picks it at create). FOLLOW: the sample is taken at
// the end of aovFollow's chain instead of at the first hit. MATTE: the pixel's coverage table is kept beside the sums.
template <bool COLD_LDS, bool LISTS = false, int GHOME = 0, bool FOLLOW = false, bool MATTE = false>
KDEV void aovBody(const AovArgs& args, unsigned char* ldsRaw)
{
    const DSceneView& sc = args.scene;
    const int lane = threadIdx.x & 63;
    const int block = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6))); // (wave-uniform)
    // The wave's 8x8 pixel block and where its sums live. Whole-frame buffers: the blocks of the frame in row order, a pixel's sums at its
    // row-major index. TILED (KAJO_FLAG_AOV_TILED): the blocks of the handle's OWN tiles in the order of the accumulation's tile buffer
    // (integrator.inc.hip: owned tile, then wave block inside the tile), a pixel's sums at kajoTileSlot's slot = block * 64 + lane -- a wave's
    // 64 float4 are contiguous. The arithmetic is the wave's, not the lane's: it stays in scalar registers.
    // The tiled shape is worked out IN FRONT of the scene's staging and leaves ONE scalar register behind, `where`: the block's corner in
    // units of 8 pixels, x | y << 16 (capi.cpp bounds the frame of a tiled handle accordingly), -1 = whole-frame buffers, -2 = a wave beyond
    // the owner's blocks. The large-scene instances have no scalar register to spare while they stage, and none was to be added to them.
    int where = -1;
    if (args.tiledBlocks) {
        where = -2;
        if (block < args.tiledBlocks) {
            const int wavesX = (int)(args.tileWaves & 0xffffu), wavesY = (int)(args.tileWaves >> 16), wavesPerTile = wavesX * wavesY;
            const int tilesX = (args.W + wavesX * 8 - 1) / (wavesX * 8);
            const int ownedTile = block / wavesPerTile, wb = block - ownedTile * wavesPerTile;
            const int tile = args.tileIndex + ownedTile * args.tileCount;
            const int ty = tile / tilesX, by = wb / wavesX;
            where = ((tile - ty * tilesX) * wavesX + (wb - by * wavesX)) | ((ty * wavesY + by) << 16);
        }
    }
    where = __builtin_amdgcn_readfirstlane(where);
    const LdsScene lds = stageToLds<COLD_LDS>(sc, ldsRaw);
    // (the grid's last workgroup may have waves beyond the blocks: they leave here, past the last barrier)
    const bool tiled = where >= 0;
    const int blocksX = (args.W + 7) >> 3;
    if (tiled ? false : where == -2 || block >= blocksX * ((args.H + 7) >> 3))
        return;
    const int x0 = tiled ? (where & 0xffff) * 8 : (block % blocksX) * 8;
    const int y0 = tiled ? (where >> 16) * 8 : (block / blocksX) * 8;
    const int px = x0 + (lane & 7), py = y0 + (lane >> 3);
    const bool inImage = px < args.W && py < args.H;
    // (x0 and y0 are multiples of 8: the pixel's low bits are its lane)
    const size_t at = !inImage ? 0 : tiled ? (size_t)block * 64 + (size_t)(((py & 7) << 3) | (px & 7)) : (size_t)py * args.W + px;
    float4* const albedoHits = static_cast<float4*>(args.albedoHits);
    float4* const normalDepth = albedoHits + args.slots;
    float4 A = make_float4(0.0f, 0.0f, 0.0f, 0.0f), B = A;
    if (inImage) {
        A = albedoHits[at];
        B = normalDepth[at];
    }
    uint4* const matteIds = static_cast<uint4*>(args.matteIds);
    uint4* const matteCounts = matteIds + 2 * (size_t)args.slots;
    uint4 i0 = make_uint4(0u, 0u, 0u, 0u), i1 = i0, c0 = i0, c1 = i0;
    if (MATTE && inImage) {
        i0 = matteIds[2 * at];
        i1 = matteIds[2 * at + 1];
        c0 = matteCounts[2 * at];
        c1 = matteCounts[2 * at + 1];
    }
    const F3 bg = f3(sc.background[0], sc.background[1], sc.background[2]);
    const int n = args.n, endPass = args.firstPass + args.nPasses;
    for (int pass = args.firstPass; pass < endPass; pass++) {
        for (int sampleY = 0; sampleY < n; sampleY++) {
            for (int sampleX = 0; sampleX < n; sampleX++) {
                F3 O, d;
                aovCameraRay(args, lds, px, py, sampleX, sampleY, pass, O, d);
                F3 T = f3(1.0f, 1.0f, 1.0f);
                float D = 0.0f;
                // (lanes outside the frame trace nothing through the grid; their sums are never written)
                Hit h = trace<!COLD_LDS, GHOME, LISTS>(sc, lds, O, d, inImage);
                if (FOLLOW)
                    h = aovFollow<COLD_LDS, LISTS, GHOME>(sc, lds, h, O, d, inImage, T, D);
                F3 albedo = bg, N = f3(0.0f, 0.0f, 0.0f);
                float depth = 0.0f, hit = 0.0f;
                if (h.id != 0) {
                    const DMaterial& m = lds.material[h.id - 1];
                    const float r = (m.diffuse[0] + m.specular[0]) + m.transparency[0];
                    const float g = (m.diffuse[1] + m.specular[1]) + m.transparency[1];
                    const float bl = (m.diffuse[2] + m.specular[2]) + m.transparency[2];
                    albedo = f3(fminf(fmaxf(r, 0.0f), 1.0f), fminf(fmaxf(g, 0.0f), 1.0f), fminf(fmaxf(bl, 0.0f), 1.0f));
                    N = hitNormal<LISTS>(sc, lds, h, O, d);
                    depth = h.t;
                    hit = 1.0f;
                }
                if (FOLLOW) { // (without a follow T = 1 and D = 0: the same bits as the first-hit sample)
                    albedo = T * albedo;
                    depth = h.id != 0 ? D + depth : 0.0f;
                }
                // (a miss adds zeros: every sample is one addition per word, as the definition sums them)
                A.x += albedo.x;
                A.y += albedo.y;
                A.z += albedo.z;
                A.w += hit;
                B.x += N.x;
                B.y += N.y;
                B.z += N.z;
                B.w += depth;
                if (MATTE)
                    matteAdd(i0, i1, c0, c1, (uint32_t)h.id);
            }
        }
    }
    if (inImage) {
        albedoHits[at] = A;
        normalDepth[at] = B;
    }
    if (MATTE && inImage) {
        matteIds[2 * at] = i0;
        matteIds[2 * at + 1] = i1;
        matteCounts[2 * at] = c0;
        matteCounts[2 * at + 1] = c1;
    }
}

} // namespace

// whole scene in LDS
extern "C" __global__ void __launch_bounds__(256) KAJO_AOV_NAME(const AovArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    aovBody<true>(args, ldsRaw);
}

// hot records in LDS, cold ones in global memory: an instance per home of the grid's cell lists (LDS: _lg), as the render kernels
extern "C" __global__ void __launch_bounds__(256) KAJO_AOV_CAT(KAJO_AOV_NAME, _big)(const AovArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    aovBody<false, false, 2>(args, ldsRaw);
}

extern "C" __global__ void __launch_bounds__(256) KAJO_AOV_CAT(KAJO_AOV_NAME, _big_lg)(const AovArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    aovBody<false, false, 1>(args, ldsRaw);
}

// scenes with visibility lists: the walk of a closed room of (centre, radius) spheres, nothing else compiled in
extern "C" __global__ void __launch_bounds__(256) KAJO_AOV_CAT(KAJO_AOV_NAME, _biglist)(const AovArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    aovBody<false, true, 2>(args, ldsRaw);
}

extern "C" __global__ void __launch_bounds__(256) KAJO_AOV_CAT(KAJO_AOV_NAME, _biglist_lg)(const AovArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    aovBody<false, true, 1>(args, ldsRaw);
}

// The same five with the chain of KAJO_FLAG_AOV_SPECULAR
#define KAJO_AOV_SPEC_KERNEL(suffix, ...)                                                                              \
    extern "C" __global__ void __launch_bounds__(256) KAJO_AOV_CAT(KAJO_AOV_NAME, suffix)(const AovArgs args)           \
    {                                                                                                                  \
        extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];                                         \
        aovBody<__VA_ARGS__, true>(args, ldsRaw);                                                                      \
    }
KAJO_AOV_SPEC_KERNEL(_spec, true, false, 0)
KAJO_AOV_SPEC_KERNEL(_spec_big, false, false, 2)
KAJO_AOV_SPEC_KERNEL(_spec_big_lg, false, false, 1)
KAJO_AOV_SPEC_KERNEL(_spec_biglist, false, true, 2)
KAJO_AOV_SPEC_KERNEL(_spec_biglist_lg, false, true, 1)

// The ten again with the coverage tables of KAJO_FLAG_AOV_MATTE (COLD_LDS, LISTS, GHOME, FOLLOW as above)
#define KAJO_AOV_MATTE_KERNEL(suffix, ...)                                                                             \
    extern "C" __global__ void __launch_bounds__(256) KAJO_AOV_CAT(KAJO_AOV_NAME, suffix)(const AovArgs args)           \
    {                                                                                                                  \
        extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];                                         \
        aovBody<__VA_ARGS__, true>(args, ldsRaw);                                                                      \
    }
KAJO_AOV_MATTE_KERNEL(_matte, true, false, 0, false)
KAJO_AOV_MATTE_KERNEL(_matte_big, false, false, 2, false)
KAJO_AOV_MATTE_KERNEL(_matte_big_lg, false, false, 1, false)
KAJO_AOV_MATTE_KERNEL(_matte_biglist, false, true, 2, false)
KAJO_AOV_MATTE_KERNEL(_matte_biglist_lg, false, true, 1, false)
KAJO_AOV_MATTE_KERNEL(_spec_matte, true, false, 0, true)
KAJO_AOV_MATTE_KERNEL(_spec_matte_big, false, false, 2, true)
KAJO_AOV_MATTE_KERNEL(_spec_matte_big_lg, false, false, 1, true)
KAJO_AOV_MATTE_KERNEL(_spec_matte_biglist, false, true, 2, true)
KAJO_AOV_MATTE_KERNEL(_spec_matte_biglist_lg, false, true, 1, true)

// (instance, kernel suffix) of the matte instances, in KajoAovInstance's order
#define KAJO_AOV_MATTE_INSTANCES(X)                                                                                    \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_SMALL, _matte)                                                                   \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_BIG, _matte_big)                                                                 \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_BIG_LG, _matte_big_lg)                                                           \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_BIGLIST, _matte_biglist)                                                         \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_BIGLIST_LG, _matte_biglist_lg)                                                   \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_SPEC_SMALL, _spec_matte)                                                         \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_SPEC_BIG, _spec_matte_big)                                                       \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_SPEC_BIG_LG, _spec_matte_big_lg)                                                 \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_SPEC_BIGLIST, _spec_matte_biglist)                                               \
    X(KAJO_AOV_MATTE_SMALL + KAJO_AOV_SPEC_BIGLIST_LG, _spec_matte_biglist_lg)

namespace
{
const void* aovKernel(int instance)
{
    switch (instance) {
    case KAJO_AOV_BIG: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _big));
    case KAJO_AOV_BIG_LG: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _big_lg));
    case KAJO_AOV_BIGLIST: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _biglist));
    case KAJO_AOV_BIGLIST_LG: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _biglist_lg));
    case KAJO_AOV_SPEC_SMALL: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec));
    case KAJO_AOV_SPEC_BIG: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec_big));
    case KAJO_AOV_SPEC_BIG_LG: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec_big_lg));
    case KAJO_AOV_SPEC_BIGLIST: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec_biglist));
    case KAJO_AOV_SPEC_BIGLIST_LG: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec_biglist_lg));
#define KAJO_AOV_MATTE_CASE(instance, suffix) case instance: return reinterpret_cast<const void*>(KAJO_AOV_CAT(KAJO_AOV_NAME, suffix));
    KAJO_AOV_MATTE_INSTANCES(KAJO_AOV_MATTE_CASE)
#undef KAJO_AOV_MATTE_CASE
    default: return reinterpret_cast<const void*>(KAJO_AOV_NAME);
    }
}
} // namespace

// 256 threads = four pixel blocks per workgroup; `grid` = ceil(blocks / 4). ldsBytes: the scene copy of the instance.
extern "C" int KAJO_AOV_CAT(KAJO_AOV_NAME, _launch)(const AovArgs* args, int instance, unsigned grid, size_t ldsBytes, void* stream)
{
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (instance) {
    case KAJO_AOV_BIG: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _big), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    case KAJO_AOV_BIG_LG: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _big_lg), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    case KAJO_AOV_BIGLIST: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _biglist), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    case KAJO_AOV_BIGLIST_LG: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _biglist_lg), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    case KAJO_AOV_SPEC_SMALL: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    case KAJO_AOV_SPEC_BIG: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec_big), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    case KAJO_AOV_SPEC_BIG_LG: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec_big_lg), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    case KAJO_AOV_SPEC_BIGLIST: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec_biglist), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    case KAJO_AOV_SPEC_BIGLIST_LG: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, _spec_biglist_lg), dim3(grid), dim3(256), ldsBytes, st, *args); break;
#define KAJO_AOV_MATTE_CASE(instance, suffix) case instance: hipLaunchKernelGGL(KAJO_AOV_CAT(KAJO_AOV_NAME, suffix), dim3(grid), dim3(256), ldsBytes, st, *args); break;
    KAJO_AOV_MATTE_INSTANCES(KAJO_AOV_MATTE_CASE)
#undef KAJO_AOV_MATTE_CASE
    default: hipLaunchKernelGGL(KAJO_AOV_NAME, dim3(grid), dim3(256), ldsBytes, st, *args); break;
    }
    return (int)hipGetLastError();
}

// Dynamic LDS above the default: the opt-in per function and device, only ever raised (see the render kernels' _set_lds, launch.inc.hip).
extern "C" int KAJO_AOV_CAT(KAJO_AOV_NAME, _set_lds)(int instance, size_t ldsBytes)
{
    static size_t highWaterOfDevice[64][KAJO_AOV_INSTANCES] = {};
    static std::mutex guard;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess)
        return (int)e;
    if (device < 0 || device >= 64 || instance < 0 || instance >= KAJO_AOV_INSTANCES)
        return (int)hipErrorInvalidValue;
    std::lock_guard<std::mutex> lock(guard);
    size_t& highWater = highWaterOfDevice[device][instance];
    if (ldsBytes <= highWater)
        return (int)hipSuccess;
    e = hipFuncSetAttribute(aovKernel(instance), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    if (e == hipSuccess)
        highWater = ldsBytes;
    return (int)e;
}
