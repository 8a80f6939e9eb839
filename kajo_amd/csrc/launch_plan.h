// launch_plan.h -- what kajo_hip_create refuses and derives from a frame, how a handle uses the LDS, cuts its passes into launches and
// shapes them, as plain host arithmetic (capi.cpp kajo_hip_create / kajo_hip_render; tools/host_san.cpp and the programs inside
// tests/test_tiles_cpu.py and tests/test_adaptive_cpu.py run the same lines for the host-only tests). Static functions, no HIP: no symbols
// of libkajo_hip.so's.
#ifndef KAJO_LAUNCH_PLAN_H
#define KAJO_LAUNCH_PLAN_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "kajo_hip.h"

#include "adapt_math.h"
#include "render_args.h"
#include "stage.h"
#include "tuning.h"

constexpr int kMaxParts = 8; // workgroups a block of the launch tail is rendered in: one per group of a launch of 2 .. 8 groups

// numerics build a handle runs (include/kajo_hip.h)
enum class Numerics { Fast, Strict, Exact };

static inline Numerics kajoNumerics(uint32_t flags)
{
    return (flags & KAJO_FLAG_STRICT) ? Numerics::Strict : (flags & KAJO_FLAG_EXACT) ? Numerics::Exact : Numerics::Fast;
}

static inline int samplesPerAxis(const KajoParams& p)
{
    return (int)sqrt((double)(unsigned)p.samplesPerPass); // Renderer.cpp:38
}

// The parameter refusals of kajo_hip_create (KAJO_E_INVALID), which it issues before it looks for a device, in its order: the sentence of
// the first check that fails, or null. *p: the caller's parameters; the defaults are applied to it (tile 0 -> 64x16, tileCount 0 -> 1).
// msg: room for the one sentence that names what it found.
static inline const char* kajoCheckCreate(const KajoScene& scene, int width, int height, KajoParams* params, char (&msg)[256])
{
    KajoParams& p = *params;
    if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 31) - 1)
        return "image size out of range";
    if (scene.nPlanes < 0 || scene.nSpheres < 0 || (scene.nPlanes && !scene.planes) || (scene.nSpheres && !scene.spheres))
        return "scene arrays inconsistent";
    if (p.tileW == 0)
        p.tileW = 64;
    if (p.tileH == 0)
        p.tileH = 16;
    if (p.tileCount == 0)
        p.tileCount = 1;
    if (p.samplesPerPass < 1 || p.samplesPerPass > 65535)
        return "samplesPerPass must be in [1, 65535]";
    if ((p.flags & KAJO_FLAG_STRICT) && (p.flags & KAJO_FLAG_EXACT))
        return "the strict and the exact flag name two different numerics builds: set one";
    if (p.flags & KAJO_FLAG_COOP)
        return "KAJO_FLAG_COOP: the cooperative-traversal experiment is not built into this library (make -C kajo_amd/csrc experiments)";
    if (p.flags & KAJO_FLAG_DEFERRED)
        return "KAJO_FLAG_DEFERRED: the deferred-shading experiment is not built into this library (make -C kajo_amd/csrc experiments)";
    if (p.depthLimit < 0 || p.depthLimit > 1000) // (the reference's limit is 8)
        return "depthLimit must be in [0, 1000]";
    if (p.tileW < 8 || p.tileH < 8 || (p.tileW & 7) || (p.tileH & 7) || ((long long)p.tileW * p.tileH) % 256)
        return "tile size must be multiples of 8 with tileW*tileH a multiple of 256";
    if (p.tileCount < 1 || p.tileIndex < 0 || p.tileIndex >= p.tileCount)
        return "tileIndex/tileCount out of range";
    if ((p.flags & KAJO_FLAG_AOV) && !(p.flags & KAJO_FLAG_AOV_TILED) && p.tileCount != 1)
        return "first-hit AOVs need the whole frame on one handle (tileCount 1)";
    if ((p.flags & KAJO_FLAG_AOV_SPECULAR) && !(p.flags & KAJO_FLAG_AOV))
        return "the first-non-delta-hit flag changes what the AOV flag's buffers hold: set the AOV flag with it";
    if ((p.flags & KAJO_FLAG_AOV_MATTE) && !(p.flags & KAJO_FLAG_AOV))
        return "the matte flag keeps its coverage tables over the AOV flag's samples: set the AOV flag with it";
    if ((p.flags & KAJO_FLAG_AOV_TILED) && !(p.flags & KAJO_FLAG_AOV))
        return "the tiled flag changes where the AOV flag's sums are kept: set the AOV flag with it";
    if ((p.flags & KAJO_FLAG_ADAPTIVE) && !(p.flags & KAJO_FLAG_NOISE))
        return "the adaptive flag retires units by the noise flag's estimate: set the noise flag with it";
    // (aov.inc.hip: a wave of the tiled launch carries its block's corner and the tile's shape in 16-bit fields, in units of 8 pixels)
    if ((p.flags & KAJO_FLAG_AOV_TILED) && (width > 524288 || height > 262144 || p.tileW > 524280 || p.tileH > 524280))
        return "tiled AOVs: the frame must be within 524288 x 262144 and a tile within 524280 pixels a side";
    if (p.flags & (KAJO_FLAG_STRICT | KAJO_FLAG_EXACT)) {
        // integrator.inc.hip kdiv / ksqrt: the IEEE quotient and root without the compiler's range scaling are exact while operands stay
        // dozens of binades inside the float range, which a scene of ordinary coordinates guarantees; outside it STRICT would silently
        // stop being the oracle
        float lo = 0.f, hi = 0.f;
        kajo::coordinateRange(scene, &lo, &hi);
        if (!(hi == hi) || (hi > 0.f && (lo < 0x1p-40f || hi > 0x1p40f))) {
            snprintf(msg, sizeof msg, "strict / exact numerics need the scene's non-zero coordinates within 2^-40 .. 2^40 in magnitude "
                                      "(found %g .. %g): use the fast build or rescale the scene", (double)lo, (double)hi);
            return msg;
        }
    }
    return nullptr;
}

// What a scene puts in LDS (device_scene.h / integrator.inc.hip renderBody): hot records always, cold records in the small-scene kernels,
// the grid's header and -- if it fits -- its cell lists in the large-scene ones.
struct KajoSceneLds
{
    size_t hotBytes, coldBytes, gridHeaderBytes, gridBytes;
};

static inline KajoSceneLds kajoSceneLds(const kajo::StagedScene& st)
{
    const size_t nPlanes = (size_t)st.nPlanes, nSpheres = (size_t)st.nSpheres, nLights = st.light.size();
    KajoSceneLds s;
    // (integrator.inc.hip stageToLds: the 4-byte arrays are padded to a 16-byte boundary before the light records)
    s.hotBytes = nPlanes * 16 + st.sphereHot.size() * 16 + (((nPlanes + (st.allTranslated ? 0 : nSpheres) + nLights) * 4 + 15) & ~(size_t)15) +
                 nLights * (64 + 16) + (((nLights * nPlanes) * 4 + 15) & ~(size_t)15) + 8 * 16;
    s.coldBytes = nPlanes * 48 + nSpheres * 64 + (nPlanes + nSpheres) * sizeof(DMaterial);
    s.gridHeaderBytes = st.gridEnabled ? 5 * 16 : 0; // always in LDS (integrator.inc.hip gridWalk)
    s.gridBytes = st.gridEnabled ? ((st.gridCellStart.size() * sizeof(uint32_t) + st.gridItems.size() * sizeof(uint16_t)) + 15) & ~(size_t)15 : 0;
    return s;
}

// A handle's LDS budget per workgroup: the scene copy, and what every wave adds to it (render_args.h): the mailbox of taken-over passes.
struct KajoLdsPlan
{
    bool big = false;       // large scene: hot records (+ grid) in LDS, the rest in global memory
    bool coldInLds = false; // small scene: the whole scene in LDS
    bool gridInLds = false; // the grid's cell lists in LDS
    int stealWindow = 4;    // render_args.h; 1 when a large scene needs the LDS for its grid
    int ldsExtra = 0;       // (KAJO_TUNING builds only) unused bytes per wave, to study a launch at a lower occupancy
    int helpBytes = 0;      // list scenes: [64] owner lanes + [64] blocker flags of the cooperative list walk (integrator.inc.hip), behind the mailbox
    int accBytes = 0;       // FAST / EXACT, small scenes: [64] float4, the lanes' running totals behind the mailbox (integrator.inc.hip GROUPS)
    int thrL = 1, holdTrips = 1; // integrator.inc.hip MODE_HOLD
    size_t hotBytes = 0;    // what the big-scene staging (and the known-answer kernels) put in LDS
    size_t ldsBytes = 0;    // the scene copy of the render kernel
    unsigned wavesPerBlock = 1; // workgroup = 64 * wavesPerBlock threads: single-wave groups dispatch and retire
                                // independently (measured +2.3 % over 4-wave groups)
    bool fits = false;      // scene copy + the waves' areas fit a CU's 160 KiB

    size_t perWaveBytes(bool withMailbox) const
    {
        return (size_t)ldsExtra + (size_t)helpBytes + (withMailbox ? (size_t)64 * stealWindow * 16 + (size_t)accBytes : 0);
    }
    void fillWaveLds(RenderArgs& a, size_t perWaveOffset, bool withMailbox) const
    {
        a.perWaveOffset = (uint32_t)perWaveOffset;
        a.perWaveBytes = (uint32_t)perWaveBytes(withMailbox);
        a.thrL = thrL;
        a.holdTrips = holdTrips;
    }
    size_t mailboxOffset() const { return (ldsBytes + 15) & ~(size_t)15; }
    // scene copy + every wave's mailbox
    size_t ldsTotal() const { return mailboxOffset() + (size_t)wavesPerBlock * perWaveBytes(true); }
};

// The LDS budget of a scene (cold records in LDS while the total stays small enough for four workgroups per CU: 160 KiB / 4).
static inline KajoLdsPlan kajoLdsPlan(size_t hotBytes, size_t coldBytes, size_t gridHeaderBytes, size_t gridBytes, bool grid, bool shadowLists, int nLights,
                                      Numerics numerics)
{
    KajoLdsPlan p;
    // the oracle's arithmetic in everything that decides (STRICT and EXACT): which walk, which hold policy, whose resolve
    const bool strict = numerics != Numerics::Fast;
    p.big = grid || hotBytes + coldBytes > 40 * 1024;
    p.helpBytes = shadowLists ? 512 : 0;
    KAJO_TUNE_INT("KAJO_STEAL_WINDOW", 1, 16, p.stealWindow);
    KAJO_TUNE_INT("KAJO_LDS_EXTRA", 0, 64 * 1024, p.ldsExtra);
    p.ldsExtra &= ~15;
    // integrator.inc.hip MODE_HOLD: lanes that must want the light / BSDF blocks before they run without any lane having
    // waited a trip; 1 = every trip. Large scenes run them every trip (16 lights: most lanes are in them anyway).
    p.thrL = p.big ? 1 : (strict ? 28 : 20);
    if (!p.big && strict) {
        // the STRICT loop of small scenes with several lights walks its shadow rays inside the light loop (KAJO_INLINE_SHADOW): a heavier
        // block, worth waiting longer for (three lights: 11.6 -> 13.4 G paths/s at 48 lanes / three trips). One light (its own instance:
        // one visit per vertex, the shadow ray in a trip of its own): 20.5-20.7 at 32-44 lanes / two trips (profiles/r04_presample.txt).
        p.thrL = nLights > 1 ? 48 : 36;
        p.holdTrips = nLights > 1 ? 3 : 2;
    }
    if (shadowLists) {
        // Large scenes with visibility lists: the light loop runs to its end inside one trip (16 lights: ~10 rounds of light
        // sample + shadow query) and is the expensive block of a trip, with a third of the lanes in it. It runs when 60 lanes
        // have a vertex waiting or it has been put off six trips in a row; the walk loses lanes to the waiting (lane
        // efficiency 0.975 -> 0.64) -- lanes without a ray skip the grid walk, so that costs the walk nothing but the slots -- and
        // the launch gains: FAST 2.35 -> 4.34 G paths/s on the 1000-sphere scene at 4K x 32 passes with 48 lanes / three trips,
        // 5.38 -> 5.54 from there to 60 / six once the idle lanes stopped walking stale rays (profiles/r04_c5_notes.txt).
        p.thrL = 60;
        p.holdTrips = 6;
    }
    KAJO_TUNE_INT("KAJO_THR_L", 1, 65, p.thrL);
    KAJO_TUNE_INT("KAJO_HOLD_TRIPS", 1, 16, p.holdTrips);
    if (grid) {
        // The DDA reads a cell record and an item per step, each a dependent load: ~64 cycles from LDS, ~500 from L2. But the
        // walk is latency-bound and wants its workgroups per CU (measured on the 1000-sphere scene in round 2: the grid in LDS
        // at three workgroups per CU is 12 % SLOWER than the grid in L2 at four), so the grid moves into LDS only while hot
        // records + grid + the four waves' areas stay within the limit.
        int gridLimit = 40 * 1024;
        KAJO_TUNE_INT("KAJO_GRID_LDS_LIMIT", 0, 160 * 1024, gridLimit); // bytes
        // ... with the mailboxes shrunk to a one-pass steal window if need be
        const int wanted = p.stealWindow;
        for (int window : {4, 2, 1}) {
            if (window > wanted)
                continue;
            p.stealWindow = window;
            if (hotBytes + gridHeaderBytes + gridBytes + 4 * p.perWaveBytes(true) <= (size_t)gridLimit) {
                p.gridInLds = true;
                break;
            }
        }
        if (!p.gridInLds) {
            p.stealWindow = wanted;
            gridBytes = 0;
        }
    }
    p.hotBytes = hotBytes + gridHeaderBytes + gridBytes;
    p.coldInLds = !p.big;
    if (p.coldInLds && numerics != Numerics::Strict) {
        // (the lanes' running totals take the room of one pass of the mailbox: three passes to take over instead of four costs nothing,
        // tools/steal_window_sweep.sh, and the scene copy + a wave's area of BASELINE's scenes stays within a fifth wave per SIMD's share)
        p.accBytes = 64 * 16;
        p.stealWindow = 3;
        KAJO_TUNE_INT("KAJO_STEAL_WINDOW", 1, 16, p.stealWindow);
    }
    p.ldsBytes = hotBytes + (p.coldInLds ? coldBytes : 0) + gridHeaderBytes + gridBytes;
    // every workgroup stages its own LDS copy of the scene: single-wave groups only while that copy is small
    p.wavesPerBlock = p.ldsBytes <= 6 * 1024 ? 1 : 4;
    {
        int w = 0;
        KAJO_TUNE_INT("KAJO_WAVES_PER_BLOCK", 1, 4, w); // 1, 2 or 4
        if (w == 1 || w == 2 || w == 4)
            p.wavesPerBlock = (unsigned)w;
    }
    // the one check, with the final values: scene copy + the waves' areas must fit a CU
    p.fits = p.ldsTotal() <= 160 * 1024;
    return p;
}

static inline KajoLdsPlan kajoLdsPlan(const kajo::StagedScene& st, Numerics numerics)
{
    const KajoSceneLds b = kajoSceneLds(st);
    return kajoLdsPlan(b.hotBytes, b.coldBytes, b.gridHeaderBytes, b.gridBytes, st.gridEnabled, st.shadowEnabled, (int)st.light.size(), numerics);
}

// What kajo_hip_create derives from the frame, the parameters (defaults applied: kajoCheckCreate) and the scene's plan: the owner's share
// of the tiles, its launch grid, and what every launch of the handle has in common. 64-bit where a frame create accepts could overflow.
struct KajoFramePlan
{
    TileMap map{};
    int tilesY = 0, nTiles = 0, nTilesOwned = 0, tilesPerOwner = 0;
    size_t tileBytes = 0;              // float4 [map.slotsPerOwner]
    unsigned long long gridBlocks = 0; // workgroups of a whole launch (the units of adaptive sampling): the owner's pixel blocks / wavesPerBlock
    bool tooManyBlocks = false;        // ... 2^28 or more (render_args.h: an order word has 28 bits for the block): create refuses the frame
    unsigned long long pixelBlocks = 0; // the owner's 8x8 pixel blocks in whole launch blocks
    int n = 0;                         // samplesPerAxis
    bool grouped = false;              // integrator.inc.hip GROUPS: FAST / EXACT kernels of small scenes
    int home = 0;                      // launch.inc.hip: coldInLds, or 2: the small-scene instance of any number of lights although the scene
                                       // has one (KAJO_FLAG_NO_ONE_LIGHT)
    bool partsAllowed = false;         // FAST / EXACT handle of a small scene that orders its launches and may divide them (capi.cpp partTheTail)
    unsigned unitShift = 0;            // adaptive sampling: a unit is 1 << unitShift slots; 0: neither 64, 128 nor 256, create refuses the flag
    AdaptGeom adaptGeom{};
};

static inline KajoFramePlan kajoFramePlan(int W, int H, const KajoParams& p, const KajoLdsPlan& lds, Numerics numerics)
{
    KajoFramePlan f;
    TileMap& m = f.map;
    m.W = W;
    m.H = H;
    m.tileW = p.tileW;
    m.tileH = p.tileH;
    m.tilesX = (int32_t)(((long long)W + p.tileW - 1) / p.tileW);
    m.tileCount = p.tileCount;
    f.tilesY = (int)(((long long)H + p.tileH - 1) / p.tileH);
    f.nTiles = m.tilesX * f.tilesY;
    f.tilesPerOwner = (int)(((long long)f.nTiles + p.tileCount - 1) / p.tileCount);
    f.nTilesOwned = (int)(((long long)f.nTiles - p.tileIndex + p.tileCount - 1) / p.tileCount);
    if (f.nTilesOwned < 0)
        f.nTilesOwned = 0;
    m.slotsPerOwner = (int32_t)((long long)f.tilesPerOwner * p.tileW * p.tileH);
    f.tileBytes = (size_t)m.slotsPerOwner * 16;
    f.gridBlocks = (unsigned long long)f.nTilesOwned * (p.tileW / 8) * (p.tileH / 8) / lds.wavesPerBlock;
    f.tooManyBlocks = f.gridBlocks >= (1ull << 28);
    f.pixelBlocks = f.gridBlocks * lds.wavesPerBlock;
    f.n = samplesPerAxis(p);
    f.grouped = lds.coldInLds && numerics != Numerics::Strict;
    f.home = (lds.coldInLds && (p.flags & KAJO_FLAG_NO_ONE_LIGHT)) ? 2 : lds.coldInLds;
    f.partsAllowed = f.grouped && !(p.flags & (KAJO_FLAG_NO_SPLIT | KAJO_FLAG_NO_REORDER));
    f.unitShift = lds.wavesPerBlock == 1 ? 6 : lds.wavesPerBlock == 2 ? 7 : lds.wavesPerBlock == 4 ? 8 : 0;
    f.adaptGeom = AdaptGeom{W, H, p.tileW, p.tileH, m.tilesX, p.tileIndex, p.tileCount, f.nTilesOwned};
    return f;
}

// The passes of the next launch of kajo_hip_render with `left` to go: passesPerLaunch at the most (0: 16) and, on a handle with the noise
// flag, none across an absolute multiple of the batch (the frame's bits do not depend on the cut)
static inline int kajoLaunchPasses(int left, int passesPerLaunch, bool noise, int passesDone)
{
    const int perLaunch = passesPerLaunch > 0 ? passesPerLaunch : 16;
    int now = left < perLaunch ? left : perLaunch;
    if (noise && now > KAJO_NOISE_BATCH_PASSES - passesDone % KAJO_NOISE_BATCH_PASSES)
        now = KAJO_NOISE_BATCH_PASSES - passesDone % KAJO_NOISE_BATCH_PASSES;
    return now;
}

// The shape of one launch of kajo_hip_render: how it joins the groups of four passes, and how many waves share a pixel block.
struct KajoLaunchShape
{
    // (integrator.inc.hip GROUPS, FAST / EXACT kernels of small scenes: the total takes the passes in groups of four by their absolute
    // numbers. A launch that begins or ends inside a group hands the group over through `carry`: render_args.h)
    bool startsInside = false, endsInside = false;
    int launchGroups = 0; // whole groups, or 0
    unsigned split = 1;   // waves of a block that divide the passes of the launch
    unsigned chunks = 1;  // waves of a block per pass that divide its samples
    bool parted = false;  // the launch tail: the cheapest blocks as one workgroup per group of the launch (capi.cpp partTheTail)
};

// pixelBlocks: the handle's 8x8 pixel blocks; now: passes of this launch; n: samples per pass and axis; perWaveBytes: the plan's
// perWaveBytes(false); passesDone: the passes before this launch; grouped: a FAST / EXACT handle of a small scene.
static inline KajoLaunchShape kajoLaunchShape(unsigned long long pixelBlocks, int now, int n, bool coldInLds, bool noSplit, size_t mailboxOffset,
                                              size_t perWaveBytes, int passesDone, bool grouped, bool orderValid, unsigned nParted)
{
    KajoLaunchShape s;
    s.startsInside = grouped && passesDone % KAJO_GROUP_PASSES != 0;
    s.endsInside = grouped && (passesDone + now) % KAJO_GROUP_PASSES != 0;
    s.launchGroups = (!s.startsInside && !s.endsInside) ? now / KAJO_GROUP_PASSES : 0;
    // Small frames: fewer pixel blocks than a few rounds of the chip's 4096 wave slots. 2 or 4 waves then share a
    // block and divide the passes of the launch (when they divide evenly); the per-pass terms meet in LDS.
    if (coldInLds && !noSplit) {
        // measured (tools/size_sweep.py with KAJO_SPLIT=1..16, 256x144 ... 1920x1080): frames of fewer than three
        // rounds of the 4096 wave slots run best with the largest power of two -- up to 16 waves per block, as far
        // as the passes divide -- that keeps the launch within 8 rounds: many short waves pack the tail of the
        // launch better than few long ones. From 1280x720 on the unsplit kernel is 3-8 % faster.
        while (pixelBlocks < 3 * 4096 && s.split < 16 && now % (int)(s.split * 2) == 0 && pixelBlocks * s.split * 2 <= 8 * 4096)
            s.split *= 2;
        int v = 0;
        KAJO_TUNE_INT("KAJO_SPLIT", 1, 16, v);
        if (v >= 1 && (v & (v - 1)) == 0 && now % v == 0)
            s.split = (unsigned)v;
    }
    while (s.split > 1 && mailboxOffset + (size_t)now * 64 * 16 + s.split * perWaveBytes > 48 * 1024)
        s.split /= 2; // the table and the waves' areas would need the large-LDS opt-in: not worth it
    // Launches of FEW passes (BASELINE configs[0] is one pass of 16 samples on 1024 pixel blocks: a quarter of the chip's SIMDs,
    // one wave each): the waves of a block divide the SAMPLES of every pass instead -- `chunks` per pass, now * chunks waves
    // per block -- and the paths' radiances meet in the table [pass][sample][pixel]. Chosen when it puts more waves on a
    // block than dividing the passes does.
    if (coldInLds && !noSplit && pixelBlocks < 3 * 4096) {
        const unsigned nn = (unsigned)(n * n);
        // the smallest division that gives the launch one round of the chip's wave slots (measured on configs[0], 1024 blocks:
        // 4 chunks 18.0, 8 chunks 17.4, 16 chunks 15.5 G paths/s against 8.3 undivided; profiles/r03_configs.txt)
        for (unsigned q = 2; q <= nn && (unsigned)now * q <= 16; q++)
            if (nn % q == 0 && pixelBlocks * now * q <= 8 * 4096 && mailboxOffset + (size_t)now * nn * 64 * 16 + (size_t)now * q * perWaveBytes <= 48 * 1024) {
                s.chunks = q;
                if (pixelBlocks * now * q >= 4096)
                    break;
            }
        int v = 0;
        KAJO_TUNE_INT("KAJO_SAMPLE_CHUNKS", 1, 16, v); // (held to the same 48 KiB bound as the automatic choice, the waves' areas included)
        if (v >= 1 && nn % (unsigned)v == 0 && (unsigned)now * v <= 16 && mailboxOffset + (size_t)now * nn * 64 * 16 + (size_t)now * v * perWaveBytes <= 48 * 1024)
            s.chunks = (unsigned)v;
        if ((unsigned)now * s.chunks <= s.split)
            s.chunks = 1;
    }
    s.parted = s.chunks == 1 && s.split == 1 && grouped && orderValid && nParted && s.launchGroups >= 2 && s.launchGroups <= kMaxParts;
    return s;
}

// ... of a handle's launch of `now` passes behind passesDone
static inline KajoLaunchShape kajoLaunchShape(const KajoFramePlan& f, const KajoLdsPlan& lds, uint32_t flags, int now, int passesDone, bool orderValid,
                                              unsigned nParted)
{
    return kajoLaunchShape(f.pixelBlocks, now, f.n, lds.coldInLds, (flags & KAJO_FLAG_NO_SPLIT) != 0, lds.mailboxOffset(), lds.perWaveBytes(false),
                           passesDone, f.grouped, orderValid, nParted);
}

#endif
