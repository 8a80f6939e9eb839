// Sanitizer harness (CPU only; tests/test_sanitize_cpu.py, tools/stage_sanitize.sh): the host-side index arithmetic of the product, compiled
// from the product's own sources with -fsanitize=address,undefined.
//   host_san stage  a.pod ...            kajo_amd/csrc/stage.cpp: object records, uniform grid, per-light visibility lists, coordinate range
//   host_san parse  aspect a.json ...    kajo_amd/host/scene/SceneLoader.cpp on scene files (and on every prefix of each: truncated input)
//   host_san order  in.bin out.bin       kajo_amd/csrc/launch_order.h: cost order + parted tail from a trip table; side-buffer slots checked
//   host_san tiles  W H tileW tileH owners   render_args.h kajoTileSlot over a whole frame: every slot in range, none taken twice
//   host_san plan lds a.pod ...          kajo_amd/csrc/launch_plan.h kajoLdsPlan: a scene's LDS plan per staging (plain, no grid, no
//                                        visibility lists) and numerics build
//   host_san plan shape in.bin out.bin   launch_plan.h kajoLaunchShape over a table of launches
//   host_san plan shape a.pod W H tileW tileH S fast|strict|exact flags tileIndex tileCount now passesDone [now passesDone ...]
//                                        the plan and the launch shapes of a handle of that scene, frame, S, build and flags
//                                        (tests/test_launch_shapes_cpu.py): kajoCheckCreate, kajoLdsPlan, kajoFramePlan and kajoLaunchShape,
//                                        the functions create / render call
//   host_san plan cuts passesPerLaunch noise passesDone call [call ...]
//                                        launch_plan.h kajoLaunchPasses: "now passesDone" of every launch kajo_hip_render cuts the calls into
//   host_san plan sizes a.pod ...        what a scene's size does to its staging (tests/test_scene_sizes_cpu.py): the plan's ldsTotal() per
//                                        numerics build, the grid's cells per axis against the cells it wanted, the visibility lists' bins
//                                        and their longest row of 16-bit offsets; and the staged scene's allTranslated, planesRigid and
//                                        roomClosed beside nLights (tests/test_one_light_routing_cpu.py: which small-scene kernel it runs)
//   host_san plan kernel a.pod ...       the render kernel an EXACT handle of the scene launches, by name: launch.inc.hip's choice with
//                                        fixed_counts.h's table (tests/test_fixed_kernel_cpu.py, tests/test_hip_fixed_instance.py)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kajo_hip.h"
#include "kajo_scene.h"
#include "fixed_counts.h"
#include "launch_order.h"
#include "launch_plan.h"
#include "render_args.h"
#include "scene/Scene.h"
#include "stage.h"

// a scene written by kajo_amd/scene.py Scene.write_pod; 0 or the error code
struct Pod
{
    KajoScene sc{};
    std::vector<KajoSphere> sp;
    std::vector<KajoPlane> pl;
    int read(const char* path)
    {
        FILE* f = fopen(path, "rb");
        if (!f) return 2;
        int32_t n[2];
        if (fread(n, 4, 2, f) != 2) return 3;
        sp.resize(n[0]);
        pl.resize(n[1]);
        if (fread(sc.backgroundColor, 4, 4, f) != 4 || fread(&sc.camera, 4, 32, f) != 32) return 4;
        if (n[0] && fread(sp.data(), sizeof(KajoSphere), n[0], f) != (size_t)n[0]) return 5;
        if (n[1] && fread(pl.data(), sizeof(KajoPlane), n[1], f) != (size_t)n[1]) return 6;
        fclose(f);
        sc.nSpheres = n[0]; sc.nPlanes = n[1]; sc.spheres = sp.data(); sc.planes = pl.data();
        return 0;
    }
};

static int stage(int argc, char** argv)
{
    for (int a = 0; a < argc; a++) {
        Pod pod;
        if (int rc = pod.read(argv[a])) return rc;
        const KajoScene& sc = pod.sc;
        const int n[2] = {sc.nSpheres, sc.nPlanes};
        float lo, hi;
        kajo::coordinateRange(sc, &lo, &hi);
        for (int lists = 0; lists < 2; lists++) {
            kajo::StagedScene out;
            kajo::stageScene(sc, out, 48, lists != 0);
            printf("%s: %d spheres %d planes, lists %d, coordinates %g .. %g: ok\n", argv[a], n[0], n[1], lists, lo, hi);
        }
    }
    return 0;
}

static int parse(int argc, char** argv)
{
    if (argc < 2) return 2;
    const float aspect = (float)atof(argv[0]);
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 3;
        std::string text;
        char buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0)
            text.append(buf, got);
        fclose(f);
        scene::Scene s;
        if (!scene::Parser::loadFromString(s, text, aspect)) return 4;
        printf("%s: %zu spheres %zu planes\n", argv[a], s.spheres.size(), s.planes.size());
        // truncated input: the reader must fail or succeed, never read past the end (every prefix, in steps of 7 bytes)
        size_t accepted = 0;
        for (size_t cut = 0; cut < text.size(); cut += 7) {
            scene::Scene t;
            std::string part(text.data(), cut); // (a fresh, exactly sized buffer: an overread is an ASan error)
            accepted += scene::Parser::loadFromString(t, part, aspect) ? 1 : 0;
        }
        printf("%s: %zu of its prefixes parse\n", argv[a], accepted);
    }
    return 0;
}

static int order(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[0], "rb");
    if (!f) return 3;
    uint32_t head[5]; // nBlocks, wavesPerBlock, waveSlots, parts, threads
    if (fread(head, 4, 5, f) != 5) return 4;
    std::vector<uint32_t> trips((size_t)head[0] * head[1]);
    if (!trips.empty() && fread(trips.data(), 4, trips.size(), f) != trips.size()) return 5;
    fclose(f);
    std::vector<uint32_t> cost, plain, out;
    kajoBlockCosts(trips.data(), head[0], head[1], cost);
    kajoCostOrder(cost, plain);
    const unsigned nParted = kajoTailBlocks(head[0], head[2] / head[1]);
    const uint32_t parts = head[3], threads = head[4];
    if (parts >= 2 && nParted)
        kajoPartedOrder(plain, nParted, (int)parts, out);
    else
        out = plain;
    // side-buffer slots of the later parts' workgroups (render_args.h kajoSideSlot): in range, none taken twice
    if (parts >= 2 && nParted) {
        const uint32_t sideStride = nParted * threads, partedFirst = head[0] - nParted;
        std::vector<unsigned char> taken((size_t)(parts - 1) * sideStride, 0);
        for (size_t i = 0; i < out.size(); i++) {
            const uint32_t w = out[i];
            if (!(w & KAJO_ORDER_PARTED)) continue;
            if (i < partedFirst) return 6;
            const uint32_t part = (w >> KAJO_ORDER_PART_SHIFT) & 7u;
            if (part == 0) continue;
            for (uint32_t t = 0; t < threads; t += threads - 1 ? threads - 1 : 1) { // first and last thread of the workgroup
                const uint32_t s = kajoSideSlot((uint32_t)i, partedFirst, parts, part, sideStride, threads, t);
                if (s >= taken.size() || taken[s]) return 7;
                taken[s] = 1;
            }
        }
    }
    f = fopen(argv[1], "wb");
    if (!f) return 8;
    const uint32_t tail[2] = {nParted, (uint32_t)out.size()};
    fwrite(tail, 4, 2, f);
    if (!out.empty())
        fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}

static int tiles(int argc, char** argv)
{
    if (argc != 5) return 2;
    KajoParams p{};
    p.tileW = atoi(argv[2]); p.tileH = atoi(argv[3]); p.tileCount = atoi(argv[4]);
    const TileMap m = kajoFramePlan(atoi(argv[0]), atoi(argv[1]), p, KajoLdsPlan(), Numerics::Fast).map; // (the map as kajo_hip_create fills it)
    std::vector<unsigned char> taken((size_t)m.tileCount * m.slotsPerOwner, 0);
    for (int y = 0; y < m.H; y++)
        for (int x = 0; x < m.W; x++) {
            int owner;
            uint32_t slot;
            kajoTileSlot(m, x, y, &owner, &slot);
            if (owner < 0 || owner >= m.tileCount || slot >= (uint32_t)m.slotsPerOwner) return 3;
            unsigned char& t = taken[(size_t)owner * m.slotsPerOwner + slot];
            if (t) return 4;
            t = 1;
        }
    printf("%d x %d, tiles %d x %d, %d owners: %d slots per owner, ok\n", m.W, m.H, m.tileW, m.tileH, m.tileCount, m.slotsPerOwner);
    return 0;
}

// LDS plan of each scene file: one line per staging and numerics build, "<file> <staging> <numerics>: field=value ..."
static int planLds(int argc, char** argv)
{
    for (int a = 0; a < argc; a++) {
        Pod pod;
        if (int rc = pod.read(argv[a])) return rc;
        for (const char* staging : {"plain", "no_grid", "no_shadow_lists"}) {
            const bool grid = strcmp(staging, "no_grid") != 0, lists = strcmp(staging, "no_shadow_lists") != 0;
            kajo::StagedScene st;
            kajo::stageScene(pod.sc, st, grid ? 48 : 0, lists); // (as kajo_hip_create stages with KAJO_FLAG_NO_GRID / NO_SHADOW_LISTS)
            for (Numerics k : {Numerics::Fast, Numerics::Strict, Numerics::Exact}) {
                const KajoLdsPlan p = kajoLdsPlan(st, k);
                printf("%s %s %s: big=%d coldInLds=%d gridInLds=%d stealWindow=%d helpBytes=%d accBytes=%d thrL=%d holdTrips=%d hotBytes=%zu "
                       "ldsBytes=%zu wavesPerBlock=%u fits=%d\n",
                       argv[a], staging, k == Numerics::Fast ? "fast" : k == Numerics::Strict ? "strict" : "exact", p.big, p.coldInLds, p.gridInLds,
                       p.stealWindow, p.helpBytes, p.accBytes, p.thrL, p.holdTrips, p.hotBytes, p.ldsBytes, p.wavesPerBlock, p.fits);
            }
        }
    }
    return 0;
}

// Size facts of each scene file as kajo_hip_create stages it without flags: one line "<file>: field=value ...". gridWant*: the cells
// per axis stage.cpp buildGrid asks for before its clamp to 128 (ext / side, restated from the staged bounds); shadowMaxRow: the most items
// in one row of bins, which is the largest value a row's 16-bit offsets hold (shadowMaxOff16: read back from them).
static int planSizes(int argc, char** argv)
{
    for (int a = 0; a < argc; a++) {
        Pod pod;
        if (int rc = pod.read(argv[a])) return rc;
        kajo::StagedScene st;
        kajo::stageScene(pod.sc, st, 48, true);
        printf("%s: nSpheres=%d nLights=%zu grid=%d lists=%d", argv[a], st.nSpheres, st.light.size(), st.gridEnabled, st.shadowEnabled);
        // (what launch.inc.hip's choice among the small-scene kernels reads: tests/test_one_light_routing_cpu.py)
        printf(" allTranslated=%d planesRigid=%d roomClosed=%d", st.allTranslated, st.planesRigid, st.roomClosed ? 1 : 0);
        for (Numerics k : {Numerics::Fast, Numerics::Strict, Numerics::Exact}) {
            const KajoLdsPlan p = kajoLdsPlan(st, k);
            const char* name = k == Numerics::Fast ? "Fast" : k == Numerics::Strict ? "Strict" : "Exact";
            printf(" ldsTotal%s=%zu fits%s=%d", name, p.ldsTotal(), name, p.fits);
        }
        if (st.gridEnabled) {
            double ext[3], vol = 1;
            for (int k = 0; k < 3; k++) {
                ext[k] = std::fmax((double)st.gridMax[k] - st.gridMin[k], 1e-3);
                vol *= ext[k];
            }
            const double side = std::cbrt(vol / st.nSpheres);
            uint32_t longest = 0;
            for (size_t c = 0; c + 1 < st.gridCellStart.size(); c++)
                longest = std::max(longest, st.gridCellStart[c + 1] - st.gridCellStart[c]);
            const char axis[3] = {'X', 'Y', 'Z'};
            for (int k = 0; k < 3; k++)
                printf(" gridDim%c=%d gridWant%c=%d", axis[k], st.gridDim[k], axis[k], (int)std::ceil(ext[k] / side));
            printf(" gridItems=%zu gridMaxCell=%u", st.gridItems.size(), longest);
        }
        if (st.shadowEnabled || st.shadowN) { // (shadowN without lists: built, then dropped for a row beyond 16 bits)
            const size_t N = (size_t)st.shadowN, rows = st.light.size() * 6 * N;
            uint32_t maxRow = 0, maxOff = 0;
            for (size_t row = 0; row < rows; row++)
                maxRow = std::max(maxRow, st.shadowStart[(row + 1) * N] - st.shadowStart[row * N]);
            for (uint16_t o : st.shadowOff16)
                maxOff = std::max(maxOff, (uint32_t)o);
            printf(" shadowN=%d shadowItems=%zu shadowMaxRow=%u shadowMaxOff16=%u", st.shadowN, st.shadowItems.size(), maxRow, maxOff);
        }
        printf("\n");
    }
    return 0;
}

// Launch shapes: in.bin holds records of 11 uint32 (pixelBlocks, now, n, coldInLds, noSplit, mailboxOffset, perWaveBytes, passesDone,
// grouped, orderValid, nParted); out.bin gets 6 per record (startsInside, endsInside, launchGroups, split, chunks, parted).
static int planShape(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[0], "rb");
    if (!f) return 3;
    std::vector<uint32_t> in;
    uint32_t r[11];
    while (fread(r, 4, 11, f) == 11)
        in.insert(in.end(), r, r + 11);
    fclose(f);
    std::vector<uint32_t> out;
    for (size_t i = 0; i < in.size(); i += 11) {
        const uint32_t* c = &in[i];
        const KajoLaunchShape s = kajoLaunchShape(c[0], (int)c[1], (int)c[2], c[3] != 0, c[4] != 0, c[5], c[6], (int)c[7], c[8] != 0, c[9] != 0, c[10]);
        const uint32_t o[6] = {s.startsInside, s.endsInside, (uint32_t)s.launchGroups, s.split, s.chunks, s.parted};
        out.insert(out.end(), o, o + 6);
    }
    f = fopen(argv[1], "wb");
    if (!f) return 4;
    if (!out.empty())
        fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}

// Launch shapes of a handle as kajo_hip_create / kajo_hip_render plan them, through the functions they call: one line "now=..
// passesDone=..: field=value ..." per launch. argv: a.pod W H tileW tileH S fast|strict|exact flags tileIndex tileCount, then now
// passesDone for every launch. kajoCheckCreate refuses what create refuses (exit code 2), the scene is staged by the flags as create()
// stages it, the plans are kajoLdsPlan's (7: it does not fit) and kajoFramePlan's, the shape is kajoLaunchShape's. parted: with an order
// and a tail to part (orderValid, nParted = 1), which is the most a launch can be.
static int planShapeOf(int argc, char** argv)
{
    if (argc < 12 || (argc - 10) % 2 != 0) return 2;
    Pod pod;
    if (int rc = pod.read(argv[0])) return rc;
    const std::string build = argv[6];
    if (build != "fast" && build != "strict" && build != "exact") return 2;
    KajoParams p{};
    p.samplesPerPass = atoi(argv[5]);
    p.flags = (uint32_t)atoi(argv[7]) | (build == "strict" ? KAJO_FLAG_STRICT : build == "exact" ? KAJO_FLAG_EXACT : 0u);
    p.tileW = atoi(argv[3]); p.tileH = atoi(argv[4]); p.tileIndex = atoi(argv[8]); p.tileCount = atoi(argv[9]);
    const int W = atoi(argv[1]), H = atoi(argv[2]);
    char msg[256];
    if (kajoCheckCreate(pod.sc, W, H, &p, msg)) return 2;
    kajo::StagedScene st;
    kajo::stageScene(pod.sc, st, (p.flags & KAJO_FLAG_NO_GRID) ? 0 : 48, !(p.flags & KAJO_FLAG_NO_SHADOW_LISTS));
    const KajoLdsPlan lds = kajoLdsPlan(st, kajoNumerics(p.flags));
    if (!lds.fits) return 7;
    const KajoFramePlan f = kajoFramePlan(W, H, p, lds, kajoNumerics(p.flags));
    if (f.tooManyBlocks) return 2;
    for (int a = 10; a + 1 < argc; a += 2) {
        const int now = atoi(argv[a]), passesDone = atoi(argv[a + 1]);
        if (now < 1 || passesDone < 0) return 2;
        const KajoLaunchShape s = kajoLaunchShape(f, lds, p.flags, now, passesDone, true, 1u);
        printf("now=%d passesDone=%d: split=%u chunks=%u parted=%d startsInside=%d endsInside=%d launchGroups=%d wavesPerBlock=%u coldInLds=%d "
               "home=%d grouped=%d n=%d gridBlocks=%llu pixelBlocks=%llu ldsTotal=%zu\n",
               now, passesDone, s.split, s.chunks, s.parted, s.startsInside, s.endsInside, s.launchGroups, lds.wavesPerBlock, lds.coldInLds, f.home,
               f.grouped, f.n, f.gridBlocks, f.pixelBlocks, lds.ldsTotal());
    }
    return 0;
}

// The launches kajo_hip_render cuts calls into: "now passesDone" per launch. argv: passesPerLaunch noise(0|1) passesDone, then the passes
// of every call.
static int planCuts(int argc, char** argv)
{
    if (argc < 4) return 2;
    const int perLaunch = atoi(argv[0]), noise = atoi(argv[1]);
    int done = atoi(argv[2]);
    if (perLaunch < 0 || done < 0) return 2;
    for (int a = 3; a < argc; a++)
        for (int left = atoi(argv[a]), now; left > 0; left -= now, done += now) {
            now = kajoLaunchPasses(left, perLaunch, noise != 0, done);
            printf("%d %d\n", now, done);
        }
    return 0;
}

// Which render kernel an EXACT handle of each scene file launches when the whole scene is staged in LDS and no flag says otherwise:
// launch.inc.hip's choice restated over the staged scene, its last step through the function the launcher itself calls
// (fixed_counts.h kajoFixedKernelName). One line "<file>: nPlanes=.. nSpheres=.. nLights=.. coldInLds=.. kernel=<name>".
static int planKernel(int argc, char** argv)
{
    for (int a = 0; a < argc; a++) {
        Pod pod;
        if (int rc = pod.read(argv[a])) return rc;
        kajo::StagedScene st;
        kajo::stageScene(pod.sc, st, 48, true);
        const KajoLdsPlan p = kajoLdsPlan(st, Numerics::Exact);
        const char* fixed = kajoFixedKernelName(st.nPlanes, st.nSpheres);
        const char* name = !p.coldInLds ? "large-scene" : st.light.size() != 1 ? "kajo_render_exact_lights"
                         : !(st.allTranslated && st.planesRigid) ? "kajo_render_exact" : fixed ? fixed : "kajo_render_exact_simple";
        printf("%s: nPlanes=%d nSpheres=%d nLights=%zu coldInLds=%d kernel=%s\n", argv[a], st.nPlanes, st.nSpheres, st.light.size(), p.coldInLds, name);
    }
    return 0;
}

static int plan(int argc, char** argv)
{
    if (argc < 1) return 2;
    const std::string what = argv[0];
    if (what == "kernel") return planKernel(argc - 1, argv + 1);
    if (what == "lds") return planLds(argc - 1, argv + 1);
    if (what == "cuts") return planCuts(argc - 1, argv + 1);
    if (what == "shape" && argc - 1 > 2) return planShapeOf(argc - 1, argv + 1);
    if (what == "shape") return planShape(argc - 1, argv + 1);
    if (what == "sizes") return planSizes(argc - 1, argv + 1);
    return 2;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 1;
    const std::string mode = argv[1];
    if (mode == "stage") return stage(argc - 2, argv + 2);
    if (mode == "parse") return parse(argc - 2, argv + 2);
    if (mode == "order") return order(argc - 2, argv + 2);
    if (mode == "tiles") return tiles(argc - 2, argv + 2);
    if (mode == "plan") return plan(argc - 2, argv + 2);
    return 1;
}
