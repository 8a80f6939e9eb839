// checkpoint_san.cpp -- the host half of checkpoints (kajo_amd/csrc/checkpoint_host.h, checkpoint_math.h) as a stand-alone program for the
// host-only tests (tests/test_checkpoint_cpu.py builds it with -fsanitize=address,undefined): no HIP, no library, no Python in the process.
//   checkpoint_san rank W H tileW tileH owners out.bin   the canonical order of every owner: out.bin = int32 [owners][H][W], the index of the
//                                                        pixel in its owner's order, -1 for the others' pixels; the inverse and the slot
//                                                        map are checked against it and against kajoTileSlot here
//   checkpoint_san info a.ckpt ...                       kajo_hip_checkpoint_info's checks; per file one line "ok <pixels> <planes>" or
//                                                        "refused <sentence>"
//   checkpoint_san merge out.ckpt a.ckpt ...             kajo_hip_checkpoint_merge; "ok <bytes>" or "refused <sentence>"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "checkpoint_host.h"

static bool readFile(const char* path, std::vector<unsigned char>* out)
{
    FILE* f = fopen(path, "rb");
    if (!f)
        return false;
    unsigned char buf[65536];
    size_t n;
    out->clear();
    while ((n = fread(buf, 1, sizeof buf, f)) > 0)
        out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

static int fail(const char* what)
{
    fprintf(stderr, "checkpoint_san: %s\n", what);
    return 2;
}

static int runRank(int W, int H, int tileW, int tileH, int owners, const char* outPath)
{
    TileMap m{};
    m.W = W;
    m.H = H;
    m.tileW = tileW;
    m.tileH = tileH;
    m.tilesX = (W + tileW - 1) / tileW;
    m.tileCount = owners;
    const int tilesY = (H + tileH - 1) / tileH;
    const int perOwner = (m.tilesX * tilesY + owners - 1) / owners;
    m.slotsPerOwner = perOwner * tileW * tileH;
    std::vector<int32_t> plane((size_t)owners * W * H, -1);
    uint64_t total = 0;
    for (int o = 0; o < owners; o++) {
        const KajoCkptGeom g = kajoCkptGeom(m, o);
        std::vector<uint32_t> prefix((size_t)g.tilesY + 1);
        const uint64_t pixels = kajoCkptPrefix(g, prefix.data());
        total += pixels;
        uint64_t seen = 0;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                int owner;
                uint32_t slot;
                kajoTileSlot(m, x, y, &owner, &slot);
                if (kajoCkptOwns(g, x, y) != (owner == o))
                    return fail("kajoCkptOwns disagrees with kajoTileSlot");
                if (owner != o)
                    continue;
                const uint32_t r = kajoCkptRank(g, prefix.data(), x, y);
                if (r != seen++)
                    return fail("the ranks of an owner's pixels are not 0, 1, 2, ... in row-major order");
                int bx, by;
                kajoCkptPixel(g, prefix.data(), r, &bx, &by);
                if (bx != x || by != y)
                    return fail("kajoCkptPixel is not the inverse of kajoCkptRank");
                if (!kajoCkptSlotPixel(g, slot, &bx, &by) || bx != x || by != y)
                    return fail("kajoCkptSlotPixel is not the inverse of kajoTileSlot");
                plane[((size_t)o * H + y) * W + x] = (int32_t)r;
            }
        if (seen != pixels)
            return fail("the prefix table's total is not the owner's pixel count");
        // every slot of the owner's buffer: a pixel of its own inside the image, or none
        uint64_t inside = 0;
        for (uint32_t slot = 0; slot < (uint32_t)m.slotsPerOwner; slot++) {
            int x, y;
            if (!kajoCkptSlotPixel(g, slot, &x, &y))
                continue;
            int owner;
            uint32_t back;
            kajoTileSlot(m, x, y, &owner, &back);
            if (owner != o || back != slot)
                return fail("a slot maps to a pixel that does not map back");
            inside++;
        }
        if (inside != pixels)
            return fail("the slots inside the image are not the owner's pixels");
    }
    if (total != (uint64_t)W * H)
        return fail("the owners' pixels do not add up to the frame");
    FILE* f = fopen(outPath, "wb");
    if (!f || fwrite(plane.data(), sizeof(int32_t), plane.size(), f) != plane.size())
        return fail("cannot write the plane");
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rank" && argc == 8)
        return runRank(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), argv[7]);
    if (mode == "info" && argc >= 3) {
        for (int i = 2; i < argc; i++) {
            std::vector<unsigned char> blob;
            if (!readFile(argv[i], &blob))
                return fail("cannot read a section");
            // (from an allocation of exactly the blob's size: a read past its end is the sanitizer's to find)
            KajoCheckpointInfo info;
            std::string why;
            if (kajoCkptInfo(blob.empty() ? nullptr : blob.data(), blob.size(), &info, &why))
                printf("ok %llu %u\n", (unsigned long long)info.header.pixels, info.header.nPlanes);
            else
                printf("refused %s\n", why.c_str());
        }
        return 0;
    }
    if (mode == "merge" && argc >= 4) {
        std::vector<std::vector<unsigned char>> blobs((size_t)argc - 3);
        std::vector<const void*> ptrs;
        std::vector<size_t> sizes;
        for (int i = 3; i < argc; i++) {
            if (!readFile(argv[i], &blobs[(size_t)i - 3]))
                return fail("cannot read a section");
            ptrs.push_back(blobs[(size_t)i - 3].data());
            sizes.push_back(blobs[(size_t)i - 3].size());
        }
        std::vector<unsigned char> merged;
        std::string why;
        if (!kajoCkptMerge(ptrs.data(), sizes.data(), (int)ptrs.size(), merged, &why)) {
            printf("refused %s\n", why.c_str());
            return 0;
        }
        FILE* f = fopen(argv[2], "wb");
        if (!f || fwrite(merged.data(), 1, merged.size(), f) != merged.size())
            return fail("cannot write the merged section");
        fclose(f);
        printf("ok %llu\n", (unsigned long long)merged.size());
        return 0;
    }
    return fail("usage: checkpoint_san rank W H tileW tileH owners out.bin | info a.ckpt ... | merge out.ckpt a.ckpt ...");
}
