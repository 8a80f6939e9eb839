// checkpoint_math.h -- the arithmetic of checkpoints (include/kajo_hip.h "Checkpoints"), host and device: the kernels of checkpoint_kernels.cpp, the
// host half in checkpoint.cpp and the stand-alone programs of tests/test_checkpoint_cpu.py are compiled from the same lines. No HIP.
//   kajoCkptMix        the splitmix64 finaliser
//   kajoCkptTerm       the digest's term of one 32-bit word: mix(mix(p * w + j) ^ b), p the pixel's index y * W + x in the whole frame
//   KajoCkptGeom       an owner's share of a frame as the canonical order sees it: the owner's in-image pixels, y ascending then x
//   kajoCkptRank       (x, y) of an owned pixel -> its index in that order;  kajoCkptPixel: the inverse
// A plane's digest is the sum of its words' terms modulo 2^64: it depends neither on the tile layout nor on the order of summation, and the
// digests of owners that share a frame add up to the whole frame's.
#ifndef KAJO_CHECKPOINT_MATH_H
#define KAJO_CHECKPOINT_MATH_H

#include <stdint.h>

#include "render_args.h"

#if defined(__HIPCC__)
#define KAJO_CKPT_HD __host__ __device__
#else
#define KAJO_CKPT_HD
#endif

KAJO_CKPT_HD static inline uint64_t kajoCkptMix(uint64_t k)
{
    k += 0x9E3779B97F4A7C15ull;
    k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
    k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
    return k ^ (k >> 31);
}

// word j of the w words of pixel p, with the bits b
KAJO_CKPT_HD static inline uint64_t kajoCkptTerm(uint64_t p, uint32_t w, uint32_t j, uint32_t b)
{
    return kajoCkptMix(kajoCkptMix(p * w + j) ^ (uint64_t)b);
}

// The owner's share of the frame. Tiles are dealt round-robin (render_args.h kajoTileSlot): in tile row ty the owner has the tiles
// tx = first(ty), first(ty) + tileCount, ...; every image row of a tile row holds the same number of its pixels, and only the frame's
// last tile column can be narrower than tileW -- it is the last of its row, so k / tileW still numbers the owner's tiles of a row.
// prefix[ty]: the owner's pixels in the tile rows above ty (tilesY + 1 words, built on the host by kajoCkptPrefix).
struct KajoCkptGeom
{
    int32_t W, H, tileW, tileH, tilesX, tilesY, tileIndex, tileCount;
};

KAJO_CKPT_HD static inline KajoCkptGeom kajoCkptGeom(const TileMap& m, int tileIndex)
{
    KajoCkptGeom g;
    g.W = m.W;
    g.H = m.H;
    g.tileW = m.tileW;
    g.tileH = m.tileH;
    g.tilesX = m.tilesX;
    g.tilesY = (m.H + m.tileH - 1) / m.tileH;
    g.tileIndex = tileIndex;
    g.tileCount = m.tileCount;
    return g;
}

// the owner's first tile column of tile row ty (>= tilesX: none)
KAJO_CKPT_HD static inline int kajoCkptFirstTile(const KajoCkptGeom& g, int ty)
{
    const long long base = (long long)ty * g.tilesX;
    return (int)(((g.tileIndex - base) % g.tileCount + g.tileCount) % g.tileCount);
}

// the owner's pixels in one image row of tile row ty
KAJO_CKPT_HD static inline uint32_t kajoCkptRowPixels(const KajoCkptGeom& g, int ty)
{
    const int first = kajoCkptFirstTile(g, ty);
    if (first >= g.tilesX)
        return 0;
    const int n = (g.tilesX - 1 - first) / g.tileCount + 1;
    const int last = first + (n - 1) * g.tileCount;
    uint32_t pixels = (uint32_t)n * (uint32_t)g.tileW;
    if (last == g.tilesX - 1)
        pixels -= (uint32_t)(g.tilesX * g.tileW - g.W); // the frame's last tile column, as wide as the frame leaves it
    return pixels;
}

// prefix[0 .. tilesY]; returns the owner's pixels. prefix == null: only the count (no table is needed for it)
static inline uint64_t kajoCkptPrefix(const KajoCkptGeom& g, uint32_t* prefix)
{
    uint64_t at = 0;
    for (int ty = 0; ty < g.tilesY; ty++) {
        if (prefix)
            prefix[ty] = (uint32_t)at;
        const int rows = g.H - ty * g.tileH < g.tileH ? g.H - ty * g.tileH : g.tileH;
        at += (uint64_t)kajoCkptRowPixels(g, ty) * (uint32_t)rows;
    }
    if (prefix)
        prefix[g.tilesY] = (uint32_t)at;
    return at;
}

// Does the owner have pixel (x, y) of the image?
KAJO_CKPT_HD static inline bool kajoCkptOwns(const KajoCkptGeom& g, int x, int y)
{
    const int tx = x / g.tileW, ty = y / g.tileH;
    return (int)(((long long)ty * g.tilesX + tx) % g.tileCount) == g.tileIndex;
}

// The index of the owner's pixel (x, y) in canonical order
KAJO_CKPT_HD static inline uint32_t kajoCkptRank(const KajoCkptGeom& g, const uint32_t* prefix, int x, int y)
{
    const int tx = x / g.tileW, ty = y / g.tileH;
    const int j = (tx - kajoCkptFirstTile(g, ty)) / g.tileCount;
    return prefix[ty] + (uint32_t)(y - ty * g.tileH) * kajoCkptRowPixels(g, ty) + (uint32_t)j * (uint32_t)g.tileW + (uint32_t)(x - tx * g.tileW);
}

// ... and the pixel of index r < prefix[tilesY]
KAJO_CKPT_HD static inline void kajoCkptPixel(const KajoCkptGeom& g, const uint32_t* prefix, uint32_t r, int* x, int* y)
{
    // the last tile row whose prefix is <= r: prefix[ty] <= r < prefix[ty + 1] (a tile row without a pixel of the owner's shares its
    // prefix with the next one and is never the last)
    int lo = 0, hi = g.tilesY - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int ty = lo;
    const uint32_t row = kajoCkptRowPixels(g, ty), in = r - prefix[ty];
    const uint32_t iy = in / row, k = in - iy * row;
    const uint32_t j = k / (uint32_t)g.tileW;
    *y = ty * g.tileH + (int)iy;
    *x = (kajoCkptFirstTile(g, ty) + (int)j * g.tileCount) * g.tileW + (int)(k - j * (uint32_t)g.tileW);
}

// The pixel of slot `slot` of the owner's tile buffer (the inverse of kajoTileSlot), or false: padding, or outside the image
KAJO_CKPT_HD static inline bool kajoCkptSlotPixel(const KajoCkptGeom& g, uint32_t slot, int* x, int* y)
{
    const uint32_t wavesPerTile = (uint32_t)(g.tileW >> 3) * (uint32_t)(g.tileH >> 3);
    const uint32_t lane = slot & 63u, wave = slot >> 6;
    const uint32_t local = wave / wavesPerTile, wb = wave - local * wavesPerTile;
    const long long tile = (long long)local * g.tileCount + g.tileIndex;
    if (tile >= (long long)g.tilesX * g.tilesY)
        return false;
    const int tx = (int)(tile % g.tilesX), ty = (int)(tile / g.tilesX);
    const uint32_t bx = wb % (uint32_t)(g.tileW >> 3), by = wb / (uint32_t)(g.tileW >> 3);
    *x = tx * g.tileW + (int)(bx * 8 + (lane & 7u));
    *y = ty * g.tileH + (int)(by * 8 + (lane >> 3));
    return *x < g.W && *y < g.H;
}

// The digest of `count` consecutive records of w words in canonical order, on the host (kajo_hip_checkpoint_info; the tests)
static inline uint64_t kajoCkptDigestHost(const KajoCkptGeom& g, const uint32_t* prefix, const uint32_t* words, uint64_t count, uint32_t w)
{
    uint64_t sum = 0;
    for (uint64_t r = 0; r < count; r++) {
        int x, y;
        kajoCkptPixel(g, prefix, (uint32_t)r, &x, &y);
        const uint64_t p = (uint64_t)y * (uint32_t)g.W + (uint32_t)x;
        for (uint32_t j = 0; j < w; j++)
            sum += kajoCkptTerm(p, w, j, words[r * w + j]);
    }
    return sum;
}

// ... of a block that is not per pixel (the ADAPT block, the counters): word i is "pixel" i of one word
static inline uint64_t kajoCkptDigestWords(const uint32_t* words, uint64_t count)
{
    uint64_t sum = 0;
    for (uint64_t i = 0; i < count; i++)
        sum += kajoCkptTerm(i, 1, 0, words[i]);
    return sum;
}

#endif
