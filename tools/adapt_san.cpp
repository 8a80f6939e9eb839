// adapt_san.cpp -- the host half of adaptive sampling (kajo_amd/csrc/adapt_math.h beside launch_order.h) in a program of its own, for the
// sanitizers: g++ -fsanitize=address,undefined -Iinclude -Ikajo_amd/csrc tools/adapt_san.cpp (tests/test_adaptive_cpu.py builds and runs
// it). The filter of the launch order over every shape the handle can have -- 1 to 4 waves per block, SPLIT or not, none / all / every
// other / random units retired, cost order and image order -- checked against a count and a membership model; the rule over records of
// every kind; the slot-to-pixel arithmetic over ragged frames.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "launch_order.h"
#include "adapt_math.h"

static int failures = 0;
#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c);                                                  \
            failures++;                                                                                                \
        }                                                                                                              \
    } while (0)

int main()
{
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 32); };
    long words = 0;
    for (unsigned n : {0u, 1u, 2u, 7u, 64u, 1000u})
        for (unsigned w = 1; w <= 4; w++)
            for (int split = 0; split < 2; split++)
                for (int pattern = 0; pattern < 4; pattern++)
                    for (int costOrder = 0; costOrder < 2; costOrder++) {
                        std::vector<uint32_t> trips((size_t)n * w), cost, order, state(n), out;
                        for (uint32_t& t : trips)
                            t = next() % 50;
                        kajoBlockCosts(trips.data(), n, w, cost);
                        kajoCostOrder(cost, order);
                        size_t active = 0;
                        for (unsigned u = 0; u < n; u++) {
                            state[u] = pattern == 0 ? 0u : pattern == 1 ? 1u : pattern == 2 ? (u & 1u) : (next() & 1u);
                            active += state[u] == 0u;
                        }
                        kajoAdaptOrder(costOrder ? order.data() : nullptr, n, state.data(), w, split != 0, out);
                        CHECK(out.size() == active * (split ? w : 1u));
                        std::vector<int> seen((size_t)n * w, 0);
                        for (size_t i = 0; i < out.size(); i++) {
                            const uint32_t unit = split ? out[i] / w : out[i];
                            CHECK(unit < n && state[unit] == 0u);
                            CHECK(seen[out[i]]++ == 0);
                            if (!costOrder && i > 0)
                                CHECK(out[i] > out[i - 1]);
                        }
                        words += (long)out.size();
                    }
    // the rule: unknown, quiet, loud, a variance rounded below zero, a black pixel, the target itself
    const AdaptRule r{0.05f, 1e-2f, 0u};
    CHECK(kajo::adaptLoud(0.0, 0.0, 0, r) && kajo::adaptLoud(1.0, 1.0, 1, r));
    CHECK(!kajo::adaptLoud(8.0, 16.0, 4, r));                 // four equal batches: no variance
    CHECK(!kajo::adaptLoud(8.0, 16.0 - 1e-12, 4, r));         // s2 - s1^2 / n slightly negative: clamped
    CHECK(!kajo::adaptLoud(0.0, 0.0, 4, r));                  // black
    CHECK(kajo::adaptLoud(4.0, 20.0, 2, r));
    const float rel = kajo::adaptRel(4.0, 20.0, 2, 1e-2f);
    CHECK(rel > 0.0f && !kajo::adaptLoud(4.0, 20.0, 2, AdaptRule{rel, 1e-2f, 0u}));
    CHECK(kajo::adaptFactor(32, 4) == 2.0f && kajo::adaptFactor(18, 4) == 1.125f);
    // every slot of ragged frames lies where the tile map puts it, or outside
    for (int W : {1, 41, 65, 100})
        for (int H : {1, 9, 23, 75})
            for (int owners : {1, 3}) {
                const int tilesX = (W + 63) / 64, tilesY = (H + 15) / 16, nTiles = tilesX * tilesY;
                long inside = 0;
                for (int o = 0; o < owners; o++) {
                    const int owned = (nTiles - o + owners - 1) / owners;
                    const AdaptGeom g{W, H, 64, 16, tilesX, o, owners, owned < 0 ? 0 : owned};
                    const int perOwner = (nTiles + owners - 1) / owners;
                    for (uint32_t s = 0; s < (uint32_t)perOwner * 1024u; s++) {
                        int px, py;
                        if (kajo::adaptSlotPixel(g, s, &px, &py)) {
                            CHECK(px >= 0 && px < W && py >= 0 && py < H);
                            inside++;
                        }
                    }
                }
                CHECK(inside == (long)W * H);
            }
    std::printf("adapt_san: %ld order words: %s\n", words, failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
