/* Per-binade checksums of include/kajo_strictmath.h over EVERY binary32 argument, from the host build of the header: what the device
 * sweep (kajo_hip_kat_strictmath_sweep, kernel_strict.hip kajo_kat_math_sweep) must reproduce word for word.
 *   gcc -O2 -mfma -ffp-contract=off -Iinclude -o /tmp/sm_binades tools/strictmath_binades.c -lm -lpthread
 *   /tmp/sm_binades FN [YBITS [THREADS]]     FN: 0 sin, 1 cos, 2 asin, 3 acos, 4 pow(x, y), 6 the IEEE sqrtf; YBITS: y's binary32 bits, hex
 * Binade b = sign * 256 + biased exponent holds the arguments with bits b << 23 | m. One output line per binade, "A B" in hex:
 *   A = sum over m of bits(r),  B = sum over m of bits(r) * (2 m + 1),  both mod 2^64, a NaN result counted as 0x7fc00000
 * (the sign and payload of a NaN differ legitimately between x86-64 and gfx950). tools/make_strictmath_binades.py runs this for every
 * table of tests/golden/strictmath_binades.npz.
 */
#include "kajo_strictmath.h"
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>

static int g_fn, g_threads;
static float g_y;
static uint64_t g_sums[512][2];

static void* run(void* p)
{
    for (uint32_t b = (uint32_t)(uintptr_t)p; b < 512; b += (uint32_t)g_threads) {
        uint64_t A = 0, B = 0;
        for (uint32_t m = 0; m < (1u << 23); m++) {
            const float x = ksm_from_bits32((b << 23) | m);
            float r;
            switch (g_fn) {
            case 0: r = kajo_sinf(x); break;
            case 1: r = kajo_cosf(x); break;
            case 2: r = kajo_asinf(x); break;
            case 3: r = kajo_acosf(x); break;
            case 6: r = sqrtf(x); break;
            default: r = kajo_powf(x, g_y); break;
            }
            const uint64_t bits = r != r ? 0x7fc00000u : ksm_bits32(r);
            A += bits;
            B += bits * (uint64_t)(2u * m + 1u);
        }
        g_sums[b][0] = A;
        g_sums[b][1] = B;
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2 || (g_fn = atoi(argv[1])) < 0 || g_fn > 6 || g_fn == 5) {
        fprintf(stderr, "usage: %s FN [YBITS [THREADS]]   FN in 0 1 2 3 4 6\n", argv[0]);
        return 2;
    }
    g_y = ksm_from_bits32(argc > 2 ? (uint32_t)strtoul(argv[2], 0, 16) : 0u);
    g_threads = argc > 3 ? atoi(argv[3]) : 16;
    if (g_threads < 1 || g_threads > 512)
        g_threads = 16;
    pthread_t th[512];
    for (int i = 0; i < g_threads; i++)
        pthread_create(&th[i], 0, run, (void*)(uintptr_t)i);
    for (int i = 0; i < g_threads; i++)
        pthread_join(th[i], 0);
    for (int b = 0; b < 512; b++)
        printf("%016llx %016llx\n", (unsigned long long)g_sums[b][0], (unsigned long long)g_sums[b][1]);
    return 0;
}
