// integrator.inc.hip -- the per-pixel Monte-Carlo integrator as ONE wave64 megakernel.
//
// Included three times: kernel_fast.hip (KAJO_STRICT 0, compiled with FMA contraction and the
// gfx950 hardware transcendentals), kernel_strict.hip (KAJO_STRICT 1, compiled
// -ffp-contract=off, include/kajo_strictmath.h for the five libm functions, IEEE divide and
// sqrt, binary64 exactly where the reference's expressions promote through M_PI / M_1_PI) and
// kernel_exact.hip (KAJO_STRICT 1 + KAJO_EXACT 1, compiled -ffp-contract=off as well).
// STRICT exists to prove that the kernel takes, path for path, the decisions of the CPU
// integrator (it is compared bit for bit with the oracle); FAST is the fastest path.
// EXACT ("decision-exact", round 5) is STRICT wherever a value can reach a DECISION -- the closest-hit
// walk, hit point, normal, reflection vector, every sampled direction, every coin, the generator -- so each
// path meets the oracle's objects, draws the oracle's random numbers and ends in the oracle's generator state;
// and FAST wherever a value only SCALES what the path carries: BSDF values and pdfs toward a given direction
// (BSDF.cpp:30-39,62-74,87-91), the light's pdf (Light.cpp:48-62), the MIS weight and the throughput /
// contribution products (Shader.cpp:74-83,203-212). Its radiance differs from the oracle's in the last places
// of each path's products and in nothing else: KAJO_RSTRICT below marks the forks that are radiance only.
//
// What it replaces (reference file:line):
//   camera ray generation + sample loop     renderer/cpu/Renderer.cpp:38-72
//   closest hit over planes, then spheres   renderer/cpu/Raytracer.cpp:21-138
//   Russian roulette, lobe choice, MIS      renderer/cpu/Shader.cpp:50-215
//   Lambert / Phong / mirror / refraction   renderer/cpu/BSDF.cpp:14-136
//   spherical light sampling                renderer/cpu/Light.cpp:26-62
//   the shuffle-add generator               renderer/cpu/Random.cpp:27-53,104-117
//
// Execution model (not the reference's): one lane owns one pixel of an 8x8 block and works
// through that pixel's n*n*passes camera paths in the reference's order, so the per-pixel
// float sums are formed exactly as Renderer.cpp:66-71 forms them. A path is a little state
// machine; every trip round the loop traces exactly ONE ray per lane (camera/extension ray
// or shadow ray) through the brute-force closest-hit loop -- the part that is 65 % of the
// reference's CPU time -- with all 64 lanes testing the same primitive from one LDS
// broadcast read. When a lane's path ends (Russian roulette kills 65 % at the first vertex)
// the lane starts its next camera path in the same trip: lanes regenerate work locally
// instead of idling until the longest path of the wave finishes. Shader::shade's recursion
// is a loop carrying a throughput; calculateLightProbabilities' re-traces are replaced by
// the hit of the extension ray that they duplicate (same ray, Shader.cpp:197-205).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_scene.h"
#include "kajo_stream.h"
#include "render_args.h"
#ifndef KAJO_EXACT
#define KAJO_EXACT 0
#endif
#if KAJO_EXACT && !KAJO_STRICT
#error "KAJO_EXACT is a variant of the STRICT build"
#endif
// the oracle's arithmetic for values that only scale radiance, too (STRICT proper)
#define KAJO_RSTRICT (KAJO_STRICT && !KAJO_EXACT)
#if KAJO_STRICT
#include "kajo_strictmath.h"
#endif

#define KDEV __device__ __forceinline__
// in front of the two loops of trace()'s SIMPLE STRICT / EXACT walk: nothing, unless the including unit instantiates the walk with
// compile-time counts and asks for straight-line code (kernel_exact_fixed.cpp)
#ifndef KAJO_FIXED_UNROLL
#define KAJO_FIXED_UNROLL
#endif
typedef __attribute__((address_space(3))) volatile uint32_t KajoLdsWord; // a word of LDS that other lanes of the wave write
// A float4 of global memory behind a pointer that waited in two LDS words (renderBody GROUPS): the address space spelled out -- a
// pointer made from an integer is generic, and stores through it would be flat_store instructions.
typedef float KajoVec4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) KajoVec4 KajoGlobalVec4;
#define KAJO_GLOBAL_VEC4(lo, hi) \
    ((KajoGlobalVec4*)((uint64_t)__builtin_bit_cast(uint32_t, lo) | ((uint64_t)__builtin_bit_cast(uint32_t, hi) << 32)))

namespace
{

struct F3
{
    float x, y, z;
};

KDEV F3 f3(float x, float y, float z) { return F3{x, y, z}; }
KDEV F3 operator+(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
KDEV F3 operator-(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
KDEV F3 operator-(F3 a) { return f3(-a.x, -a.y, -a.z); }
KDEV F3 operator*(F3 a, float s) { return f3(a.x * s, a.y * s, a.z * s); }
KDEV F3 operator*(float s, F3 a) { return f3(a.x * s, a.y * s, a.z * s); }
KDEV F3 operator*(F3 a, F3 b) { return f3(a.x * b.x, a.y * b.y, a.z * b.z); }
KDEV float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
KDEV F3 cross(F3 a, F3 b) { return f3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }
KDEV F3 ld3(const float* p) { return f3(p[0], p[1], p[2]); }
// Sums of products that only SCALE what a path carries (its radiance, its throughput, a pdf toward a given direction): the EXACT build --
// compiled -ffp-contract=off for the sake of everything that decides -- forms them with fused multiply-adds, spelled out so that every
// kernel instance forms the same bits (a contraction left to the compiler is per instance). STRICT proper keeps the oracle's separate
// roundings, FAST the expressions its compiler contracts as before. NOT for a cosine that something is divided by: where the oracle's
// separately rounded dot product is exactly zero the quotient is infinite and inf * 0 a not-a-number pixel (the reference has them:
// grazing glass and mirror hits), which a fused sum -- almost never exactly zero -- would turn into a finite one (caustics scene: 19
// such pixels against the oracle's 29, tests/test_hip_whole_frames.py).
#ifndef KAJO_EXACT_FMA
#define KAJO_EXACT_FMA 1
#endif
#if defined(KAJO_EXACT) && KAJO_EXACT && KAJO_EXACT_FMA
KDEV float rdot(F3 a, F3 b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
KDEV F3 rmadd(F3 a, F3 b, F3 c) { return f3(__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y), __builtin_fmaf(a.z, b.z, c.z)); } // c + a * b
#else
KDEV float rdot(F3 a, F3 b) { return dot(a, b); }
KDEV F3 rmadd(F3 a, F3 b, F3 c) { return c + a * b; }
#endif

// ---- numerics policy ------------------------------------------------------------------
#if KAJO_STRICT
#ifndef KAJO_IEEE_BY_COMPILER
#define KAJO_IEEE_BY_COMPILER 0 // 1: `a / b` and __builtin_sqrtf as hipcc lowers them (the A/B baseline of the two functions below)
#endif
#if KAJO_IEEE_BY_COMPILER
KDEV float kdiv(float a, float b) { return a / b; }
KDEV float ksqrt(float a) { return __builtin_sqrtf(a); }
KDEV float ksqrtWalk(float a) { return ksqrt(a); }
#else
// The correctly rounded quotient and square root, as hipcc's own lowering computes them, WITHOUT its range scaling.
// hipcc: v_div_scale x2 (pre-scale by 2^+-64 when the denominator is subnormal or beyond 2^126, the exponents are 96 or more apart,
// the quotient would be subnormal, or the numerator is below 2^-103), v_rcp, one Newton step on the reciprocal, quotient, two residual
// corrections (the last one v_div_fmas, which undoes the scaling), v_div_fixup (zeros, infinities, NaNs): 11 instructions, four of
// them in the half-rate classes. Below: the same v_rcp, the same six FMAs / multiply on the same operands, the same v_div_fixup -- 9
// instructions, one half-rate -- so every operand pair that v_div_scale leaves alone gets hipcc's bits, i.e. the IEEE quotient the
// oracle's x86 division returns. The walk's operands -- plane offsets over direction components no smaller than FLT_EPSILON
// (Raytracer.cpp:82-85; the quotient of a smaller one is not used), roots q / a and c / q (Raytracer.cpp:36-44), reciprocal lengths --
// are zero or sit dozens of binades inside that range for any scene whose non-zero coordinates lie in 2^-40 .. 2^40: a difference of
// binary32 values is zero or at least 2^-24 of the smaller one. tests/test_hip_exact.py pins both functions against IEEE on 2^22
// operand pairs over 2^-47 .. 2^47 plus the special values, and every STRICT = oracle frame test pins them in the walk.
// tests/test_strictmath.py checks the quotient on EVERY exponent pair of 2^-47 .. 2^47 and of the whole domain stated above (a normal
// denominator of at most 2^126, exponents fewer than 96 apart, a normal quotient, a numerator of at least 2^-103), with the mantissas
// at the ends, in the middle and at random: no quotient differs from IEEE.
KDEV float kdiv(float a, float b)
{
    float y = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, y, 1.0f);
    y = __builtin_fmaf(e, y, y);
    float q = a * y;
    float r = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(r, y, q);
    r = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(r, y, q);
    return __builtin_amdgcn_div_fixupf(q, b, a);
}
// hipcc: scale arguments below 2^-96 by 2^32, v_sqrt (1 ulp), the two neighbours of its result by integer +-1, the exact residuals
// x - s * neighbour (one FMA each) pick the correctly rounded one, unscale, and a v_cmp_class patch for 0 / inf: 16 instructions, nine
// half-rate. Below: the middle part alone, 9 instructions. Zeros, infinities, NaNs and negative normal arguments fall through the two
// selections unchanged (their residuals are NaN or zero: no comparison holds), so only arguments in (0, 2^-96) are outside its domain:
// a discriminant, squared length or variate is zero or above 2^-64 under the range stated above. A negative SUBNORMAL argument is not
// among them: v_sqrt_f32 flushes it to -0 and returns -0 where IEEE gives NaN (found by the sweep below). ksqrt answers negative
// arguments by a select of its own. ksqrtWalk is the root without that select, for the sphere tests of the closest-hit and shadow walks
// alone (the select there is 1 % of the benchmarked frame's time): their discriminants are zero or at least 2^-64 in magnitude under
// the range kajo_hip_create enforces, never a negative subnormal, and equal to ksqrt everywhere else by construction.
// Checked against the IEEE sqrtf at EVERY binary32 (tests/test_strictmath.py, kajo_hip_kat_strictmath_sweep): all 225 positive binades
// from 2^-96 up, +-0, +inf, NaNs and all 256 negative binades agree for ksqrt, and for ksqrtWalk all of them but the negative subnormal
// one. Of the 31 positive binades below 2^-96, which are not asserted, the 8 from 2^-104 up agree too and the 23 below (v_sqrt_f32's
// own denormal range for the root's neighbours and residuals) do not.
KDEV float ksqrtWalk(float x)
{
    float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) - 1u), su = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) + 1u);
    const float rd = __builtin_fmaf(-sd, s, x), ru = __builtin_fmaf(-su, s, x);
    s = 0.0f >= rd ? sd : s;
    s = 0.0f < ru ? su : s;
    return s;
}
KDEV float ksqrt(float x)
{
    const float s = ksqrtWalk(x);
    return x < 0.0f ? __builtin_bit_cast(float, 0x7fc00000u) : s;
}
#endif
KDEV float krcp(float a) { return kdiv(1.0f, a); }
KDEV float kpow(float x, float y) { return kajo_powf(x, y); }
#else
// FAST: the hardware's 1-ulp reciprocal, square root and reciprocal square root (profiles/r01_hwmath_accuracy.txt; swapping in
// the correctly rounded operations does not move the pixels where FAST and the oracle part: profiles/r01_flip_experiment.txt).
KDEV float krcp(float a) { return __builtin_amdgcn_rcpf(a); }
KDEV float ksqrt(float a) { return __builtin_amdgcn_sqrtf(a); }
KDEV float ksqrtWalk(float a) { return ksqrt(a); }
KDEV float krsq(float a) { return __builtin_amdgcn_rsqf(a); }
KDEV float kdiv(float a, float b) { return a * krcp(b); }
// x >= 0 (clamped cosine / uniform variate / clamped colour): x^y = 2^(y log2 x); v_log(0) = -inf
// gives 2^-inf = 0 for y > 0, and y == 0 is answered explicitly as libm does (pow(x, 0) = 1)
KDEV float kpow(float x, float y)
{
    float r = __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));
    return y == 0.0f ? 1.0f : r;
}
#endif
// the Phong lobe: its exponent is never zero (a zero exponent selects the ideal reflector, Shader.cpp:155-158)
// (value and pdf toward a GIVEN direction: radiance only)
#if KAJO_RSTRICT
KDEV float kpowPhong(float x, float y) { return kajo_powf(x, y); }
#else
KDEV float kpowPhong(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }
#endif
// reciprocal of a value that only scales radiance (a pdf, a pdf sum, a clamped cosine under a colour)
#if KAJO_RSTRICT
KDEV float rrcp(float a) { return kdiv(1.0f, a); }
#else
KDEV float rrcp(float a) { return __builtin_amdgcn_rcpf(a); }
#endif

// max(0, x) for an x that cannot exceed 1 (cosines of unit vectors, 1 - u, 1 - x^2): FAST folds it into the
// clamp modifier of the instruction that produces x (v_max_f32 issues at half rate on gfx950)
#if KAJO_STRICT
KDEV float kmax0(float x) { return fmaxf(0.0f, x); }
#else
KDEV float kmax0(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }
#endif

KDEV F3 normalize(F3 a)
{
    float sqr = a.x * a.x + a.y * a.y + a.z * a.z;
#if KAJO_STRICT
    return a * kdiv(1.0f, ksqrt(sqr)); // glm: x * inversesqrt(dot), inversesqrt = 1 / sqrt
#else
    return a * krsq(sqr);
#endif
}

KDEV float length(F3 a) { return ksqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
KDEV F3 reflect(F3 I, F3 N) { return I - N * dot(N, I) * 2.0f; }

const float kEps = 0.001f;              // g_surfaceEpsilon, Shader.cpp:23
const float kFltEpsilon = 1.1920929e-7f; // std::numeric_limits<float>::epsilon()
#if KAJO_STRICT
const double kPi = 3.14159265358979323846;
#endif
#if KAJO_RSTRICT
const double kInvPi = 0.31830988618379067154;
#else
const float kInvPiF = 0.31830988618379067154f;
const float kInv2PiF = 0.15915494309189533577f;
#endif

// ---- RNG (Random.cpp:27-53): state = (lo, hi); hi += perm(hi), lo += old hi -----------
struct Rng
{
    uint64_t lo, hi;
};

KDEV void rngStep(Rng& r)
{
    uint64_t h = r.hi;
    uint32_t h0 = (uint32_t)h, h1 = (uint32_t)(h >> 32);
    // 16-bit words [a,b,c,d] -> [c,d,b,a]: low dword = old high dword, high dword = rot16(old low)
    uint64_t p = (uint64_t)h1 | ((uint64_t)__builtin_amdgcn_alignbit(h0, h0, 16) << 32);
    r.lo = r.lo + h;
    r.hi = h + p;
}

// One lane of Random::generate (Random.cpp:41-42) mapped to [0, 1) as every caller does: (float)(int)bits * 2^-31, then
// x * .5 + .5 (Random.cpp:113, Renderer.cpp:55, Light.cpp:39-41, Random.cpp:79-80). The two multiplications are by
// powers of two -- exact -- so the value is fl(f * 2^-32 + .5) with f = (float)(int)bits, which ONE fused multiply-add
// delivers with the same single rounding, in both numerics modes (two instructions instead of four).
KDEV float unitBits(uint32_t bits) { return __builtin_fmaf((float)(int32_t)bits, 2.3283064365386963e-10f, 0.5f); }

// flipCoin, Random.cpp:111-117
KDEV bool flipCoin(Rng& r, float probability, float& outProbability)
{
    rngStep(r);
    float u = unitBits((uint32_t)r.lo);
    bool v = (probability != 0.0f) && (u <= probability);
    outProbability = v ? probability : __fsub_rn(1.0f, probability);
    return v;
}

// ---- closest hit (Raytracer.cpp:21-138) --------------------------------------------------
struct Hit
{
    int id;     // 0 miss; 1..nPlanes planes; nPlanes+1.. spheres
    float t;    // ray.maxDistance after the walk
    float t0;   // object-space parameter of a sphere hit
};

// Pointers the integrator reads the scene through. The hot records are always in LDS; the cold
// ones (shading frames, sphere centres, materials, light list) are in LDS too when the whole scene
// fits the workgroup's budget, else they stay in global memory (L2-resident: a 1000-sphere scene is
// 200 KiB).
struct LdsScene
{
    const DFloat4* planeRow;
    const float* planeDet;
    const DFloat4* sphereHot;
    const uint32_t* sphereHotOffset;
    const DFloat4* planeFrame;
    const DSphereCold* sphereCold;
    const DMaterial* material;
    const int32_t* light;          // [nLights] sphere indices, always in LDS
    const DSphereCold* lightCold;  // [nLights] the lights' own cold records and
    const DFloat4* lightEmission;  // [nLights] emissions, always in LDS: a large scene's light loop reads nothing from global memory
    const float* lightPlaneSide;   // [nLights][nPlanes] +1 / -1: the light's whole ball lies on that side of the plane (by a margin); 0: it does not
    const DFloat4* camera;         // [8] p1, p2 - p1, p3 - p1, origin (Renderer.cpp:29-34), background, the pixel / sample sizes of
                                   // Renderer.cpp:39-42, stream key words + W + H: read where a camera ray is formed /
                                   // a ray escapes, instead of fifteen scalar registers held through the whole loop (the loop spills SGPRs);
                                   // [7] and the .w words of [0..3]: what the end of the kernel needs of the launch (renderBody)
    const DFloat4* gridHeader;     // [5] (bmin, dim.x), (bmax, dim.y), (cell, dim.z), (1 / cell, -), (centre, reach^2): LDS, read at the start of a walk
    // The grid's cell lists, as staged into LDS when they fit (DGrid.inLds; else they are read from sc.grid's global arrays).
    // The two homes are kept in SEPARATE pointers and the walk is instantiated once per home: a pointer that may be either
    // compiles to FLAT loads with a full `s_waitcnt vmcnt(0) lgkmcnt(0)` behind each -- which is what round 2's walk paid for
    // every cell record and every item (profiles/r03_c5_notes.txt).
    const uint32_t* gridCellStartLds;
    const uint16_t* gridItemsLds;
#ifdef KAJO_COUNT_SPHERE_TESTS
    unsigned long long* testCounter; // diagnostic twin: [0] sphere tests of the grid walks, [1] of the list walks, [2] light-sphere tests of the queries (lane counts)
#endif
};

// Counting twin only (`make -C kajo_amd/csrc count`: -DKAJO_COUNT_SPHERE_TESTS; its atomics distort every timing): how many sphere
// tests the LANES of this wave are about to run -- the algorithmic work of a culled walk is what each ray's own walk tests
// (tools/configs_roofline.py) -- one atomic per wave and loop round, by its first active lane.
#ifdef KAJO_COUNT_SPHERE_TESTS
#define KAJO_COUNT_TESTS(lds, which)                                                                                   \
    do {                                                                                                               \
        if ((lds).testCounter) {                                                                                       \
            const unsigned long long m_ = __ballot(true);                                                              \
            if ((int)(threadIdx.x & 63) == __builtin_ctzll(m_))                                                        \
                atomicAdd((lds).testCounter + (which), (unsigned long long)__builtin_popcountll(m_));                  \
        }                                                                                                              \
    } while (0)
#else
#define KAJO_COUNT_TESTS(lds, which)                                                                                   \
    do {                                                                                                               \
    } while (0)
#endif

// One sphere of Raytracer.cpp:21-72 up to (not including) processIntersection: returns false when the
// reference returns early (discriminant < 0, or both roots behind the origin); otherwise th = the
// object-space parameter the reference reports and ts = th * determinant.
// ALLT: every sphere of the scene is known to be a (centre, radius) record (the kernels of scenes with visibility lists: stage.cpp builds
// lists only for such scenes) -- the general record's code is not compiled in.
template <bool ALLT = false>
KDEV bool sphereCandidate(const DSceneView& sc, const LdsScene& lds, int i, F3 O, F3 d, float aT, float iaT, float& ts, float& th)
{
    // a t^2 + 2 h t + c = 0 in object space (the reference's b = 2 h); ia = 1 / a
    float a, h, c, det;
#if !KAJO_STRICT
    float ia;
#endif
    const uint32_t off = (ALLT || sc.allTranslated) ? (uint32_t)i : lds.sphereHotOffset[i];
    if (ALLT || !(off & KAJO_SPHERE_GENERAL)) {
        const DFloat4 s = lds.sphereHot[off];
        F3 o = f3(O.x + s.x, O.y + s.y, O.z + s.z);
        a = aT;
        h = dot(d, o);
        c = dot(o, o) - s.w;
        det = 1.0f;
#if !KAJO_STRICT
        ia = iaT;
#endif
    } else {
        const int k = (int)(off & ~KAJO_SPHERE_GENERAL);
        const DFloat4 r0 = lds.sphereHot[k], r1 = lds.sphereHot[k + 1], r2 = lds.sphereHot[k + 2];
        const DFloat4 q = lds.sphereHot[k + 3];
        F3 dir = f3(r0.x * d.x + r0.y * d.y + r0.z * d.z, r1.x * d.x + r1.y * d.y + r1.z * d.z,
                    r2.x * d.x + r2.y * d.y + r2.z * d.z);
        F3 o = f3(r0.x * O.x + r0.y * O.y + r0.z * O.z + r0.w * 1.0f, r1.x * O.x + r1.y * O.y + r1.z * O.z + r1.w * 1.0f,
                  r2.x * O.x + r2.y * O.y + r2.z * O.z + r2.w * 1.0f);
        a = dot(dir, dir);
        h = dot(dir, o);
        c = dot(o, o) - q.x;
        det = q.y;
#if !KAJO_STRICT
        ia = krcp(a);
#endif
    }
#if KAJO_STRICT
    // Raytracer.cpp:26-44 verbatim: b = 2 dot, discriminant b^2 - 4ac, q by the sign of b,
    // roots q/a and c/q, sorted
    float b = 2 * h;
    float discr = b * b - 4 * a * c;
    // The correctly rounded square root and the two divisions are 38 of this test's 62 instructions; a wave whose rays ALL
    // miss the sphere's line (primary rays of an 8x8 block mostly do) skips them. No lane's result depends on it.
    // (Lanes without a ray run along with stale registers and vote too; taking their vote away -- one scalar AND per sphere --
    // measured 1 % slower than the skips it adds are worth.)
    if (__builtin_amdgcn_ballot_w64(!(discr < 0.0f)) == 0ull) {
        ts = th = 0.0f;
        return false;
    }
    float sq = ksqrtWalk(discr);
    float q = (b < 0.0f) ? (-b - sq) * .5f : (-b + sq) * .5f;
    float t0 = kdiv(q, a);
    float t1 = kdiv(c, q);
    bool sw = t0 > t1;
    float lo = sw ? t1 : t0, hi = sw ? t0 : t1;
#else
    // The same two roots (q/a and c/q are the roots of a t^2 + b t + c, by Vieta) as
    // t = (-h -+ sqrt(h^2 - a c)) / a: one reciprocal per ray instead of two per sphere, no
    // sort. Differs from the reference's evaluation in the last bits only.
    float discr = h * h - a * c;
    float sq = ksqrtWalk(discr);
    float lo = (-h - sq) * ia, hi = (sq - h) * ia;
#endif
    th = (lo < 0.0f) ? hi : lo;
    ts = th * det;
    return !(discr < 0.0f) && !(hi < 0.0f);
}

// Large scenes: visit only the spheres registered in the grid cells the ray crosses, front to back.
// Acceptance reproduces the brute-force walk: closest ts wins; among equal ts the later object wins
// (Raytracer.cpp:115 rejects only ts > max), so a sphere ties over a plane and over a lower-index sphere.
template <bool ALLT>
KDEV void gridWalkIn(const DSceneView& sc, const LdsScene& lds, const uint32_t* gridCellStart, const uint16_t* gridItems, F3 O, F3 d, float aT,
                     float iaT, float& tMax, int& best, float& bestT0)
{
    // the grid's header from LDS into vector registers for the duration of the walk (held in scalar registers through the
    // whole render loop it made the large-scene kernels spill them by the dozen)
    struct
    {
        float bmin[3], bmax[3], cell[3], invCell[3];
        int dim[3];
    } g;
    {
        const DFloat4 h0 = lds.gridHeader[0], h1 = lds.gridHeader[1], h2 = lds.gridHeader[2], h3 = lds.gridHeader[3];
        g.bmin[0] = h0.x, g.bmin[1] = h0.y, g.bmin[2] = h0.z, g.dim[0] = __builtin_bit_cast(int, h0.w);
        g.bmax[0] = h1.x, g.bmax[1] = h1.y, g.bmax[2] = h1.z, g.dim[1] = __builtin_bit_cast(int, h1.w);
        g.cell[0] = h2.x, g.cell[1] = h2.y, g.cell[2] = h2.z, g.dim[2] = __builtin_bit_cast(int, h2.w);
        g.invCell[0] = h3.x, g.invCell[1] = h3.y, g.invCell[2] = h3.z;
    }
    const int np = sc.nPlanes;
    const float inf = __builtin_inff();
    const float ix_ = 1.0f / d.x, iy_ = 1.0f / d.y, iz_ = 1.0f / d.z;
    // slab test against the grid bounds (fminf/fmaxf drop the NaN of 0 * inf)
    float ax = (g.bmin[0] - O.x) * ix_, bx = (g.bmax[0] - O.x) * ix_;
    float ay = (g.bmin[1] - O.y) * iy_, by = (g.bmax[1] - O.y) * iy_;
    float az = (g.bmin[2] - O.z) * iz_, bz = (g.bmax[2] - O.z) * iz_;
    float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
    float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    // a ray parallel to a slab and outside it never enters
    bool outside = (d.x == 0.0f && (O.x < g.bmin[0] || O.x > g.bmax[0])) || (d.y == 0.0f && (O.y < g.bmin[1] || O.y > g.bmax[1])) ||
                   (d.z == 0.0f && (O.z < g.bmin[2] || O.z > g.bmax[2]));
    if (outside || !(tn <= tf) || !(tn <= tMax))
        return;
    const float px = O.x + d.x * tn, py = O.y + d.y * tn, pz = O.z + d.z * tn;
    int cx = min(max((int)__builtin_floorf((px - g.bmin[0]) * g.invCell[0]), 0), g.dim[0] - 1);
    int cy = min(max((int)__builtin_floorf((py - g.bmin[1]) * g.invCell[1]), 0), g.dim[1] - 1);
    int cz = min(max((int)__builtin_floorf((pz - g.bmin[2]) * g.invCell[2]), 0), g.dim[2] - 1);
    const int sx = d.x >= 0.0f ? 1 : -1, sy = d.y >= 0.0f ? 1 : -1, sz = d.z >= 0.0f ? 1 : -1;
    // ray parameter at which the next cell boundary along each axis is crossed, and its increment
    float nx = d.x == 0.0f ? inf : ((cx + (sx > 0 ? 1 : 0)) * g.cell[0] + g.bmin[0] - O.x) * ix_;
    float ny = d.y == 0.0f ? inf : ((cy + (sy > 0 ? 1 : 0)) * g.cell[1] + g.bmin[1] - O.y) * iy_;
    float nz = d.z == 0.0f ? inf : ((cz + (sz > 0 ? 1 : 0)) * g.cell[2] + g.bmin[2] - O.z) * iz_;
    const float dx = d.x == 0.0f ? inf : g.cell[0] * __builtin_fabsf(ix_);
    const float dy = d.y == 0.0f ? inf : g.cell[1] * __builtin_fabsf(iy_);
    const float dz = d.z == 0.0f ? inf : g.cell[2] * __builtin_fabsf(iz_);
    // The walk is one loop without inner branches on the axis: the cell is a linear index moved by a per-axis stride, the
    // cells left before the grid ends are counted per axis, and the axis to cross is chosen with selects (the three-way
    // branch of a textbook DDA runs all three arms in a wave of incoherent rays).
    int cell = (cz * g.dim[1] + cy) * g.dim[0] + cx;
    const int strideX = sx, strideY = sy * g.dim[0], strideZ = sz * g.dim[0] * g.dim[1];
    int leftX = sx > 0 ? g.dim[0] - 1 - cx : cx, leftY = sy > 0 ? g.dim[1] - 1 - cy : cy, leftZ = sz > 0 ? g.dim[2] - 1 - cz : cz;
    for (int guard = g.dim[0] + g.dim[1] + g.dim[2] + 3; guard > 0; guard--) {
        const uint32_t k0 = gridCellStart[cell];
        const uint32_t e = gridCellStart[cell + 1];
#if !KAJO_STRICT
        if (ALLT || sc.allTranslated) {
            // (centre, radius) spheres with the bookkeeping of the brute-force walk: the smaller non-negative root is
            // the smaller bit pattern, "exists, not behind, closer" one unsigned compare (plus the tie rule)
            // Closest wins; among bit-identical distances the LATER object (Raytracer.cpp:115 rejects only t > max, objects in scene
            // order) -- whatever the order the cells deliver them in. (distance pattern, ~id) as ONE 64-bit key, smaller wins: a
            // sphere ties over a plane and over a lower-index sphere, and a sphere met again in a later cell (same key) changes
            // nothing. One 64-bit compare where round 3-4 had a 32-bit one that gave ties to the object met first.
            uint64_t key = ((uint64_t)__builtin_bit_cast(uint32_t, tMax) << 32) | (uint32_t)~best;
            uint32_t nidBase = ~(uint32_t)(np + 1);
            asm volatile("" : "+v"(nidBase)); // (one v_sub per item: left to itself the compiler re-derives -(np + i) - 2 in three)
            for (uint32_t k = k0; k < e; k++) {
                KAJO_COUNT_TESTS(lds, 0);
                const int i = (int)gridItems[k];
                const DFloat4 s = lds.sphereHot[i];
                F3 o = f3(O.x + s.x, O.y + s.y, O.z + s.z);
                float h = dot(d, o);
                float c = __builtin_fmaf(o.x, o.x, __builtin_fmaf(o.y, o.y, __builtin_fmaf(o.z, o.z, -s.w)));
                float sq = ksqrtWalk(h * h - aT * c);
                const uint32_t klo = __builtin_bit_cast(uint32_t, (-h - sq) * iaT), khi = __builtin_bit_cast(uint32_t, (sq - h) * iaT);
                const uint32_t kth = klo < khi ? klo : khi;
                const uint64_t cand = ((uint64_t)kth << 32) | (nidBase - (uint32_t)i); // ~(np + 1 + i)
                key = cand < key ? cand : key;
            }
            tMax = __builtin_bit_cast(float, (uint32_t)(key >> 32));
            best = (int)~(uint32_t)key;
            bestT0 = tMax;
        } else
#endif
        for (uint32_t k = k0; k < e; k++) {
            KAJO_COUNT_TESTS(lds, 0);
            const int i = (int)gridItems[k];
            float ts, th;
            const bool valid = sphereCandidate<ALLT>(sc, lds, i, O, d, aT, iaT, ts, th);
            const int id = np + 1 + i;
            const bool ok = valid && !(ts < 0.0f) && (ts < tMax || (ts == tMax && id > best));
            tMax = ok ? ts : tMax;
            best = ok ? id : best;
            bestT0 = ok ? th : bestT0;
        }
        const float tExit = fminf(nx, fminf(ny, nz));
        if (tMax < tExit) // nothing in a later cell can be closer (spheres are registered with a margin)
            break;
        const bool stepX = nx <= ny && nx <= nz, stepY = !stepX && ny <= nz;
        const int left = stepX ? leftX : (stepY ? leftY : leftZ);
        if (left == 0) // the ray leaves the grid
            break;
        cell += stepX ? strideX : (stepY ? strideY : strideZ);
        leftX -= stepX ? 1 : 0;
        leftY -= stepY ? 1 : 0;
        leftZ -= (stepX || stepY) ? 0 : 1;
        nx += stepX ? dx : 0.0f;
        ny += stepY ? dy : 0.0f;
        nz += (stepX || stepY) ? 0.0f : dz;
    }
}

// GHOME: where the grid's cell lists live -- 1 in LDS, 2 in global memory (the STRICT large-scene kernel instances, which know: typed
// loads, one walk; kernel_strict.hip), 0 decided at run time (the known-answer kernels; the FAST render kernels, which carry both typed walks)
template <int GHOME, bool ALLT>
KDEV void gridWalk(const DSceneView& sc, const LdsScene& lds, F3 O, F3 d, float aT, float iaT, float& tMax, int& best, float& bestT0)
{
    if (GHOME == 1) {
        gridWalkIn<ALLT>(sc, lds, lds.gridCellStartLds, lds.gridItemsLds, O, d, aT, iaT, tMax, best, bestT0);
        return;
    }
    if (GHOME == 2) {
        gridWalkIn<ALLT>(sc, lds, sc.grid.cellStart, sc.grid.items, O, d, aT, iaT, tMax, best, bestT0);
        return;
    }
#if KAJO_STRICT
    // (the known-answer kernels: one instance over a pointer of either home -- flat loads; a second instance costs 20 more spilled registers)
    gridWalkIn<ALLT>(sc, lds, sc.grid.inLds ? lds.gridCellStartLds : sc.grid.cellStart, sc.grid.inLds ? lds.gridItemsLds : sc.grid.items, O, d, aT, iaT, tMax,
               best, bestT0);
#else
    if (sc.grid.inLds) // (wave-uniform) LDS reads
        gridWalkIn<ALLT>(sc, lds, lds.gridCellStartLds, lds.gridItemsLds, O, d, aT, iaT, tMax, best, bestT0);
    else // global loads
        gridWalkIn<ALLT>(sc, lds, sc.grid.cellStart, sc.grid.items, O, d, aT, iaT, tMax, best, bestT0);
#endif
}

// hasRay: the lane has a ray to trace. Lanes without one (holding a vertex, done) go through the motions of the every-object walk
// -- it is the same instructions for the whole wave either way -- but must NOT set out on a grid walk with whatever their ray
// registers hold: a wave walks as long as its longest lane.
// LISTS_SCENE: the scene is known to have visibility lists -- and so (stage.cpp buildShadowLists / buildGrid) a closed room, the grid, rigid
// planes and nothing but (centre, radius) spheres: the kernel instances of such scenes carry one plane loop and the grid walk, nothing else.
// SIMPLE: the scene is known to have rigid planes and nothing but (centre, radius) spheres (launch.inc.hip picks the kernel): a small-scene
// kernel instantiated with it carries one plane loop and one sphere loop (kernel_exact_simple.cpp); every other scene runs the kernels
// that carry the general loops beside them.
// NP, NS >= 0 (SIMPLE instances only): the scene has NP planes and NS spheres, known when the kernel was compiled (launch.inc.hip picks it
// by the handle's counts, fixed_counts.h): the SIMPLE STRICT / EXACT walk is then straight-line code (KAJO_FIXED_UNROLL) -- no counter,
// compare or branch per primitive, hit ids that are literals, record reads at constant offsets that can be issued ahead of their use.
// The same operations on the same operands in the same order. -1: the counts are read at run time.
template <bool GRID, int GHOME = 0, bool LISTS_SCENE = false, bool SIMPLE = false, int NP = -1, int NS = -1>
KDEV Hit trace(const DSceneView& sc, const LdsScene& lds, F3 O, F3 d, bool hasRay = true)
{
    static_assert((NP < 0 && NS < 0) || (NP >= 0 && NS >= 0 && SIMPLE && KAJO_STRICT), "compile-time counts: the SIMPLE STRICT / EXACT walk only");
    float tMax = __builtin_inff(); // Ray.cpp:10-13; minDistance = 0
    int best = 0;
    float bestT0 = 0.0f;

    const int np = NP >= 0 ? NP : sc.nPlanes;
#if !KAJO_STRICT
    // FAST selection arithmetic. On gfx950 compares, selects and min/max issue at half the rate of
    // FMA/ADD/MUL/integer add (tools/valu_rate.hip), so the closest-hit bookkeeping is kept to one compare
    // and two selects per primitive: for t >= 0 the bit pattern of a float orders like the float, while
    // negative values and NaNs are patterns above +inf -- `bits(t) <= bits(tMax)` is "0 <= t <= tMax, not
    // NaN" in one unsigned compare. The running index lives in a VGPR (an SGPR source operand halves the
    // issue rate as well).
    uint32_t kMax = 0x7f800000u; // +inf
    uint32_t idV = 1;
    asm volatile("" : "+v"(idV));
    if (LISTS_SCENE || SIMPLE || sc.planesRigid) {
        // |det - 1| <= 2^-20 for every plane: t * det is t to within its own rounding, and the
        // second sign test repeats the first
        for (int i = 0; i < np; i++) {
            const DFloat4 r = lds.planeRow[i];
            float denom = r.x * d.x + r.y * d.y + r.z * d.z;
            float oy = __builtin_fmaf(r.x, O.x, __builtin_fmaf(r.y, O.y, __builtin_fmaf(r.z, O.z, r.w))); // (three FMAs: the offset starts the chain)
            // (+ 0.0f: an origin exactly ON the plane gives t = -0.0 for one sign of denom, which the reference accepts --
            // `t < 0` is false, Raytracer.cpp:85-86,115 -- while its bit pattern would sort above +inf; x + (+0) turns -0
            // into +0 and leaves every other value as it is, and rides on the multiply as one FMA)
            const uint32_t kt = __builtin_bit_cast(uint32_t, __builtin_fmaf(-oy, krcp(denom), 0.0f));
            bool ok = !(__builtin_fabsf(denom) < kFltEpsilon) && kt <= kMax;
            kMax = ok ? kt : kMax;
            best = ok ? (int)idV : best;
            idV += 1;
        }
        tMax = __builtin_bit_cast(float, kMax);
    } else
#endif
#if KAJO_STRICT
    if (LISTS_SCENE || SIMPLE || sc.planesRigid) {
        // Every determinant within 2^-20 of 1 (all of the reference's data/ scenes: rotations and translations): t * det has the sign
        // of t -- a positive factor cannot make a product negative, and -0 stays -0, which `< 0` does not hold for either -- so
        // Raytracer.cpp:115's `t < ray.min` repeats :85-86's `t < 0` and is not asked again. The same t, the same t * det.
        KAJO_FIXED_UNROLL
        for (int i = 0; i < np; i++) {
            const DFloat4 r = lds.planeRow[i];
            const float det = lds.planeDet[i];
            float denom = r.x * d.x + r.y * d.y + r.z * d.z;
            float oy = r.x * O.x + r.y * O.y + r.z * O.z + r.w * 1.0f;
            float t = kdiv(-oy, denom);
            float ts = t * det;
            bool ok = !(__builtin_fabsf(denom) < kFltEpsilon) && !(t < 0.0f) && !(ts > tMax);
            tMax = ok ? ts : tMax;
            best = ok ? i + 1 : best;
        }
    } else
#endif
    for (int i = 0; i < np; i++) { // Raytracer.cpp:74-98; only row y of the inverse matters
        const DFloat4 r = lds.planeRow[i];
        const float det = lds.planeDet[i];
        float denom = r.x * d.x + r.y * d.y + r.z * d.z;
        float oy = r.x * O.x + r.y * O.y + r.z * O.z + r.w * 1.0f;
        // (Round 2 skipped the correctly rounded division for waves whose rays all have the plane behind them or parallel. The
        // test -- ten instructions per plane, and a scalar branch that keeps the loop from being unrolled -- cost more than the
        // division it saved on all but the first camera rays: without it STRICT runs 6.4 % faster. The spheres' skip, one
        // ballot on `discriminant < 0`, stays: removing it loses 6 %.)
        float t = kdiv(-oy, denom);
        float ts = t * det;
        bool ok = !(__builtin_fabsf(denom) < kFltEpsilon) && !(t < 0.0f) && !(ts > tMax || ts < 0.0f);
        tMax = ok ? ts : tMax;
        best = ok ? i + 1 : best;
    }

    const int ns = NS >= 0 ? NS : sc.nSpheres;
    const float aT = dot(d, d); // a of every translated sphere (mat3(inverse) = identity)
#if !KAJO_STRICT
    const float iaT = krcp(aT);
#else
    const float iaT = 0.0f;
#endif
    if (GRID && (LISTS_SCENE || sc.grid.enabled)) {
#if KAJO_STRICT
        // A ray that is not a number (a light sample whose square root went negative, Light.cpp:43-46; the Phong frame of a
        // reflection along z, BSDF.cpp:52-54): in the reference's walk every comparison with NaN is false, so every object is
        // "accepted" and the LAST one wins (Raytracer.cpp:115,131-132). The every-object walk below does that by itself; the grid
        // walk has to be told.
        if (!(aT == aT) && ns > 0)
            return Hit{np + ns, aT, aT};
#endif
        // The grid's margins are sized for rays that start within `reach` of the spheres' centre (device_scene.h DGrid: what
        // rounding lets the reference's test report as a hit grows with |O - c|^2). A ray from farther out -- a vertex far away on
        // an open floor; never in a closed room -- takes its wave to the every-sphere loop below, which needs no margin.
        // (reach2 = 3e38 -- the closed room of every scene in the reference's data/ -- skips the test: a scalar branch)
        bool anyFar = false;
        if (!LISTS_SCENE && sc.grid.reach2 < 1e38f) {
            const DFloat4 gc = lds.gridHeader[4];
            const float fx = O.x - gc.x, fy = O.y - gc.y, fz = O.z - gc.z;
            anyFar = __builtin_amdgcn_ballot_w64(hasRay && !(fx * fx + fy * fy + fz * fz <= gc.w)) != 0ull;
        }
        if (!anyFar) {
            if (hasRay)
                gridWalk<GHOME, LISTS_SCENE>(sc, lds, O, d, aT, iaT, tMax, best, bestT0);
            return Hit{best, tMax, bestT0};
        }
    }
#if !KAJO_STRICT
    if (SIMPLE || sc.allTranslated) {
        // every sphere is (centre, radius): a = d.d is one value per ray and the two roots are
        // (-h -+ sqrt(h^2 - a c)) / a. The walk compares a * t (the division is done once, for the winner);
        // the smaller non-negative root is the smaller bit pattern of the two (see above: a negative root and
        // the NaN of a negative discriminant sort above every acceptable value), so "no root, both behind,
        // beyond the closest so far" is again one unsigned compare.
        const float tPlane = tMax;
        kMax = __builtin_bit_cast(uint32_t, tMax * aT);
        idV = (uint32_t)np + 1;
        asm volatile("" : "+v"(idV));
        for (int i = 0; i < ns; i++) {
            const DFloat4 s = lds.sphereHot[i];
            F3 o = f3(O.x + s.x, O.y + s.y, O.z + s.z);
            float h = dot(d, o);
            float c = __builtin_fmaf(o.x, o.x, __builtin_fmaf(o.y, o.y, __builtin_fmaf(o.z, o.z, -s.w)));
            float discr = h * h - aT * c;
            float sq = ksqrtWalk(discr);
            const uint32_t klo = __builtin_bit_cast(uint32_t, -h - sq), khi = __builtin_bit_cast(uint32_t, sq - h);
            const uint32_t kth = klo < khi ? klo : khi;
            bool ok = kth <= kMax;
            kMax = ok ? kth : kMax;
            best = ok ? (int)idV : best;
            idV += 1;
        }
        tMax = best > np ? __builtin_bit_cast(float, kMax) * iaT : tPlane;
        return Hit{best, tMax, tMax};
    }
#endif
#if KAJO_STRICT && !KAJO_IEEE_BY_COMPILER
    if (SIMPLE || sc.allTranslated) {
        // Every sphere a (centre, radius) record (all of the reference's data/ scenes): the loop of sphereCandidate's translated branch
        // with what does not depend on the sphere taken out of it -- a = d.d, -4a, and the refined reciprocal of a that kdiv(q, a)
        // forms (the same v_rcp and two FMAs on the same operand: the same value) -- and no branch on the record's kind per
        // sphere. Same operations on the same operands in the same order: the same bits (every STRICT = oracle test runs through here).
        const float m4a = -4.0f * aT; // b^2 - (4a)c == b^2 + (-(4a))c: negation is exact
        float y = __builtin_amdgcn_rcpf(aT);
        y = __builtin_fmaf(__builtin_fmaf(-aT, y, 1.0f), y, y);
        KAJO_FIXED_UNROLL
        for (int i = 0; i < ns; i++) { // Raytracer.cpp:21-72
            const DFloat4 s = lds.sphereHot[i];
            const F3 o = f3(O.x + s.x, O.y + s.y, O.z + s.z);
            const float h = dot(d, o);
            const float c = dot(o, o) - s.w;
            const float b = 2 * h;
            const float discr = b * b + m4a * c;
            if (__builtin_amdgcn_ballot_w64(!(discr < 0.0f)) == 0ull) // (no ray of the wave reaches this sphere's line: see sphereCandidate)
                continue;
            const float sq = ksqrtWalk(discr);
            const float q = (b < 0.0f) ? (-b - sq) * .5f : (-b + sq) * .5f;
            float t0 = q * y; // q / a, kdiv's sequence on the shared reciprocal
            float r = __builtin_fmaf(-aT, t0, q);
            t0 = __builtin_fmaf(r, y, t0);
            r = __builtin_fmaf(-aT, t0, q);
            t0 = __builtin_amdgcn_div_fixupf(__builtin_fmaf(r, y, t0), aT, q);
            const float t1 = kdiv(c, q);
            const bool sw = t0 > t1;
            const float lo = sw ? t1 : t0, hi = sw ? t0 : t1;
            const float th = (lo < 0.0f) ? hi : lo; // (* determinant: exactly 1)
            // (Raytracer.cpp:115's `t < ray.min` asks nothing new here: th is lo unless lo is negative, and then it is hi, which the test
            // before it found not negative; a NaN answers false to all of them either way)
            const bool ok = !(discr < 0.0f) && !(hi < 0.0f) && !(th > tMax);
            tMax = ok ? th : tMax;
            best = ok ? np + 1 + i : best;
            bestT0 = ok ? th : bestT0;
        }
        return Hit{best, tMax, bestT0};
    }
#endif
    for (int i = 0; i < ns; i++) { // Raytracer.cpp:21-72
        float ts, th;
        bool ok = sphereCandidate(sc, lds, i, O, d, aT, iaT, ts, th) && !(ts > tMax || ts < 0.0f);
        tMax = ok ? ts : tMax;
        best = ok ? np + 1 + i : best;
        bestT0 = ok ? th : bestT0;
    }
    return Hit{best, tMax, bestT0};
}

// ---- shadow query through the light's visibility lists (large scenes) ------------------------------
// Raytracer::canReach (Raytracer.cpp:140-144): is the closest hit of the ray the light `si` (sphere index) it was aimed at?
// Answered from the light itself, the planes and the few spheres that come within reach of the segment light centre ..
// ray origin (device_scene.h DShadowLists) instead of a closest-hit walk of the grid. Every test is the closest-hit walk's own
// arithmetic; the walk's acceptance (Raytracer.cpp:115: reject only t > max, objects in scene order, so the closest wins and
// among equal distances the later object) is applied in its order-independent form: something beats the light iff its
// distance is smaller, or equal with a later index. Planes precede every sphere, so a plane must be strictly closer.
// The part of the query every lane does for its own ray: the light itself and the planes. false: the light is not hit at all, or a
// plane lies in front of it. `keyL`: the light's distance in the form the item tests compare against (STRICT: the float ts; FAST: its
// bit pattern, trace()).
KDEV bool lightReachedHead(const DSceneView& sc, const LdsScene& lds, int lightK, int si, F3 O, F3 d, uint32_t& keyL)
{
    const int np = sc.nPlanes;
    const float aT = dot(d, d);
#if KAJO_STRICT
    if (!(aT == aT)) { // a ray that is not a number: the reference's poisoned walk ends on the LAST object (see trace()); no test below blocks
        keyL = 0x7fc00000u;
        return si == sc.nSpheres - 1;
    }
    float tsL, thL;
    if (!sphereCandidate<true>(sc, lds, si, O, d, aT, 0.0f, tsL, thL) || tsL < 0.0f)
        return false;
    keyL = __builtin_bit_cast(uint32_t, tsL);
    // A plane that has the ray's origin AND the light's whole ball strictly on one side (by margins far above the rounding of
    // these sums) is crossed, if at all, behind the origin or beyond the ball: its test cannot come out "hit before the light".
    // The rays of a wave mostly agree on that (a room: everything is inside), so the rest of the test is skipped per wave.
    const float tolO = 1e-3f + 1e-5f * (__builtin_fabsf(O.x) + __builtin_fabsf(O.y) + __builtin_fabsf(O.z));
    bool blocked = false;
    for (int i = 0; i < np; i++) { // Raytracer.cpp:74-98, as in trace()
        const DFloat4 r = lds.planeRow[i];
        float oy = r.x * O.x + r.y * O.y + r.z * O.z + r.w * 1.0f;
        if (__builtin_amdgcn_ballot_w64(!(oy * lds.lightPlaneSide[lightK * np + i] > tolO + 1e-5f * __builtin_fabsf(r.w))) == 0ull)
            continue;
        const float det = lds.planeDet[i];
        float denom = r.x * d.x + r.y * d.y + r.z * d.z;
        float t = kdiv(-oy, denom);
        float ts = t * det;
        blocked = blocked || (!(__builtin_fabsf(denom) < kFltEpsilon) && !(t < 0.0f) && !(ts < 0.0f) && ts < tsL);
    }
    return !blocked;
#else
    const float iaT = krcp(aT);
    uint32_t kL;
    {
        const DFloat4 s = lds.sphereHot[si];
        F3 o = f3(O.x + s.x, O.y + s.y, O.z + s.z);
        float h = dot(d, o);
        float c = __builtin_fmaf(o.x, o.x, __builtin_fmaf(o.y, o.y, __builtin_fmaf(o.z, o.z, -s.w)));
        float sq = ksqrtWalk(h * h - aT * c);
        const uint32_t klo = __builtin_bit_cast(uint32_t, (-h - sq) * iaT), khi = __builtin_bit_cast(uint32_t, (sq - h) * iaT);
        kL = klo < khi ? klo : khi; // the smaller non-negative root; a negative root or NaN sorts above +inf (trace())
    }
    keyL = kL;
    if (kL > 0x7f800000u)
        return false;
    const float tolO = 1e-3f + 1e-5f * (__builtin_fabsf(O.x) + __builtin_fabsf(O.y) + __builtin_fabsf(O.z)); // (see the STRICT twin above)
    bool blocked = false;
    for (int i = 0; i < np; i++) {
        const DFloat4 r = lds.planeRow[i];
        float oy = __builtin_fmaf(r.x, O.x, __builtin_fmaf(r.y, O.y, __builtin_fmaf(r.z, O.z, r.w)));
        if (__builtin_amdgcn_ballot_w64(!(oy * lds.lightPlaneSide[lightK * np + i] > tolO + 1e-5f * __builtin_fabsf(r.w))) == 0ull)
            continue;
        float denom = r.x * d.x + r.y * d.y + r.z * d.z;
        // (the lists are built with the grid, which needs every plane rigid: trace()'s rigid-plane form)
        const uint32_t kt = __builtin_bit_cast(uint32_t, __builtin_fmaf(-oy, krcp(denom), 0.0f));
        blocked = blocked || (!(__builtin_fabsf(denom) < kFltEpsilon) && kt < kL);
    }
    return !blocked;
#endif
}

// Does sphere i lie in front of light `si` along the ray? The closest-hit walk's own sphere arithmetic; "in front" by the walk's
// rule in its order-independent form (closer, or as close with a later index).
KDEV bool shadowItemBlocks(const DSceneView& sc, const LdsScene& lds, int i, int si, F3 O, F3 d, float aT, float iaT, uint32_t keyL)
{
#if KAJO_STRICT
    float ts, th;
    const bool valid = sphereCandidate<true>(sc, lds, i, O, d, aT, 0.0f, ts, th);
    const float tsL = __builtin_bit_cast(float, keyL);
    return valid && !(ts < 0.0f) && (ts < tsL || (ts == tsL && i > si));
#else
    const DFloat4 s = lds.sphereHot[i];
    F3 o = f3(O.x + s.x, O.y + s.y, O.z + s.z);
    float h = dot(d, o);
    float c = __builtin_fmaf(o.x, o.x, __builtin_fmaf(o.y, o.y, __builtin_fmaf(o.z, o.z, -s.w)));
    float sq = ksqrtWalk(h * h - aT * c);
    const uint32_t klo = __builtin_bit_cast(uint32_t, (-h - sq) * iaT), khi = __builtin_bit_cast(uint32_t, (sq - h) * iaT);
    const uint32_t kth = klo < khi ? klo : khi;
    return kth < keyL || (kth == keyL && i > si);
#endif
}

// The bin of the light's cube map that u = O - C falls into -- as (row of bins, bin in the row): DShadowLists -- and how far from the
// light's centre the ray reaches, in the units of the light's quantised keys, rounded UP.
KDEV uint32_t shadowBin(const DSceneView& sc, const DSphereCold& lc, int lightK, float invKeyScale, F3 O, uint32_t& binInRow, uint32_t& reachQ)
{
    const F3 u = f3(O.x - lc.cx, O.y - lc.cy, O.z - lc.cz);
    const float ax = __builtin_fabsf(u.x), ay = __builtin_fabsf(u.y), az = __builtin_fabsf(u.z);
    const int m = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float um = m == 0 ? u.x : (m == 1 ? u.y : u.z);
    const float ua = m == 0 ? u.y : (m == 1 ? u.z : u.x);
    const float ub = m == 0 ? u.z : (m == 1 ? u.x : u.y);
    // (the hardware reciprocal in both numerics modes: the bin only selects the candidate set, which is conservative by 1e-4 rad;
    // u == 0: NaN coordinates fall into cell 0 -- a sphere that close to C is in every bin)
    const float im = __builtin_amdgcn_rcpf(__builtin_fabsf(um));
    const int N = sc.shadow.n;
    const float halfN = 0.5f * (float)N;
    int ia = (int)__builtin_floorf((ua * im + 1.0f) * halfN), ib = (int)__builtin_floorf((ub * im + 1.0f) * halfN);
    ia = min(max(ia, 0), N - 1);
    ib = min(max(ib, 0), N - 1);
    const int face = 2 * m + (um < 0.0f ? 1 : 0);
    const float reach = fmaxf(__builtin_amdgcn_sqrtf(dot(u, u)), lc.radius) * 1.000002f; // (hardware root, 1 ulp, inside the factor)
    // an item is left out of the walk only if its quantised key -- a lower bound of its true key -- exceeds this: floor(x) + 1 > x
    reachQ = (uint32_t)fminf(reach * invKeyScale * 1.000001f, 65534.0f) + 1u;
    binInRow = (uint32_t)ia;
    return (uint32_t)(((lightK * 6 + face) * N) + ib);
}

// The cooperative walk of the visibility lists of one round of shadow queries (renderBody LISTS; described there). hasQ: this lane owns a
// query (ray O, d; light sphere si at distance key keyL; list items [k0, e); reach reachQ). canHelp: this lane's ray registers are dead
// -- it may take a share of another lane's list, and O, d are overwritten with that lane's. Returns, for an owner: some sphere of its
// list lies in front of the light.
KDEV bool listWalkCooperative(const DSceneView& sc, const LdsScene& lds, KajoLdsWord* helpOwner, KajoLdsWord* helpFlag, const uint32_t* items, int lane,
                              bool hasQ, bool canHelp, F3& O, F3& d, uint32_t keyL, uint32_t k0, uint32_t e, int si, uint32_t reachQ)
{
    const unsigned long long qMask = __ballot(hasQ);
    if (qMask == 0ull)
        return false;
    const unsigned long long idleMask = __ballot(!hasQ && canHelp);
    const int nQ = __builtin_popcountll(qMask);
    int G = __builtin_popcountll(idleMask) / nQ; // helpers per query
    G = G > 7 ? 7 : G;
    const unsigned long long mine = hasQ ? qMask : idleMask;
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
    if (hasQ) {
        helpOwner[rank] = (uint32_t)lane;
        helpFlag[lane] = 0u;
    }
    __builtin_amdgcn_wave_barrier();
    const bool helper = !hasQ && canHelp && rank < nQ * G;
    int ownerLane = lane, sub = 0;
    if (helper) {
        const int qr = (int)(((float)rank + 0.5f) * __builtin_amdgcn_rcpf((float)G)); // rank / G (small integers)
        sub = 1 + rank - qr * G;
        ownerLane = (int)helpOwner[qr];
    }
    const int addr = ownerLane << 2;
#define KAJO_FROM_OWNER_F(x) x = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, x)))
#define KAJO_FROM_OWNER_U(x) x = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(x))
    KAJO_FROM_OWNER_F(O.x);
    KAJO_FROM_OWNER_F(O.y);
    KAJO_FROM_OWNER_F(O.z);
    KAJO_FROM_OWNER_F(d.x);
    KAJO_FROM_OWNER_F(d.y);
    KAJO_FROM_OWNER_F(d.z);
    KAJO_FROM_OWNER_U(keyL);
    KAJO_FROM_OWNER_U(k0);
    KAJO_FROM_OWNER_U(e);
    si = (int)__builtin_amdgcn_ds_bpermute(addr, si);
    KAJO_FROM_OWNER_U(reachQ);
#undef KAJO_FROM_OWNER_F
#undef KAJO_FROM_OWNER_U
    bool blocked = false;
    if (hasQ || helper) {
        const float aT = dot(d, d);
#if KAJO_STRICT
        const float iaT = 0.0f;
#else
        const float iaT = krcp(aT);
#endif
        const uint32_t stride = (uint32_t)G + 1u;
        uint32_t j = k0 + (uint32_t)sub;
        uint32_t nxt = 0xffffffffu;
        if (j < e)
            nxt = items[j];
        while (j < e) {
            const uint32_t cur = nxt;
            j += stride;
            if (j < e)
                nxt = items[j];
            if ((cur >> 16) > reachQ) // nothing further along the list can touch the ray before it ends
                break;
            KAJO_COUNT_TESTS(lds, 1);
            if (shadowItemBlocks(sc, lds, (int)(cur & 0xffffu), si, O, d, aT, iaT, keyL)) {
                blocked = true;
                break;
            }
        }
        if (helper && blocked)
            helpFlag[ownerLane] = 1u;
    }
    __builtin_amdgcn_wave_barrier();
    return hasQ && (blocked || helpFlag[lane] != 0u); // (a helper's `blocked` is about somebody else's query)
}

// Two stages (verdict item 2b of round 5 / round 5's own note: "a round is as long as its longest list"): every owner tests the first
// KAJO_LIST_STAGE1 items of its list itself -- most queries end there, at their first blocker or at the first item beyond the ray's reach
// --, then the lanes whose queries are answered take over the rest of the lists still open, shared out by the cooperative walk above.
// 0 = the cooperative walk alone. Which lane tests an item does not change the test: the answer is the same.
#ifndef KAJO_LIST_STAGE1
#define KAJO_LIST_STAGE1 3 // measured on configs[4], 4K x 32 (profiles/r06_notes.txt): 0 -> 6 894 / 5 074 / 4 510 M paths/s FAST / EXACT / STRICT, 2 -> 7 131 / 5 117 / 4 691, 3 -> 7 160-7 212 / 5 152-5 179 / 4 660-4 690, 4 -> 7 158 / 5 155 / 4 662, 6 -> 7 112 / 5 087 / 4 576
#endif
KDEV bool listWalk(const DSceneView& sc, const LdsScene& lds, KajoLdsWord* helpOwner, KajoLdsWord* helpFlag, const uint32_t* items, int lane, bool hasQ,
                   bool canHelp, F3& O, F3& d, uint32_t keyL, uint32_t k0, uint32_t e, int si, uint32_t reachQ)
{
    if (KAJO_LIST_STAGE1 == 0)
        return listWalkCooperative(sc, lds, helpOwner, helpFlag, items, lane, hasQ, canHelp, O, d, keyL, k0, e, si, reachQ);
    bool blocked = false, open = false;
    uint32_t j = k0;
    if (hasQ) {
        const float aT = dot(d, d);
#if KAJO_STRICT
        const float iaT = 0.0f;
#else
        const float iaT = krcp(aT);
#endif
        open = true;
        uint32_t nxt = j < e ? items[j] : 0xffffffffu;
        for (int t = 0; t < KAJO_LIST_STAGE1; t++) {
            if (j >= e) {
                open = false;
                break;
            }
            const uint32_t cur = nxt;
            j++;
            if (j < e)
                nxt = items[j];
            if ((cur >> 16) > reachQ) { // nothing further along the list can touch the ray before it ends
                open = false;
                break;
            }
            KAJO_COUNT_TESTS(lds, 1);
            if (shadowItemBlocks(sc, lds, (int)(cur & 0xffffu), si, O, d, aT, iaT, keyL)) {
                blocked = true;
                open = false;
                break;
            }
        }
        open = open && j < e;
    }
    if (__ballot(open) == 0ull)
        return hasQ && blocked;
    // (a lane whose own query is answered -- or that never had one -- has dead ray registers: it may help)
    const bool rest = listWalkCooperative(sc, lds, helpOwner, helpFlag, items, lane, open, canHelp && !open, O, d, keyL, j, e, si, reachQ);
    return hasQ && (blocked || rest);
}

// ---- surface point of an accepted hit ------------------------------------------------------
struct Surface
{
    F3 P, N; // position, shading normal
};

KDEV void sphereFrame(F3 n, F3& tg, F3& bn) // Raytracer.cpp:55-65
{
    float smallest = fminf(n.z, fminf(n.x, n.y));
    F3 t;
    if (n.x == smallest)
        t = f3(0.0f, -n.z, n.y);
    else if (n.y == smallest)
        t = f3(-n.z, 0.0f, n.x);
    else
        t = f3(-n.y, n.x, 0.0f);
    tg = normalize(t);
    bn = cross(n, tg);
}

template <bool ALLT = false, int NP = -1>
KDEV F3 hitNormal(const DSceneView& sc, const LdsScene& lds, const Hit& h, F3 O, F3 d)
{
    const int np = NP >= 0 ? NP : sc.nPlanes; // (NP: trace())
    if (h.id <= np) {
        const DFloat4 n = lds.planeFrame[3 * (h.id - 1)];
        return f3(n.x, n.y, n.z);
    }
    const int si = h.id - 1 - np;
    const uint32_t off = (ALLT || sc.allTranslated) ? (uint32_t)si : lds.sphereHotOffset[si];
    if (ALLT || !(off & KAJO_SPHERE_GENERAL)) {
#if KAJO_STRICT
        const DFloat4 s = lds.sphereHot[off];
        F3 o = f3(O.x + s.x, O.y + s.y, O.z + s.z);
        return normalize(o + d * h.t0); // mat3(M) = identity
#else
        // the hit point minus the centre has length r: scale instead of normalising; (-centre, r^2) is the hot record
        // itself (in LDS for every scene size), 1 / r its reciprocal square root
        const DFloat4 s = lds.sphereHot[off];
        F3 o = f3(O.x + s.x, O.y + s.y, O.z + s.z);
        return (o + d * h.t0) * krsq(s.w);
#endif
    }
    const int k = (int)(off & ~KAJO_SPHERE_GENERAL);
    const DFloat4 r0 = lds.sphereHot[k], r1 = lds.sphereHot[k + 1], r2 = lds.sphereHot[k + 2];
    F3 dir = f3(r0.x * d.x + r0.y * d.y + r0.z * d.z, r1.x * d.x + r1.y * d.y + r1.z * d.z,
                r2.x * d.x + r2.y * d.y + r2.z * d.z);
    F3 o = f3(r0.x * O.x + r0.y * O.y + r0.z * O.z + r0.w * 1.0f, r1.x * O.x + r1.y * O.y + r1.z * O.z + r1.w * 1.0f,
              r2.x * O.x + r2.y * O.y + r2.z * O.z + r2.w * 1.0f);
    F3 n = o + dir * h.t0;
    const float* m = lds.sphereCold[si].m;
    return normalize(f3(m[0] * n.x + m[1] * n.y + m[2] * n.z, m[3] * n.x + m[4] * n.y + m[5] * n.z,
                        m[6] * n.x + m[7] * n.y + m[8] * n.z));
}

// ---- BSDFs (BSDF.cpp). kind: 0 Lambert, 1 Phong, 2 ideal reflector ----------------------------
KDEV F3 bsdfEvaluate(int kind, F3 color, float exponent, F3 R, F3 N, F3 dir)
{
    if (kind == 0) { // BSDF.cpp:30-33
#if KAJO_RSTRICT
        return color * (float)kInvPi;
#else
        return color * kInvPiF;
#endif
    }
    if (kind == 1) { // BSDF.cpp:62-67
        float cosA = kmax0(rdot(R, dir));
#if KAJO_RSTRICT
        float s = (float)((double)(exponent + 1) / (2 * kPi));
#else
        float s = (exponent + 1) * kInv2PiF;
#endif
        return (s * color) * kpowPhong(cosA, exponent);
    }
    float cosA = kmax0(dot(dir, N)); // BSDF.cpp:87-91 (an exact zero makes the value infinite, and inf * 0 a NaN pixel the oracle has too: not rdot)
#if KAJO_RSTRICT
    return f3(kdiv(color.x, cosA), kdiv(color.y, cosA), kdiv(color.z, cosA));
#else
    return color * rrcp(cosA);
#endif
}

KDEV float bsdfProbability(int kind, float exponent, F3 R, F3 N, F3 dir)
{
    if (kind == 0) { // BSDF.cpp:35-39
        float cosT = dot(dir, N);
#if KAJO_RSTRICT
        return (float)(kInvPi * (double)cosT);
#else
        return kInvPiF * cosT;
#endif
    }
    if (kind == 1) { // BSDF.cpp:69-74
        float cosA = kmax0(rdot(R, dir));
#if KAJO_RSTRICT
        return (float)((double)(exponent + 1) / (2 * kPi) * (double)kpowPhong(cosA, exponent));
#else
        return (exponent + 1) * kInv2PiF * kpowPhong(cosA, exponent);
#endif
    }
    return 0.0f; // BSDF.cpp:93-96
}

// evaluate() and probability() toward the same direction (Shader.cpp:74-80): the Phong power is formed once.
// A zero pdf (always for the reflector) discards the sample, so no value is computed for it.
KDEV F3 bsdfEvaluateWithPdf(int kind, F3 color, float exponent, F3 R, F3 N, F3 dir, float& pdf)
{
    if (kind == 1) { // BSDF.cpp:62-74
        const float pw = kpowPhong(kmax0(rdot(R, dir)), exponent);
#if KAJO_RSTRICT
        pdf = (float)((double)(exponent + 1) / (2 * kPi) * (double)pw);
        const float s = (float)((double)(exponent + 1) / (2 * kPi));
#else
        const float s = (exponent + 1) * kInv2PiF;
        pdf = s * pw;
#endif
        return (s * color) * pw;
    }
    if (kind == 0) {
        pdf = bsdfProbability(0, exponent, R, N, dir);
        return bsdfEvaluate(0, color, exponent, R, N, dir);
    }
    pdf = 0.0f;
    return f3(0.0f, 0.0f, 0.0f);
}

// generateSample of Lambert / Phong / reflector (BSDF.cpp:20-28,48-60,82-85 with
// Random.cpp:77-102). tg/bn only read for Lambert.
// `value` = evaluate() toward the generated direction (Shader.cpp:203). FAST forms the Phong value from the
// power the pdf already needed: cos(angle to R) of the generated direction IS the sampled cosine, and
// log2 of it is the exponent argument that produced it.
KDEV F3 bsdfGenerate(int kind, F3 color, float exponent, F3 R, F3 N, F3 tg, F3 bn, Rng& rng, float& pdf, F3& value)
{
    if (kind == 2) {
        pdf = 1.0f;
        value = bsdfEvaluate(2, color, exponent, R, N, R);
        return R;
    }
    rngStep(rng);
    float u = unitBits((uint32_t)rng.lo);         // .5f * x + .5f
    float v = unitBits((uint32_t)(rng.lo >> 32));
    if (kind == 0) {
        float r = ksqrt(u);
#if KAJO_STRICT
        float phi = (float)((double)(v * 2) * kPi);
        float sphi, cphi;
        kajo_sincosf(phi, &sphi, &cphi);
        float x = r * cphi;
        float y = r * sphi;
        float z = ksqrt(fmaxf(0.0f, 1.0f - u));
#if KAJO_RSTRICT
        pdf = (float)((double)z * kInvPi);
#else
        pdf = z * kInvPiF; // (zero exactly when z is: the path ends on the same draw)
#endif
#else
        float x = r * __builtin_amdgcn_cosf(v); // v_cos_f32 takes revolutions: cos(2 pi v)
        float y = r * __builtin_amdgcn_sinf(v);
        float z = ksqrt(kmax0(1.0f - u));
        pdf = z * kInvPiF;
#endif
        value = bsdfEvaluate(0, color, exponent, R, N, N);
        return tg * x + bn * y + N * z;
    }
    F3 s;
#if KAJO_STRICT
    float a = kajo_acosf(kajo_powf(u, kdiv(1.0f, exponent + 1)));
    float phi = (float)(2 * kPi * (double)v);
    float sa, ca, sphi, cphi;
    kajo_sincosf(a, &sa, &ca);
    kajo_sincosf(phi, &sphi, &cphi);
    s = f3(sa * cphi, sa * sphi, ca);
#if KAJO_RSTRICT
    pdf = (float)((double)(exponent + 1) / (2 * kPi) * (double)kajo_powf(ca, exponent));
#else
    {
        // EXACT: the direction above is the oracle's; its pdf and the lobe's value toward it are the FAST forms over the oracle's
        // cosine (cos of the angle to R of the generated direction IS the sampled cosine). Whether the pdf is ZERO is a decision
        // (Shader.cpp:198-199: the path ends): the power can only vanish when the variate is 0 exactly -- the cosine is
        // u^(1/(e+1)) >= 2^-32 otherwise and its e-th power at least 2^-32 -- and that draw (one in 2^32) takes the oracle's power.
        float pw = kpowPhong(ca, exponent);
#ifndef KAJO_X_NOPOWFALLBACK
        if (u == 0.0f)
            pw = kajo_powf(ca, exponent);
#endif
        const float sc = (exponent + 1) * kInv2PiF;
        pdf = sc * pw;
        value = (sc * color) * pw;
    }
#endif
#else
    // cos(acos(c)) = c and sin(acos(c)) = sqrt(1 - c^2): no inverse trigonometry needed
    const float lca = __builtin_amdgcn_logf(u) * krcp(exponent + 1); // log2 of the sampled cosine
    float ca = __builtin_amdgcn_exp2f(lca);
    float sa = ksqrt(kmax0(1.0f - ca * ca));
    s = f3(sa * __builtin_amdgcn_cosf(v), sa * __builtin_amdgcn_sinf(v), ca);
    const float pw = __builtin_amdgcn_exp2f(exponent * lca); // ca ^ exponent
    const float sc = (exponent + 1) * kInv2PiF;
    pdf = sc * pw;
    value = (sc * color) * pw;
#endif
#if KAJO_STRICT
    F3 uu = normalize(cross(f3(0.0f, 0.0f, 1.0f), R));
    F3 vv = cross(uu, R);
#else
    // cross((0,0,1), R) = (-R.y, R.x, 0), written out: the products with the zeros are not folded otherwise
    const float iu = krsq(R.x * R.x + R.y * R.y);
    F3 uu = f3(-R.y * iu, R.x * iu, 0.0f);
    F3 vv = f3(uu.y * R.z, -(uu.x * R.z), uu.x * R.y - R.x * uu.y);
#endif
    const F3 nd = f3(uu.x * s.x + vv.x * s.y + R.x * s.z, uu.y * s.x + vv.y * s.y + R.y * s.z,
                     uu.z * s.x + vv.z * s.y + R.z * s.z);
#if KAJO_RSTRICT
    value = bsdfEvaluate(1, color, exponent, R, N, nd);
#endif
    return nd;
}

// IdealTransmissionBSDF::generateSample, BSDF.cpp:105-124 + glm::refract
KDEV F3 transmissionDirection(F3 view, F3 N, float ior)
{
    float cosA = dot(view, N);
    bool entering = cosA < 0.0f;
    F3 n = entering ? N : -N;
    float eta = entering ? kdiv(1.0f, ior) : kdiv(ior, 1.0f);
    cosA = dot(view, n);
    float k = 1.0f - eta * eta * (1.0f - cosA * cosA);
    if (k < 0.0f)
        return reflect(view, n);
    float dv = dot(n, view);
    return eta * view - (eta * dv + ksqrt(k)) * n;
}

// ---- SphericalLight (Light.cpp:26-62) -------------------------------------------------------
KDEV float solidAngle(F3 centre, float radius, F3 P)
{
    float dist = length(centre - P);
#if KAJO_STRICT
    if (dist < radius)
        return (float)(4 * kPi);
    return (float)(2 * kPi * (double)(1 - kajo_cosf(kajo_asinf(kdiv(radius, dist)))));
#else
    // 1 - cos(asin x) = x^2 / (1 + sqrt(1 - x^2)): same value without the cancellation
    float x = radius * krcp(dist);
    float x2 = x * x;
    float v = 6.28318530717958647692f * x2 * krcp(1.0f + ksqrt(kmax0(1.0f - x2)));
    return dist < radius ? 12.56637061435917295385f : v;
#endif
}

#if !KAJO_RSTRICT
// 1 / solidAngle without forming the angle: with x = r / dist,
// 1 / (2 pi (1 - cos asin x)) = (1 + sqrt(1 - x^2)) / (2 pi x^2) = (1 + sqrt(1 - r^2/d^2)) d^2 / (2 pi r^2)
KDEV float lightPdf(const DSphereCold& lc, F3 P)
{
    F3 v = f3(lc.cx - P.x, lc.cy - P.y, lc.cz - P.z);
    float d2 = rdot(v, v);
    float r2 = lc.radius * lc.radius;
    float x2 = r2 * rrcp(d2);
    float p = (1.0f + __builtin_amdgcn_sqrtf(kmax0(1.0f - x2))) * d2 * lc.invTwoPiR2;
    return d2 < r2 ? 0.07957747154594767f : p; // inside the light: 1 / (4 pi)
}
#endif

// SphericalLight::generateSample (Light.cpp:39-49) from its three uniform variates
KDEV F3 lightDirection(F3 centre, float radius, F3 P, float s1, float s2, float s3, float& pdf)
{
#if KAJO_STRICT
    float ang = (float)(2 * kPi * (double)s2);
    float sang, cang;
    kajo_sincosf(ang, &sang, &cang);
    float x = radius * ksqrt(s1) * cang;
    float y = radius * ksqrt(s1) * sang;
    float z = ksqrt(radius * radius - x * x - y * y) * kajo_sinf((float)(kPi * (double)(s3 - .5f)));
#else
    float rs = radius * ksqrt(s1);
    float x = rs * __builtin_amdgcn_cosf(s2);
    float y = rs * __builtin_amdgcn_sinf(s2);
    float z = ksqrt(radius * radius - x * x - y * y) * __builtin_amdgcn_sinf((s3 - .5f) * .5f);
#endif
    F3 dir = normalize(centre + f3(x, y, z) - P);
#if KAJO_RSTRICT
    pdf = krcp(solidAngle(centre, radius, P));
#endif
    return dir;
}

KDEV F3 lightGenerate(F3 centre, float radius, F3 P, Rng& rng, float& pdf)
{
    rngStep(rng);
    const float s1 = unitBits((uint32_t)rng.lo), s2 = unitBits((uint32_t)(rng.lo >> 32)), s3 = unitBits((uint32_t)rng.hi);
    return lightDirection(centre, radius, P, s1, s2, s3, pdf);
}

// ---- path state ---------------------------------------------------------------------------
enum : int
{
    MODE_NEW = 0,    // fetch the next camera path of this lane's pixel
    MODE_EXTEND = 1, // the traced ray continues the path: shade what it hit
    MODE_SHADOW = 2, // the traced ray asks whether light `lightK` is visible
    MODE_DONE = 3,
    MODE_HOLD = 4    // the vertex waits for a trip in which the light / BSDF sampling blocks run (RenderArgs::thrL)
};

} // namespace

// Register budgets (launch bounds). Throughput follows the number of resident waves almost linearly (profiles/r03_deferred_experiment.txt,
// sweep 3: 2 / 3 / 4 waves per SIMD -> 23.3 / 29.7 / 38.5 G paths/s), so the FAST loop is kept within 96 VGPRs = 5 waves per SIMD
// (kernel_fast.hip); STRICT and the large-scene kernels need 128.
#ifndef KAJO_WAVES_PER_SIMD
#define KAJO_WAVES_PER_SIMD 4 // 512 / 4 = 128 VGPRs per lane
#endif
#ifndef KAJO_WAVES_PER_SIMD_BIG
#define KAJO_WAVES_PER_SIMD_BIG 4
#endif
#ifndef KAJO_INLINE_SHADOW
#define KAJO_INLINE_SHADOW 0
#endif
#ifndef KAJO_LISTS_TILE_RMW
#define KAJO_LISTS_TILE_RMW 0
#endif
#ifndef KAJO_ANY_LANE_GIVES
#define KAJO_ANY_LANE_GIVES 1 // 0: only lanes that are themselves between two paths in this trip can give a pass away (rounds 2-5)
#endif
#ifndef KAJO_LISTS_BALANCED
#define KAJO_LISTS_BALANCED 1 // 0: the light loop of rounds 4 (one vertex per lane), for A/B runs
#endif
#if KAJO_STRICT
#define KAJO_IS_A_NUMBER(x) ((x) == (x))
#else
#define KAJO_IS_A_NUMBER(x) true
#endif

namespace
{

// Workgroup-cooperative copy of `count` 16-byte records into LDS.
KDEV void stage16(DFloat4* dst, const void* src, int count)
{
    const DFloat4* s = static_cast<const DFloat4*>(src);
    for (int i = threadIdx.x; i < count; i += blockDim.x)
        dst[i] = s[i];
}

// COLD_LDS (small scenes): shading frames, sphere centres, materials and the light list are staged
// into LDS next to the hot records and every sphere is tested. !COLD_LDS (large scenes): the cold
// records are read from global memory (L2) and the spheres are reached through the uniform grid.
// NP, NS >= 0: the scene's plane and sphere counts, known when the kernel was compiled (trace(): such a scene is a SIMPLE one, every
// sphere one hot record) -- the arrays behind the hot records then lie at constant offsets.
template <bool COLD_LDS, int NP = -1, int NS = -1>
KDEV LdsScene stageToLds(const DSceneView& sc, unsigned char* ldsRaw)
{
    const int np = NP >= 0 ? NP : sc.nPlanes, ns = NS >= 0 ? NS : sc.nSpheres;
    const int nSphereHot = NS >= 0 ? NS : sc.nSphereHot;
    // layout: [planeRow np x16][sphereHot nHot x16]{[planeFrame 3np x16][sphereCold ns x64]
    //         [material (np+ns) x96]}[planeDet np x4][sphereHotOffset ns x4][light nL x4] (pad to 16)
    //         [lightCold nL x64][lightEmission nL x16][lightPlaneSide nL*np x4 (pad to 16)][camera 8 x16]{[grid header 4 x16][grid cell starts][grid items]}
    DFloat4* ldsPlaneRow = reinterpret_cast<DFloat4*>(ldsRaw);
    DFloat4* ldsSphereHot = ldsPlaneRow + np;
    DFloat4* cursor = ldsSphereHot + nSphereHot;
    stage16(ldsPlaneRow, sc.planeRow, np);
    stage16(ldsSphereHot, sc.sphereHot, nSphereHot);
    LdsScene lds;
#ifdef KAJO_COUNT_SPHERE_TESTS
    lds.testCounter = nullptr;
#endif
    lds.planeRow = ldsPlaneRow;
    lds.sphereHot = ldsSphereHot;
    if (COLD_LDS) {
        DFloat4* f = cursor;
        DFloat4* c = f + 3 * np;
        DFloat4* m = c + 4 * ns;
        cursor = m + 6 * (np + ns);
        stage16(f, sc.planeFrame, 3 * np);
        stage16(c, sc.sphereCold, 4 * ns);
        stage16(m, sc.material, 6 * (np + ns));
        lds.planeFrame = f;
        lds.sphereCold = reinterpret_cast<const DSphereCold*>(c);
        lds.material = reinterpret_cast<const DMaterial*>(m);
    } else {
        lds.planeFrame = sc.planeFrame;
        lds.sphereCold = sc.sphereCold;
        lds.material = sc.material;
    }
    float* ldsPlaneDet = reinterpret_cast<float*>(cursor);
    uint32_t* ldsSphereOff = reinterpret_cast<uint32_t*>(ldsPlaneDet + np);
    const int nOff = sc.allTranslated ? 0 : ns; // (every sphere a (centre, radius) record: its offset is its index, nothing to look up)
    int32_t* ldsLight = reinterpret_cast<int32_t*>(ldsSphereOff + nOff);
    for (int i = threadIdx.x; i < np; i += blockDim.x)
        ldsPlaneDet[i] = sc.planeDet[i];
    for (int i = threadIdx.x; i < nOff; i += blockDim.x)
        ldsSphereOff[i] = sc.sphereHotOffset[i];
    for (int i = threadIdx.x; i < sc.nLights; i += blockDim.x)
        ldsLight[i] = sc.light[i];
    lds.planeDet = ldsPlaneDet;
    lds.sphereHotOffset = ldsSphereOff;
    lds.light = ldsLight;
    // the lights' records, by light index: [lightCold nL x64][lightEmission nL x16], 16-byte aligned behind the 4-byte arrays
    const uintptr_t words = (uintptr_t)(np + nOff + sc.nLights);
    DFloat4* lc4 = reinterpret_cast<DFloat4*>(ldsPlaneDet + ((words + 3u) & ~(uintptr_t)3u));
    DFloat4* le4 = lc4 + 4 * sc.nLights;
    for (int i = threadIdx.x; i < 4 * sc.nLights; i += blockDim.x)
        lc4[i] = reinterpret_cast<const DFloat4*>(sc.sphereCold + sc.light[i >> 2])[i & 3];
    for (int i = threadIdx.x; i < sc.nLights; i += blockDim.x) {
        const DMaterial& lm = sc.material[np + sc.light[i]];
        le4[i] = DFloat4{lm.emission[0], lm.emission[1], lm.emission[2], (!COLD_LDS && sc.shadow.enabled) ? sc.shadow.invKeyScale[i] : 0.0f};
    }
    // per (light, plane): which side of the plane the light's ball is on (lightReached skips planes the ray cannot cross)
    // (read by the large-scene kernels only; the space is reserved in every layout so that capi.cpp has one size formula)
    float* lps = reinterpret_cast<float*>(le4 + sc.nLights);
    for (int i = threadIdx.x; !COLD_LDS && i < sc.nLights * np; i += blockDim.x) {
        const int L = i / np, pl = i - L * np;
        const DSphereCold& c = sc.sphereCold[sc.light[L]];
        const DFloat4 r = sc.planeRow[pl];
        const float g = r.x * c.cx + r.y * c.cy + r.z * c.cz + r.w;
        // (g is the plane's LOCAL y of the centre: the world distance times |row|. planesRigid only says det = 1 to rounding -- a plane
        // scaled (2, .5, 1) passes -- so the ball's radius is measured in the same unit: round-4 advisor finding)
        const float rowNorm = __builtin_sqrtf(r.x * r.x + r.y * r.y + r.z * r.z);
        const float tol = 1.001f * c.radius * rowNorm + 1e-3f + 1e-5f * (__builtin_fabsf(r.x * c.cx) + __builtin_fabsf(r.y * c.cy) + __builtin_fabsf(r.z * c.cz) + __builtin_fabsf(r.w));
        lps[i] = (sc.planesRigid && g > tol) ? 1.0f : ((sc.planesRigid && g < -tol) ? -1.0f : 0.0f);
    }
    lds.lightPlaneSide = lps;
    DFloat4* cam4 = le4 + sc.nLights + ((sc.nLights * np + 3) >> 2);
    if (threadIdx.x == 0) {
        cam4[0] = DFloat4{sc.p1[0], sc.p1[1], sc.p1[2], 0.0f};
        cam4[1] = DFloat4{sc.dp2[0], sc.dp2[1], sc.dp2[2], 0.0f};
        cam4[2] = DFloat4{sc.dp3[0], sc.dp3[1], sc.dp3[2], 0.0f};
        cam4[3] = DFloat4{sc.origin[0], sc.origin[1], sc.origin[2], 0.0f};
        cam4[4] = DFloat4{sc.background[0], sc.background[1], sc.background[2], 0.0f};
    }
    lds.camera = cam4; // (cam4[5 .. 7] are the launch's, written by renderBody)
    lds.lightCold = reinterpret_cast<const DSphereCold*>(lc4);
    lds.lightEmission = le4;
    DFloat4* gh = cam4 + 8;
    lds.gridHeader = gh;
    if (!COLD_LDS && sc.grid.enabled && threadIdx.x == 0) {
        const DGrid& g = sc.grid;
        gh[0] = DFloat4{g.bmin[0], g.bmin[1], g.bmin[2], __builtin_bit_cast(float, g.dim[0])};
        gh[1] = DFloat4{g.bmax[0], g.bmax[1], g.bmax[2], __builtin_bit_cast(float, g.dim[1])};
        gh[2] = DFloat4{g.cell[0], g.cell[1], g.cell[2], __builtin_bit_cast(float, g.dim[2])};
        gh[3] = DFloat4{g.invCell[0], g.invCell[1], g.invCell[2], 0.0f};
        gh[4] = DFloat4{g.center[0], g.center[1], g.center[2], g.reach2};
    }
    // the cell lists behind the header, when they fit (the pointers are formed either way; they are followed only if inLds)
    uint32_t* cs = reinterpret_cast<uint32_t*>(gh + 5);
    uint16_t* it = reinterpret_cast<uint16_t*>(cs + sc.grid.nCells + 1);
    lds.gridCellStartLds = cs;
    lds.gridItemsLds = it;
    if (!COLD_LDS && sc.grid.enabled && sc.grid.inLds) {
        for (int i = threadIdx.x; i <= sc.grid.nCells; i += blockDim.x)
            cs[i] = sc.grid.cellStart[i];
        for (int i = threadIdx.x; i < sc.grid.nItems; i += blockDim.x)
            it[i] = sc.grid.items[i];
    }
    __syncthreads();
    return lds;
}

// KAT (known-answer mode): instead of its pixel's camera paths a lane runs ONE path from a given ray
// and RNG state and reports its radiance and the RNG state it ends in (kajo_hip_kat_shade).
//
// SPLIT (small frames): the waves of a workgroup share ONE 8x8-pixel block and divide the launch's passes among
// them, so that a frame with fewer blocks than the chip has wave slots still fills it. Every pass's term radiance / S
// goes to an LDS table [pass][pixel]; after a barrier wave 0 adds the terms to the accumulation in pass order -- the
// float sums are those of one wave doing all the passes.
// LISTS (large scenes whose spheres are all world-space balls): a light sample's shadow query is answered on the spot from the
// light's visibility lists (lightReached) instead of costing the lane a trip of its own through the grid: the light loop of a
// vertex runs to its end in ONE trip, as Shader::sampleLights does (Shader.cpp:50-86), and every trip's walk carries camera and
// extension rays only. Same draws, same tests, same sums in the same order: the buffer does not change by a bit.
// NP, NS >= 0: trace()'s compile-time counts.
template <bool COLD_LDS, bool KAT, bool SPLIT = false, bool LISTS = false, bool ONE_LIGHT = false, int GHOME = 0, bool SIMPLE = false, int NP = -1, int NS = -1>
KDEV void renderBody(const RenderArgs& args, unsigned char* ldsRaw)
{
    const DSceneView& sc = args.scene;
    const int np = NP >= 0 ? NP : sc.nPlanes;

    // ---- stage the scene into LDS (one copy per workgroup) ------------------------------------
#ifdef KAJO_COUNT_SPHERE_TESTS
    LdsScene lds = stageToLds<COLD_LDS, NP, NS>(sc, ldsRaw);
    lds.testCounter = args.counters ? args.counters + 29 : nullptr;
#else
    const LdsScene lds = stageToLds<COLD_LDS, NP, NS>(sc, ldsRaw);
#endif
    // GROUPS (FAST / EXACT, small scenes): the pixel's total takes the passes in groups of KAJO_GROUP_PASSES = 4 by their ABSOLUTE numbers
    // (passes 1-4, 5-8, ...; render_args.h): every group is summed from zero in pass order, the group sums are added to the total in
    // group order -- whatever launch, wave, workgroup or GPU renders a pass. A sum any division of the work can form: one wave rendering
    // all passes of a pixel block (the group sum in `total`, the running total in an LDS word of the lane), several waves dividing the
    // passes (SPLIT: wave 0 adds the terms of the table group by group), or -- PARTS, the launch tail (capi.cpp partTheTail) -- the
    // cheapest blocks of a launch of G whole groups, the ones dispatched last, as G workgroups of one group each, so that the launch ends
    // on short jobs: part 0 adds its group to the total in the tile buffer, part k > 0 leaves its group's sum in side buffer k - 1, and a
    // fold kernel adds the side buffers in part order after the launch. A launch may begin and end inside a group: the group in progress
    // and the total of the complete ones wait in args.carry between launches (the tile buffer holds their sum, the visible value).
    // The frame is a function of the scene, the parameters and the number of passes done -- not of how they were cut into render calls.
    // Not in the STRICT build: the oracle adds the passes' terms one by one (Renderer.cpp:70-71), and a sum of group sums is not that sum.
    constexpr bool GROUPS = !KAT && !KAJO_RSTRICT && COLD_LDS;
    constexpr bool PARTS = GROUPS && !SPLIT;
    constexpr int kGroupMask = KAJO_GROUP_PASSES - 1;
    const uint32_t orderWord = (!KAT && args.blockOrder) ? args.blockOrder[blockIdx.x] : blockIdx.x;
    const uint32_t logicalBlock = PARTS ? (orderWord & 0x0fffffffu) : orderWord;
    const bool parted = PARTS && (orderWord >> 31) != 0u;
    const int part = PARTS ? (int)((orderWord >> 28) & 7u) : 0; // (0 unless parted)
    const int stealWindow = args.stealWindow;
    const int partPasses = parted ? KAJO_GROUP_PASSES : args.nPasses, partFirst = args.firstPass + part * KAJO_GROUP_PASSES;
    if (threadIdx.x == 0) { // what only the camera-ray block needs of the launch: kept out of the scalar registers
        DFloat4* cam = const_cast<DFloat4*>(lds.camera);
        cam[5] = DFloat4{args.pixelWidth, args.pixelHeight, args.sampleWidth, args.sampleHeight};
        cam[6] = DFloat4{__builtin_bit_cast(float, (uint32_t)args.seed ^ 0x79622d32u), __builtin_bit_cast(float, (uint32_t)(args.seed >> 32) ^ 0x6b206574u),
                         __builtin_bit_cast(float, args.W), __builtin_bit_cast(float, args.H)};
        // (PARTS: the bounds of the workgroup's passes depend on the order word, a loaded value -- two more scalars alive through the loop,
        // in kernels that have none to spare. They are needed where a pass is taken over and after the loop only: the camera block's free words.)
        if (PARTS) {
            const int last = partFirst + partPasses;
            cam[0].w = __builtin_bit_cast(float, last);
            cam[1].w = __builtin_bit_cast(float, last - stealWindow > partFirst ? last - stealWindow : partFirst);
        }
        // (GROUPS: where the pixel's sums go when the loop is over -- the tile buffer, or the side buffer of a later part; the carry of a
        // launch that ends inside a group -- likewise: pointers in LDS words, not in scalar registers through the loop)
        if (GROUPS) {
            const uint64_t dst = reinterpret_cast<uint64_t>(part > 0 ? args.side : args.tiles), cry = args.carryOut ? reinterpret_cast<uint64_t>(args.carry) : 0ull;
            cam[7] = DFloat4{__builtin_bit_cast(float, (uint32_t)dst), __builtin_bit_cast(float, (uint32_t)(dst >> 32)), __builtin_bit_cast(float, (uint32_t)cry),
                             __builtin_bit_cast(float, (uint32_t)(cry >> 32))};
            cam[2].w = __builtin_bit_cast(float, args.carrySlots);
            // ... and the slot of the workgroup's first thread: a lane's slot is that plus its index in the workgroup (the SPLIT kernels: in
            // its wave), formed again where the sums are written instead of living -- as a zero-extended 64-bit pair -- through the loop
            cam[3].w = __builtin_bit_cast(float, (PARTS && part > 0) ? kajoSideSlot(blockIdx.x, args.partedFirst, (uint32_t)(args.nPasses / KAJO_GROUP_PASSES),
                                                                                   (uint32_t)part, args.sideStride, blockDim.x, 0u)
                                                                     : logicalBlock * (SPLIT ? 64u : blockDim.x));
        }
    }
    __syncthreads();

    // per-wave mailbox for taken-over passes: [lane][stealWindow] float4, behind the scene copy (render_args.h)
    // (the wave's index in its workgroup is the same in every lane: a scalar, not a vector register alive to the end of the kernel)
    const uint32_t waveInGroup = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    DFloat4* mailbox = reinterpret_cast<DFloat4*>(ldsRaw + args.perWaveOffset + waveInGroup * args.perWaveBytes);

    // ---- which pixel is mine ----------------------------------------------------------------
    const int lane = threadIdx.x & 63;
    const int splitWave = SPLIT ? (int)(threadIdx.x >> 6) : 0;
    const int splitCount = SPLIT ? (int)(blockDim.x >> 6) : 1;
    const uint32_t pixelSlot = SPLIT ? logicalBlock * 64u + (uint32_t)lane : logicalBlock * blockDim.x + threadIdx.x; // index into the tile buffer
    // (part k > 0: its slot of side buffer k - 1 -- the side buffers are compact, one workgroup's worth of slots per parted block in the
    // order the blocks are parted in (render_args.h); nothing more to carry through the loop than the slot itself)
    uint32_t slot = pixelSlot;
    if (PARTS && part > 0) {
        slot = kajoSideSlot(blockIdx.x, args.partedFirst, (uint32_t)(args.nPasses / KAJO_GROUP_PASSES), (uint32_t)part, args.sideStride, blockDim.x, threadIdx.x);
    }
    // SPLIT: per-pass terms of the block, [nPasses][64] float4 behind the scene copy
    DFloat4* termTable = reinterpret_cast<DFloat4*>(ldsRaw + args.mailboxOffset);
    const int wave = (int)(pixelSlot >> 6);
    const int wavesPerTile = (args.tileW >> 3) * (args.tileH >> 3);
    const int ownedTile = wave / wavesPerTile;
    const int wb = wave - ownedTile * wavesPerTile;
    const int tile = args.tileIndex + ownedTile * args.tileCount;
    const int tx = tile % args.tilesX, ty = tile / args.tilesX;
    const int bxi = wb % (args.tileW >> 3), byi = wb / (args.tileW >> 3);
    const int px = tx * args.tileW + bxi * 8 + (lane & 7);
    const int py = ty * args.tileH + byi * 8 + (lane >> 3);
    const bool inImage = KAT ? (int)slot < args.katCount : (ownedTile < args.nTilesOwned && px < args.W && py < args.H);

    const int n = args.n;
    // include/kajo_stream.h: key words (pixel, sample | pass << 16, seed lo ^ pass >> 16, seed hi) ^ constants
    // first pixel of the wave's 8x8 block: the pixel of lane l is (blockX + (l & 7), blockY + (l >> 3))
    const int blockX = __builtin_amdgcn_readfirstlane(px - (lane & 7)), blockY = __builtin_amdgcn_readfirstlane(py - (lane >> 3));

    const F3 origin = ld3(sc.origin); // (initial values only: the loop reads the camera from lds.camera)
    // accumulated radiance of the pixel (Renderer.cpp:70-71), continued across launches
    // (the handle zeroes the buffer when it is created or reset; a slot outside the image is never written and stays zero -- the fold
    // kernel of a parted launch adds to it side-buffer slots that capi.cpp partTheTail cleared and no lane writes)
    F3 total = f3(0.0f, 0.0f, 0.0f);
    float totalW = 0.0f;
    // (LISTS_RMW: the large-scene list kernels of rounds 3-4 -- 128 VGPRs and spilling -- did not carry the pixel's total through the loop:
    // a pass end added its term to the tile buffer in place, 32 bytes of traffic per pixel and PASS instead of per launch)
    constexpr bool LISTS_RMW = LISTS && KAJO_LISTS_TILE_RMW;
    // (PARTS kernels: `total` is the sum of the group of passes the lane is in; the running total waits in the lane's LDS word behind the mailbox)
    DFloat4* const accWord = mailbox + 64 * stealWindow + lane;
    // (the same word, its address formed from the lane index again where a group ends -- once in a hundred paths -- and after the loop: the
    // address as a loop-invariant vector register was what the instance of any number of lights spilled to scratch)
    const auto accWordNow = [&]() -> DFloat4* {
        uint32_t l = (uint32_t)lane; // (not threadIdx.x: the kernel's input register would have to live through the loop for it)
        asm volatile("" : "+v"(l));
        return mailbox + 64 * stealWindow + l;
    };
    if (PARTS) {
        if (inImage) {
            float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (args.carryIn) { // the launch continues a group: the complete groups' total and the group so far (never a parted launch)
                t = reinterpret_cast<const float4*>(args.carry)[slot];
                const float4 g = reinterpret_cast<const float4*>(args.carry)[args.carrySlots + slot];
                total = f3(g.x, g.y, g.z);
            } else if (part == 0) {
                t = reinterpret_cast<const float4*>(args.tiles)[slot];
            }
            *accWord = DFloat4{t.x, t.y, t.z, t.w};
        }
    } else if (!KAT && !LISTS_RMW && inImage) {
        // (SPLIT kernels of the GROUPS builds: wave 0 re-reads what it needs after the loop)
        const float4 t = reinterpret_cast<const float4*>(args.tiles)[slot];
        total = f3(t.x, t.y, t.z);
        totalW = t.w;
    }
    bool katStarted = false;
    // (LISTS kernels -- 128 VGPRs and spilling -- do not carry the pixel's total through the loop: a pass end adds its term to the
    // tile buffer in place, one coalesced 16-byte read and write per 25 paths; the same additions in the same order.)

    // ---- per-lane path state ----------------------------------------------------------------
    int mode = inImage ? MODE_NEW : MODE_DONE;
    // SPLIT, second form (sampleChunks = Q > 1; launches of fewer passes than the block should have waves, e.g. BASELINE
    // configs[0]: one pass): the block has nPasses * Q waves, wave w renders samples [q, q + 1) * n*n / Q (q = w % Q) of pass
    // w / Q, and every PATH's radiance goes to the table, [pass][sample][pixel]; wave 0 then forms the passes' sums in sample
    // order (Renderer.cpp:66) and adds the terms in pass order.
    const int chunks = SPLIT ? args.sampleChunks : 0;
    const bool bySample = SPLIT && chunks > 1;
    const int passesMine = bySample ? 1 : (SPLIT ? args.nPasses / splitCount : partPasses); // the host launches SPLIT / parts only when this divides
    const int firstMine = SPLIT ? args.firstPass + (bySample ? splitWave / chunks : splitWave * passesMine) : partFirst;
    const int sampleBegin = bySample ? (splitWave % chunks) * (n * n / chunks) : 0;
    const int sampleEnd = bySample ? sampleBegin + n * n / chunks : n * n; // (sampleY, sampleX) == (endY, endX): the lane's samples of the pass are done
    const int endY = sampleEnd / n, endX = sampleEnd % n;
    int pass = firstMine;                       // pass being rendered (own or taken over)
    const int lastPassS = firstMine + passesMine; // exclusive
    // Pass stealing. A pass of a pixel is a self-contained piece of work (its n*n paths have their own
    // streams, its sum enters the pixel's total as one term), so a lane that has finished its own pixel
    // takes over the LAST not-yet-started pass of a lane that still has several to go, renders it, and
    // leaves radiance / S in a mailbox in LDS; the owner adds the mailbox terms after its own passes, in
    // pass order -- the float sums are formed exactly as without stealing. Only the last `stealWindow`
    // passes of a launch can be given away (that is all the imbalance there is, and bounds the mailbox).
    int ownPass = firstMine; // next pass of the lane's own pixel
    int myEnd = inImage ? lastPassS : firstMine; // own passes [ownPass, myEnd); shrinks when one is taken over
    int stolenFrom = -1;          // lane whose pass is being rendered, or -1
    const int stealBaseS = lastPassS - stealWindow > firstMine ? lastPassS - stealWindow : firstMine;
#define lastPass (PARTS ? __builtin_bit_cast(int, lds.camera[0].w) : lastPassS)
#define stealBase (PARTS ? __builtin_bit_cast(int, lds.camera[1].w) : stealBaseS)
    int sampleX = sampleBegin % n, sampleY = sampleBegin / n;
    F3 radiance = f3(0.0f, 0.0f, 0.0f); // sum over the pixel's samples of this pass
    Rng rng{0, 0};
    F3 O = origin, d = f3(0.0f, 0.0f, 1.0f);
    F3 L = f3(0.0f, 0.0f, 0.0f), T = f3(1.0f, 1.0f, 1.0f);
    int depth = 0;
    bool collectEmission = true;
    // vertex being shaded
    // (the BSDF's colour, exponent and path-weight scale are constants of the material and the lobe: re-read where they are
    // used instead of carried across the traversal. FAST also sums the vertex's emission and its light samples in one vector.)
    F3 vP = origin, vN = d, vR = d, vE = L;
    int vId = 0, vKind = 0, lightK = 0;
#if KAJO_RSTRICT
    F3 vLd = L;
    float vS = 0.0f; // of the vertex the extension ray left: the MIS correction re-forms the weight with it
#endif
    F3 pendContrib = L; // light sample's contribution if its shadow ray reaches the light
    // extension ray sampled from the BSDF: weight pieces that wait for the light pdf of the hit
    bool pendBsdf = false;
    // (STRICT re-forms the weight from its pieces, in the reference's order; FAST scales the eager throughput by
    // p / (pL + p) -- the same value -- and carries only p: seven registers less across the traversal; so does EXACT)
#if KAJO_RSTRICT
    F3 pendF = L, pendT = L;
    float pendCos = 0.0f;
#endif
    float pendP = 0.0f;

    unsigned long long ctrTraversals = 0, ctrSlots = 0; // (wave-uniform: scalar registers)
    uint32_t ctrVertices = 0, ctrShadow = 0; // per lane and launch (diagnostic counters: one register each, not two, in a loop that is short of them)
    const bool counting = args.counters != nullptr;
    // Small scenes of ONE light --
    // the kernel instance launched for them: the extension ray is sampled in the same visit of the light / BSDF blocks as the light.
    // (STRICT too since its round-4 measurement: with ONE visit per vertex the shadow ray in a trip of its own -- the shared walk at
    // 88 % of the lanes -- beats the walk inside the light loop at 55 %: 19.9 -> 20.5 G paths/s, profiles/r04_presample.txt.)
    constexpr bool PRESAMPLE = ONE_LIGHT && COLD_LDS && !LISTS;
#ifdef KAJO_PROFILE
    // block profile: prof[2k] = wave executions of block k, prof[2k+1] = lanes active in it
    unsigned long long prof[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long stampSum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // [5..8]: inside the light loop of the large-scene kernels
    unsigned long long stampLast = 0;
#define KAJO_STAMP(k)                                                                                                  \
    do {                                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        stampSum[k] += now_ - stampLast;                                                                               \
        stampLast = now_;                                                                                              \
    } while (0)
#define KAJO_PROF(k, cond)                                                                                             \
    do {                                                                                                               \
        const unsigned long long m_ = __ballot(cond);                                                                  \
        if (m_) {                                                                                                      \
            prof[2 * (k)] += 1;                                                                                        \
            prof[2 * (k) + 1] += __builtin_popcountll(m_);                                                             \
        }                                                                                                              \
    } while (0)
#else
#define KAJO_PROF(k, cond)                                                                                             \
    do {                                                                                                               \
    } while (0)
#ifdef KAJO_MARKS
// (tools/isa_blocks.py: the blocks' boundaries as comments in the compiler's assembly output; not a build that runs)
#define KAJO_STAMP(k) asm volatile("; KMARK " #k)
#else
#define KAJO_STAMP(k)                                                                                                  \
    do {                                                                                                               \
    } while (0)
#endif
#endif

#ifdef KAJO_PROFILE
    stampLast = __builtin_amdgcn_s_memtime();
#endif
#if !KAJO_RSTRICT
    const float invS = rrcp(args.S);
#endif
    uint32_t trips = 0;
    int heldTrips = 0; // (wave-uniform) consecutive trips in which some lane wanted the light / BSDF blocks and they did not run
    for (;;) {
        trips++;
        KAJO_STAMP(4); // tail of the previous trip (path bookkeeping, loop back-edge)
        // ---- MODE_NEW: camera ray of the next sample (Renderer.cpp:51-64) ---------------------
        KAJO_PROF(0, mode == MODE_NEW);
        if (KAT && mode == MODE_NEW) {
            if (katStarted) {
                mode = MODE_DONE;
            } else {
                katStarted = true;
                O = ld3(args.katRays + 6 * slot);
                d = ld3(args.katRays + 6 * slot + 3);
                rng.lo = args.katStates[2 * slot];
                rng.hi = args.katStates[2 * slot + 1];
                L = f3(0.0f, 0.0f, 0.0f);
                T = f3(1.0f, 1.0f, 1.0f);
                depth = 0;
                collectEmission = true;
                pendBsdf = false;
                mode = MODE_EXTEND;
            }
        }
        constexpr bool ANY_GIVES = KAJO_ANY_LANE_GIVES && !SPLIT; // (the SPLIT kernels' waves are short: the wider ballot only costs them registers)
        // Out of own passes: take one over, or retire when nobody has one to give. ANY lane of the wave that still has a pass it has not
        // begun can give it -- also one in the middle of a path (round 6, STRICT / EXACT builds; until then, and in the FAST build and the
        // SPLIT kernels still, only lanes that are between two paths in the same trip are asked, and a lane retires for want of a giver
        // while others still have passes to spare).
        const auto takeOverPasses = [&]() {
            unsigned long long idleMask = __ballot(mode == MODE_NEW && stolenFrom < 0 && ownPass >= myEnd);
            while (idleMask) { // wave-uniform; only in the last stretch of the wave's life
                const int give = myEnd - 1; // the pass this lane could give away
                const unsigned long long giverMask = __ballot((ANY_GIVES || mode == MODE_NEW) && mode != MODE_DONE && stolenFrom < 0 &&
                                                              give > ownPass && give >= stealBase);
                if (giverMask == 0ull) {
                    if (mode == MODE_NEW && stolenFrom < 0 && ownPass >= myEnd)
                        mode = MODE_DONE;
                    break;
                }
                // lowest idle lane takes the last pass of the lowest giver
                const int thief = __builtin_ctzll(idleMask), giver = __builtin_ctzll(giverMask);
                const int takenPass = __builtin_amdgcn_readlane(myEnd, giver) - 1;
                if (lane == giver)
                    myEnd = takenPass;
                if (lane == thief) {
                    stolenFrom = giver;
                    pass = takenPass;
                }
                idleMask &= idleMask - 1; // next idle lane
            }
        };
        if (!KAT && mode == MODE_NEW) {
            if (sampleY == endY && sampleX == endX) { // pass complete: Renderer.cpp:70-71
#if KAJO_RSTRICT
                const F3 term = f3(kdiv(radiance.x, args.S), kdiv(radiance.y, args.S), kdiv(radiance.z, args.S));
#else
                const F3 term = radiance * invS;
#endif
                if (bySample) { // (the paths' radiances are in the table already; this wave has no other pass)
                    ownPass++;
                } else if (SPLIT) { // own or taken over: the term goes to the table, under its pass and pixel
                    termTable[(pass - args.firstPass) * 64 + (stolenFrom >= 0 ? stolenFrom : lane)] = DFloat4{term.x, term.y, term.z, 0.0f};
                    if (stolenFrom >= 0)
                        stolenFrom = -1;
                    else
                        ownPass++;
                } else if (stolenFrom >= 0) {
                    mailbox[stolenFrom * stealWindow + (pass - stealBase)] = DFloat4{term.x, term.y, term.z, 0.0f};
                    stolenFrom = -1;
                } else {
                    if (LISTS_RMW) {
                        float4* acc = reinterpret_cast<float4*>(args.tiles) + slot;
                        const float4 t4 = *acc;
                        *acc = make_float4(t4.x + term.x, t4.y + term.y, t4.z + term.z, t4.w);
                    } else {
                        total = total + term;
                    }
                    ownPass++;
                    if (PARTS) { // a group of passes complete
                        // (also when it was the last group: what is added after the loop is a zero then)
                        if (((ownPass - 1) & kGroupMask) == 0) { // (a group ends before pass p when (p - 1) % 4 == 0: passes are numbered from 1)
                            DFloat4* const aw = accWordNow();
                            const DFloat4 a = *aw;
                            *aw = DFloat4{a.x + total.x, a.y + total.y, a.z + total.z, a.w};
                            total = f3(0.0f, 0.0f, 0.0f);
                        }
                    }
                }
                radiance = f3(0.0f, 0.0f, 0.0f);
                sampleX = sampleBegin % n;
                sampleY = sampleBegin / n;
                pass = ownPass;
            }
            if (!ANY_GIVES)
                takeOverPasses();
        }
        if (!KAT && ANY_GIVES)
            takeOverPasses();
        {
            const bool starts = !KAT && mode == MODE_NEW && (stolenFrom >= 0 || ownPass < myEnd);
            if (starts) {
                // The pixel whose pass the lane is rendering: its own, or the one of the lane it took the pass over from (same
                // 8x8 block). Its stream key word and x * pixelWidth, (H - y) * pixelHeight of Renderer.cpp:56-57 are formed here
                // rather than carried in six registers through the whole loop.
                const int srcLane = stolenFrom >= 0 ? stolenFrom : lane;
                const int spx = blockX + (srcLane & 7), spy = blockY + (srcLane >> 3);
                const DFloat4 c5 = lds.camera[5], c6 = lds.camera[6];
                const int imgW = __builtin_bit_cast(int, c6.z), imgH = __builtin_bit_cast(int, c6.w);
                const float curPixX = spx * c5.x, curPixY = (imgH - spy) * c5.y;
                uint32_t a = (uint32_t)(spy * imgW + spx) ^ 0x61707865u, c = __builtin_bit_cast(uint32_t, c6.x) ^ ((uint32_t)pass >> 16), dd = __builtin_bit_cast(uint32_t, c6.y);
                uint32_t b = ((uint32_t)(sampleY * n + sampleX) | ((uint32_t)pass << 16)) ^ 0x3320646eu;
                KAJO_QUARTER_ROUND(a, b, c, dd);
                KAJO_QUARTER_ROUND(a, b, c, dd);
                KAJO_QUARTER_ROUND(a, b, c, dd);
                Rng fresh;
                fresh.lo = (uint64_t)a | ((uint64_t)b << 32);
                fresh.hi = (uint64_t)c | ((uint64_t)dd << 32);
                rngStep(fresh);
                float offX = unitBits((uint32_t)fresh.lo);
                float offY = unitBits((uint32_t)(fresh.lo >> 32));
                float sx = curPixX + sampleX * c5.z + offX * c5.z;
                float sy = curPixY + sampleY * c5.w + offY * c5.w;
                const DFloat4 c0 = lds.camera[0], c1 = lds.camera[1], c2 = lds.camera[2], c3 = lds.camera[3];
                const F3 camOrigin = f3(c3.x, c3.y, c3.z);
                F3 dir = f3(c0.x, c0.y, c0.z) + f3(c1.x, c1.y, c1.z) * sx + f3(c2.x, c2.y, c2.z) * sy - camOrigin;
                const F3 nd = normalize(dir);
                sampleX++;
                if (sampleX == n) {
                    sampleX = 0;
                    sampleY++;
                }
                rng = fresh;
                d = nd;
                O = camOrigin;
                L = f3(0.0f, 0.0f, 0.0f);
                T = f3(1.0f, 1.0f, 1.0f);
                depth = 0;
                collectEmission = true;
                pendBsdf = false;
                mode = MODE_EXTEND;
            }
        }
        int aliveCount;
        {
            const unsigned long long aliveMask = __ballot(mode != MODE_DONE);
            if (aliveMask == 0ull)
                break;
            aliveCount = __builtin_popcountll(aliveMask);
        }
        const unsigned long long activeMask = __ballot(mode == MODE_EXTEND || mode == MODE_SHADOW); // lanes with a ray

        KAJO_STAMP(0); // camera-ray block
        // ---- one ray per lane through the whole scene ------------------------------------------
        const Hit hit = trace<!COLD_LDS, GHOME, LISTS, SIMPLE, NP, NS>(sc, lds, O, d, mode == MODE_EXTEND || mode == MODE_SHADOW);
        KAJO_STAMP(1); // traversal
        if (counting) {
            ctrTraversals += __builtin_popcountll(activeMask);
            ctrSlots += 64;
        }

        bool sampleNext = mode == MODE_HOLD; // continue with the light loop / BSDF sampling of vertex v*
        bool pathDone = false;
        KAJO_PROF(1, mode == MODE_EXTEND && pendBsdf && hit.id > np);
        KAJO_PROF(2, mode == MODE_EXTEND && hit.id != 0);
        KAJO_PROF(6, mode == MODE_SHADOW);

        if (mode == MODE_EXTEND) {
            // the hit object's material: coins and emission in one round trip (device_scene.h)
            const DFloat4* mq = reinterpret_cast<const DFloat4*>(lds.material + (hit.id > 0 ? hit.id - 1 : 0));
            const DFloat4 m0 = mq[0], m1 = mq[1];
            const uint32_t m1flags = __builtin_bit_cast(uint32_t, m1.w);
            // Weight of the BSDF-sampled segment that just ended (Shader.cpp:203-212). The throughput was
            // advanced with a zero light pdf when the direction was sampled (0 + p == p exactly); only a ray
            // that lands on a light other than the vertex it left needs the MIS denominator pL + p.
            if (pendBsdf) {
                // (A light that is a pure emitter -- no diffuse, specular or transparent colour, pRR == 0 -- ends every path
                // that reaches it, and a path that arrives over a BSDF-sampled segment collects no emission there
                // (Shader.cpp:121,212): its throughput is never used again, so the MIS correction is skipped. STRICT
                // keeps it when the throughput is not finite: NaN * 0 must stay NaN.)
#if KAJO_STRICT
                // (EXACT keeps the test: its throughput is the oracle's to the last places, so it is finite where the oracle's is)
                const bool weightMatters = m0.x != 0.0f || !(__builtin_fabsf(T.x) < __builtin_inff() && __builtin_fabsf(T.y) < __builtin_inff() && __builtin_fabsf(T.z) < __builtin_inff());
#else
                const bool weightMatters = m0.x != 0.0f;
#endif
                if (hit.id > np && hit.id != vId && (m1flags & KAJO_MAT_IS_LIGHT) && weightMatters) {
                    const DSphereCold& lc = lds.sphereCold[hit.id - 1 - np];
#if KAJO_RSTRICT
                    const float pL = krcp(solidAngle(f3(lc.cx, lc.cy, lc.cz), lc.radius, vP));
                    const F3 wb = (krcp(pL + pendP) * pendF) * pendCos;
                    T = pendT * (vS * wb);
#else
                    const float pL = lightPdf(lc, vP);
                    T = T * (pendP * rrcp(pL + pendP));
#endif
                }
                collectEmission = false; // SampleNonEmissiveObjects
                pendBsdf = false;
            }
            if (hit.id == 0) { // Shader.cpp:116-117
                const DFloat4 bg = lds.camera[4];
                L = rmadd(T, f3(bg.x, bg.y, bg.z), L);
                pathDone = true;
            } else {
                ctrVertices += 1; // (unconditionally: an inline constant, where `counting` as an addend would be one more live register)
                const F3 view = d;
                vP = O + d * hit.t; // Raytracer.cpp:134-135
                vN = hitNormal<LISTS || SIMPLE, NP>(sc, lds, hit, O, d);
                vId = hit.id;
                vE = collectEmission ? f3(m1.x, m1.y, m1.z) : f3(0.0f, 0.0f, 0.0f); // Shader.cpp:121
                float pc;
                const bool cont = flipCoin(rng, m0.x, pc); // Shader.cpp:124-125
                if (!cont || depth >= args.depthLimit) {
                    // Shader.cpp:126-127: 1 / pc with pc = pRR (depth limit) or 1 - pRR (the coin said stop). The quotient depends on
                    // the material only and is formed on the host in the reference's order (stage.cpp), in both numerics modes.
                    float sEnd = m0.w;
                    if (cont)
                        sEnd = mq[4].w;
                    L = rmadd(T, sEnd * vE, L);
                    pathDone = true;
                } else {
                    float pt;
                    const bool transparent = flipCoin(rng, m0.y, pt); // Shader.cpp:130-134
                    KAJO_PROF(3, transparent);
                    KAJO_PROF(4, !transparent);
                    if (transparent) { // Shader.cpp:137-151; the BSDF colour is the SPECULAR colour
                        const DFloat4 m2 = mq[2], m4 = mq[4];
                        F3 nd = transmissionDirection(view, vN, m2.w);
                        float cosA = __builtin_fabsf(dot(nd, vN)); // (divided by: its exact zeros are the oracle's NaN pixels)
                        F3 spec = f3(m2.x, m2.y, m2.z);
#if KAJO_RSTRICT
                        F3 f = f3(kdiv(spec.x, cosA), kdiv(spec.y, cosA), kdiv(spec.z, cosA)); // BSDF.cpp:126-130
#else
                        F3 f = spec * rrcp(cosA);
#endif
                        F3 w = (m4.z * f) * __builtin_fabsf(dot(vN, nd)); // sTransparent = 1/pc * 1/pt, Shader.cpp:146-147
                        L = rmadd(T, w * vE, L);
                        T = T * w;
                        O = vP + nd * kEps;
                        d = nd;
                        depth++;
                        // mode stays MODE_EXTEND, the light sampling scheme is inherited
                    } else {
                        float pd;
                        const bool diffuse = flipCoin(rng, m0.z, pd); // Shader.cpp:153-154
                        vKind = diffuse ? 0 : ((m1flags & KAJO_MAT_HAS_EXPONENT) ? 1 : 2);
                        vR = reflect(view, vN);
#if KAJO_RSTRICT
                        vLd = f3(0.0f, 0.0f, 0.0f);
#endif
                        lightK = 0;
                        sampleNext = true;
                    }
                }
            }
        } else if (!LISTS && mode == MODE_SHADOW) {
            // Shader.cpp:72-73: the sample counts iff the closest hit of the shadow ray IS the light
            constexpr bool pre = PRESAMPLE; // the extension ray was sampled together with the light (every shadow ray of the one-light instance)
            const int lk = pre ? 0 : lightK;
            if (hit.id == np + 1 + lds.light[lk]) {
#if KAJO_RSTRICT
                vLd = vLd + pendContrib;
#else
                vE = vE + pendContrib;
#endif
            }
            if (pre) {
#if KAJO_RSTRICT
                // ... and waits in the register of the vertex's normal; the weight is formed here from its pieces, which wait for
                // the next hit's MIS correction anyway (the expressions of the BSDF sampling block, in its order)
                L = L + T * (vS * (vE + vLd));
                T = T * (vS * ((krcp(0.0f + pendP) * pendF) * pendCos));
                O = vP + vN * kEps;
                d = vN;
                if (pendP == 0.0f)
                    pathDone = true;
                else
                    mode = MODE_EXTEND;
#else
                // ... and waits in the vertex's dead registers: direction in vN, path-weight factor in vR (see the BSDF sampling block)
                const DFloat4 v4 = reinterpret_cast<const DFloat4*>(lds.material + (vId - 1))[4];
                L = rmadd(T, (vKind == 0 ? v4.x : v4.y) * vE, L);
                T = T * vR;
                O = vP + vN * kEps;
                d = vN;
                if (pendP == 0.0f)
                    pathDone = true;
                else
                    mode = MODE_EXTEND;
#endif
            } else {
                lightK++;
                sampleNext = true;
            }
        }

        KAJO_STAMP(2); // vertex / shadow-result block
        // The light / BSDF sampling blocks are a third of a trip's instructions (STRICT: 40 %, binary32 sin/cos/asin series, IEEE
        // divisions) and run with a quarter of the lanes. They run in this trip if at least thrL lanes want them, or if some
        // lane has waited a trip already (no vertex waits twice); lanes that want them in a trip without them keep their
        // vertex in their registers and sit the next traversal out. thrL = 1: every trip (round 2's schedule; large scenes).
        // Measured (profiles/r03_hold_sweep.txt): STRICT +7.5 % at 24-32 lanes; FAST nothing while its loop spilled scalar
        // registers (the two ballots cost what the blocks saved), +2.4 % at 20 lanes since it does not.
        const unsigned long long wantL = __ballot(sampleNext);
        // (holdTrips: how many trips in a row the blocks may be put off while somebody wants them; 1 = no vertex waits twice)
        const int wantCount = __builtin_popcountll(wantL);
        // (The FAST loop of small scenes never waits more than one trip, and has no scalar register to spare for the counter: with
        // it the loop spills five. It asks whether any lane is holding, which is the same thing for holdTrips = 1.)
        bool runL;
        if (KAJO_STRICT || !COLD_LDS) {
            // (near the end of a wave's life few lanes are left: three quarters of them are as good as it gets)
            const int thr = min(args.thrL, aliveCount - (aliveCount >> 2));
            runL = wantCount >= thr || heldTrips >= args.holdTrips;
            heldTrips = (runL || wantCount == 0) ? 0 : heldTrips + 1;
        } else {
            // (A second hold state per lane instead of the counter -- two trips of waiting without a scalar register -- measured
            // +0.5 % at best on the one-light instance, within the noise of the runs: profiles/r04_presample.txt.)
            runL = wantCount >= args.thrL || __ballot(mode == MODE_HOLD) != 0ull;
        }
        if (sampleNext && !runL)
            mode = MODE_HOLD;
        sampleNext = sampleNext && runL;
        KAJO_PROF(5, sampleNext);
        // the BSDF's colour, exponent and path-weight scale of the vertices whose light / BSDF blocks run in this trip
        F3 vColor = f3(0.0f, 0.0f, 0.0f);
        float vExp = 0.0f, vSl = 0.0f;
        if (sampleNext) {
            const DFloat4* vq = reinterpret_cast<const DFloat4*>(lds.material + (vId - 1));
            const DFloat4 v2 = vq[2], v3 = vq[3], v4 = vq[4];
            vColor = vKind == 0 ? f3(v3.x, v3.y, v3.z) : f3(v2.x, v2.y, v2.z);
            vExp = v3.w;
            vSl = vKind == 0 ? v4.x : v4.y; // 1/pc * 1/pt * 1/pd, Shader.cpp:160-177
        }
        if (LISTS && runL) {
            // ---- sampleLights with the shadow query on the spot (Shader.cpp:50-86 as the reference runs it: a vertex's whole loop in
            // one visit), in ROUNDS the whole wave takes part in: in every round a lane with lights left forms the sample of its next
            // countable light and does the part of the query that is its own (the light itself, the planes: lightReachedHead); then
            // the lists of the round's queries are walked by ALL lanes whose ray registers are dead -- a query's owner takes every
            // (G+1)-th item of its list and G helpers the others, reading the ray from the owner's registers (ds_bpermute) -- because
            // a wave makes as many item rounds as its longest list has items, and without help a third of the lanes would walk
            // lists of 5 items on average and 13 at the longest while the rest watch. Which lane tests an item does not change the
            // test; the owner adds its contribution iff nobody found a blocker: the sums form as before, in light order.
            // (The LDS address space spelled out: the compiler does not infer it for VOLATILE accesses, and through a generic pointer they
            // compile to flat_load / flat_store with system scope and a vmcnt(0) wait each -- in every round of this loop, until round 4
            // looked: +1.4 % FAST, +0.9 % STRICT on the 1000-sphere scene.)
            KajoLdsWord* helpOwner = (KajoLdsWord*)(reinterpret_cast<unsigned char*>(mailbox) + 64 * stealWindow * 16);
            KajoLdsWord* helpFlag = helpOwner + 64;
            const uint32_t* items = sc.shadow.items;
            const int nL = sc.nLights;
            const bool canHelp = sampleNext || pathDone || mode == MODE_DONE; // (their O / d are rewritten before they are read again)
#if KAJO_LISTS_BALANCED
            // BALANCED (round 5): the unit of work of this loop is a (vertex, light) PAIR, not a vertex. Lights are taken two at a time, the
            // same two for the whole wave: (A) every lane with a vertex draws the two lights' random numbers -- the one thing that is
            // sequential per path (Light.cpp:39-41: one draw per light that is not the vertex itself) -- and decides which of them can
            // count; (B) the wave's countable pairs (~50 of 128) are numbered and dealt to ALL lanes whose ray registers are dead, one
            // pair each: the lane fetches the pair's vertex from its owner's registers (ds_bpermute), forms the sample, evaluates the BSDF
            // toward it, runs the query's own part and takes part in the cooperative list walk as before; (C) the vertex's owner pulls
            // contribution and answer back and adds them in light order. A vertex on the floor counts 15 of 16 lights, one under a sphere
            // 3: with one vertex per lane the wave made as many rounds as its busiest lane has lights with 45 % of its lanes working;
            // dealt as pairs the same work takes 8 rounds at ~80 %. Which lane forms a sample does not change it: same draws, same
            // arithmetic, sums in light order -- STRICT stays the oracle bit for bit.
            KajoLdsWord* pairTable = helpOwner; // [128] pair -> owner lane | (light of the chunk) << 6; rewritten every round (the list walk reuses the words)
            const unsigned long long execMask = __ballot(canHelp);
            const int H = __builtin_popcountll(execMask);
            const int myRank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(execMask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)execMask, 0u));
            for (int c0 = 0; c0 < nL; c0 += 2) {
                // ---- (A) draws and countability of lights c0, c0 + 1 for every vertex of the wave
                float sa0 = 0.0f, sa1 = 0.0f, sa2 = 0.0f, sb0 = 0.0f, sb1 = 0.0f, sb2 = 0.0f;
                bool hasA = false, hasB = false;
                for (int j = 0; j < 2; j++) {
                    const int k = c0 + j;
                    if (k >= nL)
                        break;
                    const int sk = lds.light[k];
                    const DSphereCold& lk = lds.lightCold[k];
                    if (sampleNext && np + 1 + sk != vId) { // a light does not sample itself (and draws nothing)
                        const F3 toC = f3(lk.cx - vP.x, lk.cy - vP.y, lk.cz - vP.z);
                        const bool below = dot(vN, toC) < -(1.001f * lk.radius + 1e-6f * (__builtin_fabsf(toC.x) + __builtin_fabsf(toC.y) + __builtin_fabsf(toC.z)));
                        rngStep(rng);
                        const float u1 = unitBits((uint32_t)rng.lo), u2 = unitBits((uint32_t)(rng.lo >> 32)), u3 = unitBits((uint32_t)rng.hi);
                        // (a light that cannot count only draws: see the one-vertex-per-lane loop below for the two rules)
                        bool countable = !(vKind == 2 || below);
#if KAJO_STRICT
                        countable = countable || (vKind == 0 && u1 > 0.999999f);
#endif
                        if (j == 0) {
                            hasA = countable;
                            sa0 = u1, sa1 = u2, sa2 = u3;
                        } else {
                            hasB = countable;
                            sb0 = u1, sb1 = u2, sb2 = u3;
                        }
                    }
                }
                KAJO_STAMP(5);
                const unsigned long long mA = __ballot(hasA), mB = __ballot(hasB);
                const int nA = __builtin_popcountll(mA), P = nA + __builtin_popcountll(mB);
                if (P == 0)
                    continue;
                const int pA = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mA >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mA, 0u));
                const int pB = nA + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mB >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mB, 0u));
                for (int base = 0; base < P; base += H) {
                    // ---- (B) pairs base .. base + H - 1, one per lane that can work
                    if (hasA)
                        pairTable[pA] = (uint32_t)lane;
                    if (hasB)
                        pairTable[pB] = (uint32_t)lane | 64u;
                    __builtin_amdgcn_wave_barrier();
                    const int pMine = base + myRank;
                    const bool worker = canHelp && pMine < P;
                    uint32_t ow = (uint32_t)lane;
                    if (worker)
                        ow = pairTable[pMine];
                    __builtin_amdgcn_wave_barrier();
                    const bool second = (ow & 64u) != 0u;
                    const int addrV = (int)(ow & 63u) << 2;
#define KAJO_PULL_F(x) __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addrV, __builtin_bit_cast(int, x)))
                    const F3 qP = f3(KAJO_PULL_F(vP.x), KAJO_PULL_F(vP.y), KAJO_PULL_F(vP.z));
                    const F3 qN = f3(KAJO_PULL_F(vN.x), KAJO_PULL_F(vN.y), KAJO_PULL_F(vN.z));
                    const F3 qR = f3(KAJO_PULL_F(vR.x), KAJO_PULL_F(vR.y), KAJO_PULL_F(vR.z));
                    const F3 qColor = f3(KAJO_PULL_F(vColor.x), KAJO_PULL_F(vColor.y), KAJO_PULL_F(vColor.z));
                    const float qExp = KAJO_PULL_F(vExp);
                    const int qKind = __builtin_amdgcn_ds_bpermute(addrV, vKind);
                    const float ta0 = KAJO_PULL_F(sa0), ta1 = KAJO_PULL_F(sa1), ta2 = KAJO_PULL_F(sa2);
                    const float tb0 = KAJO_PULL_F(sb0), tb1 = KAJO_PULL_F(sb1), tb2 = KAJO_PULL_F(sb2);
#undef KAJO_PULL_F
                    const float s1 = second ? tb0 : ta0, s2 = second ? tb1 : ta1, s3 = second ? tb2 : ta2;
                    bool hasQ = false;
                    uint32_t keyL = 0, k0 = 0, e = 0, reachQ = 0;
                    int si = 0;
                    if (worker) {
                        const int k = c0 + (second ? 1 : 0);
                        si = lds.light[k];
                        const DSphereCold& lc = lds.lightCold[k];
                        float pl;
                        d = lightDirection(f3(lc.cx, lc.cy, lc.cz), lc.radius, qP, s1, s2, s3, pl);
#if !KAJO_RSTRICT
                        pl = lightPdf(lc, qP);
#endif
                        float pb;
                        const F3 fl = bsdfEvaluateWithPdf(qKind, qColor, qExp, qR, qN, d, pb);
                        const float cosL = kmax0(dot(qN, d));
                        O = qP + d * kEps;
                        if (!(pl == 0.0f || pb == 0.0f || (cosL == 0.0f && KAJO_IS_A_NUMBER(pb)))) {
                            const DFloat4 le = lds.lightEmission[k];
                            pendContrib = ((rrcp(pb + pl) * fl) * cosL) * f3(le.x, le.y, le.z);
                            ctrShadow += 1;
                            KAJO_COUNT_TESTS(lds, 2);
                            hasQ = lightReachedHead(sc, lds, k, si, O, d, keyL);
                            if (hasQ) {
                                uint32_t ia;
                                const uint32_t row = shadowBin(sc, lc, k, le.w, O, ia, reachQ);
                                const uint16_t* off = sc.shadow.off16 + row * (uint32_t)(sc.shadow.n + 1) + ia;
                                const uint32_t rb = sc.shadow.rowBase[row];
                                k0 = rb + off[0];
                                e = rb + off[1];
                            }
                        }
                    }
                    KAJO_STAMP(6);
                    const bool blocked = listWalk(sc, lds, helpOwner, helpFlag, items, lane, hasQ, canHelp, O, d, keyL, k0, e, si, reachQ);
                    KAJO_STAMP(7);
                    // ---- (C) answers back to the vertices' owners, in light order
                    const bool reached = hasQ && !blocked;
                    if (worker)
                        helpOwner[pMine - base] = (uint32_t)lane; // (the list walk is done with the words)
                    __builtin_amdgcn_wave_barrier();
                    for (int j = 0; j < 2; j++) {
                        const int pj = j == 0 ? pA : pB;
                        const bool mine = (j == 0 ? hasA : hasB) && pj >= base && pj < base + H;
                        int src = lane;
                        if (mine)
                            src = (int)helpOwner[pj - base];
                        const int addrW = src << 2;
                        const int got = __builtin_amdgcn_ds_bpermute(addrW, reached ? 1 : 0);
                        const F3 cj = f3(__builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addrW, __builtin_bit_cast(int, pendContrib.x))),
                                         __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addrW, __builtin_bit_cast(int, pendContrib.y))),
                                         __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addrW, __builtin_bit_cast(int, pendContrib.z))));
                        if (mine && got != 0) { // Shader.cpp:72-80: the closest hit is the light
#if KAJO_RSTRICT
                            vLd = vLd + cj;
#else
                            vE = vE + cj;
#endif
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    KAJO_STAMP(8);
                }
            }
#else
            int k = sampleNext ? lightK : nL;
            for (;;) {
                bool hasQ = false;
                uint32_t keyL = 0, k0 = 0, e = 0;
                int si = 0;
                uint32_t reachQ = 0;
                if (k < nL) {
                    // Lights whose sample is discarded whatever it is only draw their random number (see the loop further down)
                    for (; k < nL; k++) {
                        if (np + 1 + lds.light[k] == vId) // a light does not sample itself (and draws nothing)
                            continue;
                        const DSphereCold& lk = lds.lightCold[k];
                        const F3 toC = f3(lk.cx - vP.x, lk.cy - vP.y, lk.cz - vP.z);
                        const bool below = dot(vN, toC) < -(1.001f * lk.radius + 1e-6f * (__builtin_fabsf(toC.x) + __builtin_fabsf(toC.y) + __builtin_fabsf(toC.z)));
                        if (!(vKind == 2 || below))
                            break;
#if KAJO_STRICT
                        // (A light below the horizon adds nothing -- unless its sample is NOT A NUMBER, which the reference adds as NaN
                        // when its poisoned shadow walk ends on that light (see the skip on the cosine further down). That needs
                        // r^2 - x^2 - y^2 < 0, i.e. the sample's first uniform within rounding of 1: such a draw -- one in a million --
                        // goes through the sampling code, where the case is decided; only the diffuse lobe's pdf is NaN for a NaN direction.)
                        Rng peek = rng;
                        rngStep(peek);
                        if (vKind == 0 && unitBits((uint32_t)peek.lo) > 0.999999f)
                            break;
                        rng = peek;
#else
                        rngStep(rng);
#endif
                    }
                    if (k < nL) {
                        si = lds.light[k];
                        const DSphereCold& lc = lds.lightCold[k];
                        float pl;
                        d = lightGenerate(f3(lc.cx, lc.cy, lc.cz), lc.radius, vP, rng, pl);
#if !KAJO_RSTRICT
                        pl = lightPdf(lc, vP);
#endif
                        float pb;
                        const F3 fl = bsdfEvaluateWithPdf(vKind, vColor, vExp, vR, vN, d, pb);
                        const float cosL = kmax0(dot(vN, d));
                        O = vP + d * kEps;
                        if (!(pl == 0.0f || pb == 0.0f || (cosL == 0.0f && KAJO_IS_A_NUMBER(pb)))) { // (such a sample adds nothing whatever its shadow ray finds; see the loop further down)
                            const DFloat4 le = lds.lightEmission[k];
                            pendContrib = ((rrcp(pb + pl) * fl) * cosL) * f3(le.x, le.y, le.z);
                            ctrShadow += 1;
                            KAJO_COUNT_TESTS(lds, 2);
                            hasQ = lightReachedHead(sc, lds, k, si, O, d, keyL);
                            if (hasQ) {
                                uint32_t ia;
                                const uint32_t row = shadowBin(sc, lc, k, le.w, O, ia, reachQ);
                                const uint16_t* off = sc.shadow.off16 + row * (uint32_t)(sc.shadow.n + 1) + ia;
                                const uint32_t base = sc.shadow.rowBase[row];
                                k0 = base + off[0];
                                e = base + off[1];
                            }
                        }
                        k++;
                    }
                }
                KAJO_STAMP(5); // (light loop of the large-scene kernels: samples + the queries' own part)
                const unsigned long long qMask = __ballot(hasQ);
                if (qMask != 0ull) {
                    // (Giving the helpers to the long lists only -- bins of at least 2 / 4 / 6 / 9 items -- measured the same or worse:
                    // a bin's length says little about how far along it the ray's reach goes.)
                    const unsigned long long idleMask = __ballot(!hasQ && canHelp);
                    const int nQ = __builtin_popcountll(qMask);
                    int G = __builtin_popcountll(idleMask) / nQ; // helpers per query
                    G = G > 7 ? 7 : G;
                    const unsigned long long mine = hasQ ? qMask : idleMask;
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
                    if (hasQ) {
                        helpOwner[rank] = (uint32_t)lane;
                        helpFlag[lane] = 0u;
                    }
                    __builtin_amdgcn_wave_barrier();
                    const bool helper = !hasQ && canHelp && rank < nQ * G;
                    int ownerLane = lane, sub = 0;
                    if (helper) {
                        const int qr = (int)(((float)rank + 0.5f) * __builtin_amdgcn_rcpf((float)G)); // rank / G (small integers)
                        sub = 1 + rank - qr * G;
                        ownerLane = (int)helpOwner[qr];
                    }
                    // The query's ray and keys from its owner's registers, IN PLACE: an owner reads its own lane, and so does every lane
                    // that is neither owner nor helper -- their registers keep their values; a helper's are dead (canHelp). No second
                    // set of eleven registers in a kernel that has none to spare.
                    const int addr = ownerLane << 2;
#define KAJO_FROM_OWNER_F(x) x = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, x)))
#define KAJO_FROM_OWNER_U(x) x = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(x))
                    KAJO_FROM_OWNER_F(O.x);
                    KAJO_FROM_OWNER_F(O.y);
                    KAJO_FROM_OWNER_F(O.z);
                    KAJO_FROM_OWNER_F(d.x);
                    KAJO_FROM_OWNER_F(d.y);
                    KAJO_FROM_OWNER_F(d.z);
                    KAJO_FROM_OWNER_U(keyL);
                    KAJO_FROM_OWNER_U(k0);
                    KAJO_FROM_OWNER_U(e);
                    si = (int)__builtin_amdgcn_ds_bpermute(addr, si);
                    KAJO_FROM_OWNER_U(reachQ);
#undef KAJO_FROM_OWNER_F
#undef KAJO_FROM_OWNER_U
                    bool blocked = false;
                    KAJO_STAMP(6); // (helpers found, rays fetched)
                    if (hasQ || helper) {
                        const float aT = dot(d, d);
#if KAJO_STRICT
                        const float iaT = 0.0f;
#else
                        const float iaT = krcp(aT);
#endif
                        // (quantised key << 16 | sphere index), 4 bytes each, the next one requested before the current one is tested; sorted by key
                        const uint32_t stride = (uint32_t)G + 1u;
                        uint32_t j = k0 + (uint32_t)sub;
                        uint32_t nxt = 0xffffffffu;
                        if (j < e)
                            nxt = items[j];
                        while (j < e) {
                            const uint32_t cur = nxt;
                            j += stride;
                            if (j < e)
                                nxt = items[j];
                            if ((cur >> 16) > reachQ) // nothing further along the list can touch the ray before it ends
                                break;
                            KAJO_COUNT_TESTS(lds, 1);
                            if (shadowItemBlocks(sc, lds, (int)(cur & 0xffffu), si, O, d, aT, iaT, keyL)) {
                                blocked = true;
                                break;
                            }
                        }
                        if (helper && blocked)
                            helpFlag[ownerLane] = 1u;
                    }
                    __builtin_amdgcn_wave_barrier();
                    KAJO_STAMP(7); // (lists walked)
                    if (hasQ && !blocked && helpFlag[lane] == 0u) { // Shader.cpp:72-80: the closest hit is the light
#if KAJO_RSTRICT
                        vLd = vLd + pendContrib;
#else
                        // (the product above stays a rounded value of its own, as in the kernels where it waits a trip for its
                        // shadow ray: contracted into this sum it would round once -- FAST with and without lists must agree bit for bit)
                        asm volatile("" : "+v"(pendContrib.x), "+v"(pendContrib.y), "+v"(pendContrib.z));
                        vE = vE + pendContrib;
#endif
                    }
                }
                KAJO_STAMP(8); // (contributions added)
                if (__ballot(k < nL) == 0ull)
                    break;
            }
#endif
            if (sampleNext)
                lightK = nL;
        }
        if (sampleNext) {
            // ---- sampleLights (Shader.cpp:50-86), one light per trip ------------------------------
            bool shadowRay = false;
            while (!LISTS && lightK < (PRESAMPLE ? 1 : sc.nLights)) {
                // Lights whose sample is discarded whatever it is -- the ideal reflector asks for none (its pdf toward any
                // given direction is 0, BSDF.cpp:93-96), and a light that lies wholly below the vertex's horizon has
                // max(0, n.l) = 0 for every point of it -- only draw their random number (Light.cpp:39-41: one draw per
                // sample), in a loop of its own: the full sampling code below then runs for lights that can count. Scenes
                // of many lights only (16 lights: +6 % FAST, +25 % STRICT); with one light the test is pure overhead (-4.6 %).
                if (!COLD_LDS && sc.nLights >= 4) { // (large-scene kernels only: in the small-scene loop the extra code costs 5 % by itself)
                    for (; lightK < sc.nLights; lightK++) {
                        const int sk = lds.light[lightK];
                        if (np + 1 + sk == vId) // a light does not sample itself (and draws nothing)
                            continue;
                        const DSphereCold& lk = lds.lightCold[lightK];
                        const F3 toC = f3(lk.cx - vP.x, lk.cy - vP.y, lk.cz - vP.z);
                        const bool below = dot(vN, toC) < -(1.001f * lk.radius + 1e-6f * (__builtin_fabsf(toC.x) + __builtin_fabsf(toC.y) + __builtin_fabsf(toC.z)));
                        if (!(vKind == 2 || below))
                            break;
#if KAJO_STRICT
                        // (A light below the horizon adds nothing -- unless its sample is NOT A NUMBER, which the reference adds as NaN
                        // when its poisoned shadow walk ends on that light (see the skip on the cosine further down). That needs
                        // r^2 - x^2 - y^2 < 0, i.e. the sample's first uniform within rounding of 1: such a draw -- one in a million --
                        // goes through the sampling code, where the case is decided; only the diffuse lobe's pdf is NaN for a NaN direction.)
                        Rng peek = rng;
                        rngStep(peek);
                        if (vKind == 0 && unitBits((uint32_t)peek.lo) > 0.999999f)
                            break;
                        rng = peek;
#else
                        rngStep(rng);
#endif
                    }
                    if (lightK >= sc.nLights)
                        break;
                }
                const int si = lds.light[lightK];
                if (np + 1 + si == vId) { // a light does not sample itself
                    lightK++;
                    continue;
                }
                const DSphereCold& lc = lds.lightCold[lightK];
                float pl;
                // written straight into the ray: a discarded sample leaves d and O to the next light or to the BSDF sample
                d = lightGenerate(f3(lc.cx, lc.cy, lc.cz), lc.radius, vP, rng, pl);
                const F3 l = d;
#if !KAJO_RSTRICT
                pl = lightPdf(lc, vP);
#endif
                // The reference traces first and asks the BSDF afterwards; a zero BSDF pdf (always for
                // the reflector, outside the lobe for Phong) discards the sample either way, so the
                // trace is skipped for it.
                float pb;
                const F3 fl = bsdfEvaluateWithPdf(vKind, vColor, vExp, vR, vN, l, pb);
                // A light at or below the horizon contributes max(0, n.l) = 0 whatever the shadow ray
                // finds (the sum stays as it is: x + (+-0) == x), so that walk is skipped as well.
                const float cosL = kmax0(dot(vN, l));
                O = vP + l * kEps;
                // (... unless the sample is NOT A NUMBER: r^2 - x^2 - y^2 of Light.cpp:43-46 rounds below zero once in ~1e8 samples, its
                // square root makes the direction NaN, and the reference then adds f * max(0, NaN) * Le / (NaN + pl) = NaN when the
                // poisoned walk -- every comparison with NaN is false, so every object is "accepted" and the last one wins,
                // Raytracer.cpp:115 -- ends on the light. max(0, NaN) is 0 here as there, so the cosine alone would have skipped the
                // sample: two pixels of the 1080p x 16-pass frame, finite here and NaN in the reference, until round 4 compared whole frames.)
                // FAST, whose walk rejects NaN distances by their bit patterns, keeps skipping on the cosine (its loop has no scalar register
                // for the extra test, and its NaN pixels are counted, not matched).
                if (pl == 0.0f || pb == 0.0f || (cosL == 0.0f && KAJO_IS_A_NUMBER(pb))) {
                    lightK++;
                    continue;
                }
                const DFloat4 le = lds.lightEmission[lightK];
                const F3 Le = f3(le.x, le.y, le.z);
                pendContrib = ((rrcp(pb + pl) * fl) * cosL) * Le;
#if KAJO_INLINE_SHADOW
                if (!LISTS && COLD_LDS && !KAT && !SPLIT && !PRESAMPLE) {
                    // Small scenes, STRICT build: the shadow ray walks the scene right here (the closest-hit walk itself, so the
                    // answer is the walk's by construction) instead of costing its lane a trip of its own: with the blocks held
                    // until args.thrL lanes want them the walk runs for those lanes at once. STRICT +6.4 % on spheres.json, +20 %
                    // with three lights (profiles/r04_inline_shadow.txt). The FAST loop does not have the registers for it: at
                    // five waves per SIMD it spills 47 (-26 %), at four it loses the fifth wave (-10 %).
                    ctrShadow += 1;
                    const Hit sh = trace<false, 0, false, SIMPLE, NP, NS>(sc, lds, O, l);
                    if (sh.id == np + 1 + si) {
#if KAJO_RSTRICT
                        vLd = vLd + pendContrib;
#else
                        asm volatile("" : "+v"(pendContrib.x), "+v"(pendContrib.y), "+v"(pendContrib.z));
                        vE = vE + pendContrib;
#endif
                    }
                    lightK++;
                    continue;
                }
#endif
                mode = MODE_SHADOW;
                shadowRay = true;
                break;
            }
            // FAST, small scenes with one light (a kernel instance of their own: with several lights only the last light's visit
            // could take the BSDF along, which measured a loss -- profiles/r04_presample.txt): the extension ray is sampled in this
            // visit too (the random numbers come in the reference's order either way: the light's draw, then the BSDF's) and waits
            // out the shadow ray's trip in the registers of the vertex's normal and reflection vector, which nothing reads again.
            // The block then runs once per vertex instead of twice -- each visit with the lanes of both halves -- where it ran
            // with a fifth of the lanes per half; the arithmetic, and so every bit of the result, is the same. (STRICT walks the
            // shadow ray inside the light loop and has had the one visit since then.)
            const bool presample = PRESAMPLE && shadowRay;
            KAJO_PROF(7, !shadowRay || presample);
            if (!shadowRay || presample) {
                // ---- BSDF sampling (Shader.cpp:191-200) ------------------------------------------
                F3 tg = f3(0.0f, 0.0f, 0.0f), bn = tg;
                if (vKind == 0) {
                    if (vId <= np) {
                        const DFloat4 t4 = lds.planeFrame[3 * (vId - 1) + 1], b4 = lds.planeFrame[3 * (vId - 1) + 2];
                        tg = f3(t4.x, t4.y, t4.z);
                        bn = f3(b4.x, b4.y, b4.z);
                    } else {
                        sphereFrame(vN, tg, bn);
                    }
                }
                float p;
                F3 fd;
#if KAJO_RSTRICT
                const F3 dB = bsdfGenerate(vKind, vColor, vExp, vR, vN, tg, bn, rng, p, fd);
                vS = vSl;
                // The next segment's state is written unconditionally: a path that ends here (p == 0) re-initialises
                // all of it when its lane starts the next camera path, and unconditional writes need no copies.
                pendP = p;
                pendBsdf = true;
                pendF = fd;
                pendCos = kmax0(dot(vN, dB));
                pendT = T;
                depth++;
                if (presample) { // the shadow ray goes first (O, d hold it); the shadow-result block takes it from here
                    vN = dB;
                } else {
                    L = L + T * (vSl * (vE + vLd));
                    T = T * (vSl * ((krcp(0.0f + p) * pendF) * pendCos));
                    O = vP + dB * kEps;
                    d = dB;
                    if (p == 0.0f)
                        pathDone = true;
                    else
                        mode = MODE_EXTEND;
                }
#else
                const F3 dB = bsdfGenerate(vKind, vColor, vExp, vR, vN, tg, bn, rng, p, fd);
                const F3 w = vSl * ((rrcp(p) * fd) * kmax0(dot(vN, dB)));
                pendP = p;
                pendBsdf = true;
                depth++;
                if (presample) { // the shadow ray goes first (O, d hold it); the shadow-result block takes it from here
                    vN = dB;
                    vR = w;
                } else {
                    L = rmadd(T, vSl * vE, L);
                    // The next segment's state is written unconditionally: a path that ends here (p == 0) re-initialises
                    // all of it when its lane starts the next camera path, and unconditional writes need no copies.
                    T = T * w;
                    O = vP + dB * kEps;
                    d = dB;
                    if (p == 0.0f)
                        pathDone = true;
                    else
                        mode = MODE_EXTEND;
                }
#endif
            }
        }

        KAJO_STAMP(3); // light loop + BSDF sampling block
        if (pathDone) {
            if (bySample) // the path just finished is the one before the next sample to start
                termTable[((pass - args.firstPass) * n * n + sampleY * n + sampleX - 1) * 64 + lane] = DFloat4{L.x, L.y, L.z, 0.0f};
            else
                radiance = radiance + L; // Renderer.cpp:66
            mode = MODE_NEW;
            if (KAT) {
                reinterpret_cast<float4*>(args.katRgb)[slot] = make_float4(L.x, L.y, L.z, 0.0f);
                args.katFinal[2 * slot] = rng.lo;
                args.katFinal[2 * slot + 1] = rng.hi;
            }
        }
    }

    if (SPLIT) {
        __syncthreads(); // every wave of the block has left its loop: the table is complete
        if (splitWave == 0 && inImage) {
            // (GROUPS: `group` is the sum of the group of passes p is in, `total` the total the complete groups have been added to)
            F3 group = f3(0.0f, 0.0f, 0.0f);
            const uint32_t slotE = GROUPS ? __builtin_bit_cast(uint32_t, lds.camera[3].w) + (uint32_t)lane : slot;
            if (GROUPS && args.carryIn) {
                const float4 t = reinterpret_cast<const float4*>(args.carry)[slotE], g = reinterpret_cast<const float4*>(args.carry)[args.carrySlots + slotE];
                total = f3(t.x, t.y, t.z);
                totalW = t.w;
                group = f3(g.x, g.y, g.z);
            }
            for (int p = 0; p < args.nPasses; p++) { // Renderer.cpp:70-71, pass by pass
                if (GROUPS && ((args.firstPass + p - 1) & kGroupMask) == 0) { // pass firstPass + p begins a group (a zero is added where the launch begins one)
                    total = total + group;
                    group = f3(0.0f, 0.0f, 0.0f);
                }
                F3 term;
                if (bySample) {
                    F3 sum = f3(0.0f, 0.0f, 0.0f);
                    for (int k = 0; k < n * n; k++) { // Renderer.cpp:66, sample by sample
                        const DFloat4 t = termTable[(p * n * n + k) * 64 + lane];
                        sum = sum + f3(t.x, t.y, t.z);
                    }
#if KAJO_RSTRICT
                    term = f3(kdiv(sum.x, args.S), kdiv(sum.y, args.S), kdiv(sum.z, args.S));
#else
                    term = sum * invS;
#endif
                } else {
                    const DFloat4 t = termTable[p * 64 + lane];
                    term = f3(t.x, t.y, t.z);
                }
                if (GROUPS)
                    group = group + term;
                else
                    total = total + term;
            }
            if (GROUPS) {
                const DFloat4 c7 = lds.camera[7];
                KajoGlobalVec4* const carry = KAJO_GLOBAL_VEC4(c7.z, c7.w);
                if (carry) { // the launch ends inside a group
                    carry[slotE] = KajoVec4{total.x, total.y, total.z, totalW};
                    carry[__builtin_bit_cast(uint32_t, lds.camera[2].w) + slotE] = KajoVec4{group.x, group.y, group.z, 0.0f};
                }
                total = total + group;
            }
            reinterpret_cast<float4*>(args.tiles)[slotE] = make_float4(total.x, total.y, total.z, totalW);
        }
    } else if (!KAT && inImage) {
        if (LISTS_RMW) { // (the own passes' terms are in the buffer already)
            const float4 t4 = reinterpret_cast<const float4*>(args.tiles)[slot];
            total = f3(t4.x, t4.y, t4.z);
            totalW = t4.w;
        }
        // passes of this pixel that other lanes rendered, in pass order
        if (PARTS) {
            const uint32_t slotE = __builtin_bit_cast(uint32_t, lds.camera[3].w) + waveInGroup * 64u + (uint32_t)lane; // (+ threadIdx.x, from what is live)
            DFloat4 a = *accWordNow();
            for (int p = myEnd; p < lastPass; p++) {
                if (p > myEnd && ((p - 1) & kGroupMask) == 0) { // (a group that ended with the lane's own last pass is in the word already)
                    a = DFloat4{a.x + total.x, a.y + total.y, a.z + total.z, a.w};
                    total = f3(0.0f, 0.0f, 0.0f);
                }
                const DFloat4 t = mailbox[lane * stealWindow + (p - stealBase)];
                total = total + f3(t.x, t.y, t.z);
            }
            const DFloat4 c7 = lds.camera[7];
            KajoGlobalVec4* const carry = KAJO_GLOBAL_VEC4(c7.z, c7.w);
            if (carry) { // the launch ends inside a group (never a parted launch): its two summands wait for the next launch
                carry[slotE] = KajoVec4{a.x, a.y, a.z, a.w};
                carry[__builtin_bit_cast(uint32_t, lds.camera[2].w) + slotE] = KajoVec4{total.x, total.y, total.z, 0.0f};
            }
            total = f3(a.x + total.x, a.y + total.y, a.z + total.z); // the last group (a zero if it ended with a pass the lane rendered itself)
            totalW = a.w;
            // (the tile buffer, or the side buffer of a later part)
            KAJO_GLOBAL_VEC4(c7.x, c7.y)[slotE] = KajoVec4{total.x, total.y, total.z, totalW};
        } else {
            for (int p = myEnd; p < lastPass; p++) {
                const DFloat4 t = mailbox[lane * stealWindow + (p - stealBase)];
                total = total + f3(t.x, t.y, t.z);
            }
            reinterpret_cast<float4*>(args.tiles)[slot] = make_float4(total.x, total.y, total.z, totalW);
        }
    }
#undef lastPass
#undef stealBase
    if (!KAT && !SPLIT && args.waveTrips && lane == 0) // (the first launch of a handle: image order, no parts)
        args.waveTrips[(PARTS ? __builtin_bit_cast(uint32_t, lds.camera[3].w) + waveInGroup * 64u : slot) >> 6] = trips;

    if (counting && lane == 0) {
        atomicAdd(&args.counters[0], ctrTraversals);
        atomicAdd(&args.counters[2], ctrSlots);
#ifdef KAJO_PROFILE
        for (int k = 0; k < 16; k++)
            atomicAdd(&args.counters[4 + k], prof[k]);
        for (int k = 0; k < 9; k++)
            atomicAdd(&args.counters[20 + k], stampSum[k]);
#endif
    }
    if (counting) {
        // vertices and shadow queries are per lane: reduce over the wave first
        unsigned long long v = ctrVertices, q = ctrShadow;
        for (int o = 32; o > 0; o >>= 1) {
            v += __shfl_down(v, o);
            q += __shfl_down(q, o);
        }
        if (lane == 0) {
            atomicAdd(&args.counters[1], v);
            if (LISTS || KAJO_INLINE_SHADOW)
                atomicAdd(&args.counters[3], q);
        }
    }
}

} // namespace

#if defined(KAJO_FIXED_KERNELS)
// A unit of the SIMPLE kernel's instances with compile-time plane and sphere counts (kernel_exact_fixed.cpp): KAJO_FIXED_KERNELS(X) lists
// them as X(planes, spheres), fixed_counts.h names them. launch.inc.hip sends a SIMPLE scene of such counts here.
#define KAJO_FIXED_KERNEL(P, S) \
    extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD) KAJO_FIXED_NAME(P, S)(const RenderArgs args) \
    { \
        extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[]; \
        renderBody<true, false, false, false, true, 0, true, P, S>(args, ldsRaw); \
    }
KAJO_FIXED_KERNELS(KAJO_FIXED_KERNEL)
#undef KAJO_FIXED_KERNEL
#elif defined(KAJO_SIMPLE_KERNEL_NAME)
// A unit of one kernel (kernel_exact_simple.cpp): the one-light small-scene kernel for scenes of rigid planes and (centre, radius) spheres
// (trace SIMPLE), without the loops for general records. launch.inc.hip sends such scenes here; the kernels below, in the build's own unit,
// stay what they were and serve every other scene.
extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD) KAJO_SIMPLE_KERNEL_NAME(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<true, false, false, false, true, 0, true>(args, ldsRaw);
}
#else
// whole scene in LDS
#ifdef KAJO_KERNEL_NAME_LIGHTS
// (FAST: scenes with exactly one light have an instance of their own, see PRESAMPLE; it carries the mode's plain name because it is
// the one the headline workload runs)
extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD) KAJO_KERNEL_NAME(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<true, false, false, false, true>(args, ldsRaw);
}

#ifndef KAJO_WAVES_PER_SIMD_LIGHTS
#define KAJO_WAVES_PER_SIMD_LIGHTS KAJO_WAVES_PER_SIMD
#endif
extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD_LIGHTS) KAJO_KERNEL_NAME_LIGHTS(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<true, false>(args, ldsRaw);
}
#else
extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD) KAJO_KERNEL_NAME(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<true, false>(args, ldsRaw);
}
#endif

// small frames: the workgroup's waves share one pixel block and divide the passes (see renderBody)
extern "C" __global__ void __launch_bounds__(1024, KAJO_WAVES_PER_SIMD) KAJO_KERNEL_NAME_SPLIT(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<true, false, true>(args, ldsRaw);
}

// hot records in LDS, cold ones in global memory (large scenes)
#ifdef KAJO_KERNEL_NAME_BIG_LG
// (instances per home of the grid's cell lists -- LDS: the _lg names, global memory: the plain ones -- see gridWalk)
#define KAJO_GHOME_PLAIN 2
extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD_BIG) KAJO_KERNEL_NAME_BIG_LG(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<false, false, false, false, false, 1>(args, ldsRaw);
}

extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD_BIG) KAJO_KERNEL_NAME_BIGLIST_LG(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<false, false, false, true, false, 1>(args, ldsRaw);
}
#else
#define KAJO_GHOME_PLAIN 0
#endif
extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD_BIG) KAJO_KERNEL_NAME_BIG(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<false, false, false, false, false, KAJO_GHOME_PLAIN>(args, ldsRaw);
}

// large scenes with per-light visibility lists: shadow queries answered inside the light loop (renderBody LISTS)
extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD_BIG) KAJO_KERNEL_NAME_BIGLIST(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<false, false, false, true, false, KAJO_GHOME_PLAIN>(args, ldsRaw);
}

// known-answer kernels (kajo_hip_kat_shade / kajo_hip_kat_trace): the SAME device functions, fed rays
extern "C" __global__ void __launch_bounds__(256, KAJO_WAVES_PER_SIMD_BIG) KAJO_KAT_SHADE_NAME(const RenderArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    renderBody<false, true>(args, ldsRaw);
}

#ifdef KAJO_KAT_TRACE_NAME // (the EXACT build's walk IS the STRICT build's: it has no instance of its own)
extern "C" __global__ void __launch_bounds__(256) KAJO_KAT_TRACE_NAME(const KatTraceArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    const DSceneView& sc = args.scene;
    const LdsScene lds = stageToLds<false>(sc, ldsRaw);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= args.count)
        return;
    const F3 O = ld3(args.rays + 6 * i), d = ld3(args.rays + 6 * i + 3);
    const Hit h = trace<true>(sc, lds, O, d);
    float* o = args.out + 13 * i;
    args.idx[i] = h.id;
    o[0] = h.t;
    F3 P = f3(0.0f, 0.0f, 0.0f), N = P, tg = P, bn = P;
    if (h.id) {
        P = O + d * h.t;
        N = hitNormal(sc, lds, h, O, d);
        if (h.id <= sc.nPlanes) {
            const DFloat4 t4 = lds.planeFrame[3 * (h.id - 1) + 1], b4 = lds.planeFrame[3 * (h.id - 1) + 2];
            tg = f3(t4.x, t4.y, t4.z);
            bn = f3(b4.x, b4.y, b4.z);
        } else {
            sphereFrame(N, tg, bn);
        }
    }
    const F3 v[4] = {P, N, tg, bn};
    for (int k = 0; k < 4; k++) {
        o[1 + 3 * k] = v[k].x;
        o[2 + 3 * k] = v[k].y;
        o[3 + 3 * k] = v[k].z;
    }
}
#endif

// ---- resolve (Renderer.cpp:73-75 + Image::linearToSRGB / colorToRGBA8, Image.cpp:14-27) ----------
// frame: W*H float4 sums over passes; dst: ARGB8, row 0 = top.
#ifdef KAJO_RESOLVE_NAME // (the EXACT build resolves with the STRICT build's kernels)
extern "C" __global__ void __launch_bounds__(256) KAJO_RESOLVE_NAME(const float4* frame, int count, float passes, uint32_t* dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const float4 a = frame[i];
    const float in[3] = {a.x, a.y, a.z};
    int out[3];
    for (int k = 0; k < 3; k++) {
        float v = kdiv(in[k], passes);
        v = fminf(fmaxf(v, 0.0f), 1.0f);
        v = kpow(v, 1 / 2.2f);
        out[k] = (int)(v * 255.f + .5f);
    }
    const int al = (int)(1.f * 255.f + .5f);
    dst[i] = ((uint32_t)al << 24) | ((uint32_t)out[0] << 16) | ((uint32_t)out[1] << 8) | (uint32_t)out[2];
}

// The same resolve straight from compact tile buffers (one owner's own, or `tileCount` gathered ones in rank order): the
// composed whole frame -- W*H float4 written by kajo_compose and read back here -- is not needed to show an image.
extern "C" __global__ void __launch_bounds__(256) KAJO_RESOLVE_TILES_NAME(const float4* gathered, TileMap map, float passes, uint32_t* dst)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= map.W || y >= map.H)
        return;
    int owner;
    uint32_t slot;
    kajoTileSlot(map, x, y, &owner, &slot);
    const float4 a = gathered[(size_t)owner * map.slotsPerOwner + slot];
    const float in[3] = {a.x, a.y, a.z};
    int out[3];
    for (int k = 0; k < 3; k++) {
        float v = kdiv(in[k], passes);
        v = fminf(fmaxf(v, 0.0f), 1.0f);
        v = kpow(v, 1 / 2.2f);
        out[k] = (int)(v * 255.f + .5f);
    }
    const int al = (int)(1.f * 255.f + .5f);
    dst[(size_t)y * map.W + x] = ((uint32_t)al << 24) | ((uint32_t)out[0] << 16) | ((uint32_t)out[1] << 8) | (uint32_t)out[2];
}
#endif
#endif // KAJO_FIXED_KERNELS, KAJO_SIMPLE_KERNEL_NAME
