/*
 * kajo_hip.h -- C ABI of the MI355X rendering backend for Kajo (libkajo_hip.so).
 *
 * This is the drop-in boundary for ONE path of the reference: the per-pixel Monte-Carlo
 * integrator that cpu::Scheduler::run() drives through cpu::Renderer::render()
 * (renderer/cpu/Scheduler.cpp:60-85, renderer/cpu/Renderer.cpp:25-81). A backend in the
 * reference is a class with the constructor (const scene::Scene&, Image*, Preview*) and one
 * method run() (renderer/Scheduler.h:12-16, selected by name in renderer/Main.cpp:135-142);
 * kajo_amd/host/HipScheduler.{h,cpp} is that class for "-r hip", and everything it needs from
 * the GPU goes through the entry points below: plain pointers and sizes, int error codes, no
 * C++ / HIP / torch types in any signature.
 *
 * What each entry point replaces in the reference:
 *   kajo_hip_create          cpu::Renderer::Renderer + cpu::Scene::Scene (Renderer.cpp:17-23,
 *                            cpu/Scene.cpp:9-38): copy the scene, stage inverse matrices and
 *                            determinants, camera basis of Renderer.cpp:29-34
 *   kajo_hip_render          the pass loop of cpu::Renderer::render (Renderer.cpp:44-72) for
 *                            every pixel this handle owns, `passes` more passes, asynchronous
 *   kajo_hip_wait            joinTasks (cpu/Scheduler.cpp:44-51)
 *   kajo_hip_resolve_argb8   Renderer.cpp:73-75 + Image::linearToSRGB/colorToRGBA8
 *                            (renderer/Image.cpp:14-27) into Image::pixels (Image.h:18-20)
 *   kajo_hip_read_radiance   the radianceMap local of Renderer.cpp:36 (not observable in the
 *                            reference; exported here for parity tests)
 *   kajo_hip_counters        the samples/s bookkeeping of Preview::update (Preview.cpp:79-98)
 *   kajo_hip_read_aov        (no counterpart: the reference has no AOVs) the first-hit albedo, normal and depth a denoiser
 *                            takes beside the beauty image, over the beauty render's own camera samples (KAJO_FLAG_AOV)
 *   kajo_hip_denoise         (no counterpart: the reference has no denoiser) an edge-aware A-trous filter of the frame guided by
 *                            those AOVs, into buffers of its own; kajo_hip_default_denoise_params gives its defaults
 *   kajo_hip_tonemap_argb8   Image::linearToSRGB / colorToRGBA8 (renderer/Image.cpp:14-27) with an exposure, a tone curve and automatic
 *                            exposure in front of the clamp; kajo_hip_tonemap_gathered_argb8_device is its twin over gathered tile
 *                            buffers, kajo_hip_tone_scale reports the scale applied, kajo_hip_default_tone_params gives the defaults
 *   kajo_hip_glare           (no counterpart: the reference has no glare) a bloom pyramid between the frame and the tone curves;
 *                            kajo_hip_display_argb8 and kajo_hip_display_gathered_argb8_device run denoise -> glare -> tone mapping,
 *                            kajo_hip_default_glare_params gives the defaults
 *   kajo_hip_meter           (no counterpart: the reference has no metering) a luminance histogram of the frame in front of the tone
 *                            curves: percentile automatic exposure, automatic white point and the range the frame spans;
 *                            kajo_hip_present_metered_argb8 and its gathered twin put it into the display chain
 *   kajo_hip_local           (no counterpart: the reference has no local operator) an edge-aware base / detail compression of log
 *                            luminance between the glare and the meter; kajo_hip_present_local_argb8 and its gathered twin put it into
 *                            the display chain, kajo_hip_local_pivot reports the pivot used
 *   kajo_hip_lens            (no counterpart: the reference's camera is a pinhole, Renderer.cpp:29-55) depth of field as a lens blur from
 *                            the depth AOV between the denoiser and the glare; kajo_hip_present_lens_argb8 puts it into the display
 *                            chain, kajo_hip_lens_coc and kajo_hip_lens_depth_at report the circle of confusion and the depth it is from
 *   kajo_hip_view_argb8      (no counterpart: the reference writes its image at the rendered size, renderer/Image.cpp) crop, zoom and
 *                            supersampled output BEHIND the tone curves: a separable resampling of the ARGB8 image in linear light;
 *                            kajo_hip_present_view_argb8 and its gathered twin put it at the end of the display chain,
 *                            kajo_hip_view_weights and kajo_hip_view_tables are the host code that defines its numbers
 *   kajo_hip_grade           (no counterpart: the reference writes the colours it integrated) white balance, an ASC CDL op and per-object
 *                            regrades weighted by the coverage mattes, between the denoiser and the lens; kajo_hip_present_grade_argb8
 *                            and its gathered twin put it into the display chain, kajo_hip_grade_pixels, kajo_hip_grade_white_balance
 *                            and kajo_hip_grade_neutral are the host code that defines its numbers
 *   kajo_hip_destroy         the unique_ptr members of cpu::Scheduler (cpu/Scheduler.h:29-31)
 *
 * Pixels are dealt to GPUs as fixed-size tiles: a handle created with
 * (tileIndex, tileCount) accumulates the tiles t with t % tileCount == tileIndex in a compact
 * device buffer; kajo_hip_tile_buffer exposes it for the one RCCL gather per frame that the
 * host performs (torch.distributed or rccl directly), kajo_hip_compose places the gathered
 * buffers into the whole frame on the root handle. Every camera path draws from its own RNG
 * stream (include/kajo_stream.h), so the frame is bit-identical for any tiling / GPU count.
 *
 * Threading: a handle is not re-entrant; distinct handles are independent (section 8b).
 * All calls return 0 on success or a negative KAJO_E_* code; kajo_hip_last_error() gives the
 * message of the calling thread's most recent failure. No exception crosses this boundary.
 */
#ifndef KAJO_HIP_H
#define KAJO_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "kajo_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KAJO_OK 0
#define KAJO_E_INVALID (-1)   /* bad argument */
#define KAJO_E_HIP (-2)       /* a HIP runtime call failed (message has the HIP error) */
#define KAJO_E_NO_DEVICE (-3) /* no usable GPU: the backend never falls back to the CPU */
#define KAJO_E_STATE (-4)     /* call not valid in the handle's current state */

/* KajoParams.flags */
#define KAJO_FLAG_FAST 0u     /* (the absence of KAJO_FLAG_STRICT and KAJO_FLAG_EXACT) fast numerics: hardware transcendentals, contracted
                                   multiply-adds. The fastest build; it does NOT meet BASELINE's per-pixel RMSE < 1e-4 on spheres.json at
                                   1920x1080 x 16 passes (6e-4: a few paths per million flip a hit / miss decision). Opt in by clearing
                                   the flags kajo_hip_default_params sets. */
#define KAJO_FLAG_STRICT 1u   /* strict numerics: bit-identical to the CPU oracle (slower). Like KAJO_FLAG_EXACT it forms the IEEE quotient
                                   and square root of the closest-hit walk by hand, which is exact for operands of ordinary size only:
                                   kajo_hip_create refuses a scene with a non-zero coordinate (object and camera transforms, radii) outside
                                   2^-40 .. 2^40 in magnitude with KAJO_E_INVALID under either flag */
#define KAJO_FLAG_COUNTERS 2u /* maintain device-side work counters */
#define KAJO_FLAG_NO_GRID 4u  /* always walk every sphere (no uniform grid for large scenes) */
#define KAJO_FLAG_NO_REORDER 8u /* dispatch workgroups in image order (no cost-sorted launch order) */
#define KAJO_FLAG_COOP 32u      /* EXPERIMENT, round 2 (measured slower, profiles/HISTORY.md section 8; only in kajo_amd/libkajo_hip_r02.so of `make
                                   experiments`, refused by the product library): the 8 waves of a workgroup pool their rays in LDS every
                                   trip, counting-sort them by kind and octant into a compact queue and walk that */
#define KAJO_FLAG_DEFERRED 64u  /* EXPERIMENT, round 3 (measured slower, profiles/HISTORY.md section 8; only in kajo_amd/libkajo_hip_exp.so of `make
                                   experiments`, refused by the product library): surviving vertices are parked in LDS and the light / BSDF
                                   sampling blocks run only in trips where enough lanes have one (deferred.inc.hip) */
#define KAJO_FLAG_NO_SPLIT 16u  /* small frames: do not let several waves share a pixel block and divide the passes; large frames
                                   (FAST / EXACT): do not render the cheapest blocks of a launch in parts (KajoCounters.tailGroups).
                                   Scheduling only: the frame is the same bit for bit with and without */
#define KAJO_FLAG_NO_SHADOW_LISTS 128u /* large scenes: shadow rays walk the uniform grid as extension rays do, instead of being answered
                                   from the lights' visibility lists inside the light loop (same results; for A/B runs and tests) */
#define KAJO_FLAG_EXACT 512u  /* decision-exact numerics (the default of kajo_hip_default_params): the oracle's arithmetic (KAJO_FLAG_STRICT's)
                                   wherever a value can reach a decision -- the closest-hit walk, hit points, normals, sampled directions,
                                   coins -- so every path meets the oracle's objects, draws its random numbers and ends in its generator
                                   state; the fast forms where a value only scales radiance (BSDF values and pdfs, the light pdf, MIS
                                   weights, throughput products). Tolerance against KAJO_FLAG_STRICT's (= the oracle's) buffer, asserted
                                   by the whole-frame tests: the same pixels are not-a-number; every other pixel's sum differs by at most
                                   KAJO_EXACT_REL_TOL of max(|oracle|, KAJO_EXACT_ABS_FLOOR * passes) per channel (measured: 9.2e-4 at
                                   worst, where the oracle's light pdf 1 - cos(asin(r / d)) cancels); clamped per-pixel RMSE of the
                                   estimate 6.5e-7 on spheres.json at 1920x1080 x 16 passes. Not with KAJO_FLAG_STRICT. */
#define KAJO_EXACT_REL_TOL 1.5e-3f
#define KAJO_EXACT_ABS_FLOOR 1e-3f
#define KAJO_FLAG_NO_ONE_LIGHT 256u /* small scenes with exactly one light, every numerics build: run the kernel instance of any number of lights
                                   (kajo_render_*_lights) instead of the one that samples the BSDF in the light's visit (same results in the
                                   FAST and EXACT builds bit for bit and in the STRICT build, which stays the oracle; the hold thresholds
                                   stay those of the scene's own instance; for A/B runs and tests) */
#define KAJO_FLAG_AOV 1024u   /* first-hit AOVs for denoisers (kajo_hip_read_aov): create() allocates and zeroes two whole-frame float4 buffers
                                   (2 x W x H x 16 bytes) and every kajo_hip_render enqueues one more kernel per render launch, on the handle's
                                   stream, over the same passes' camera samples. Whole frame on one handle only: with tileCount != 1 create()
                                   refuses the flag (KAJO_E_INVALID) unless KAJO_FLAG_AOV_TILED is set with it. Without it nothing is
                                   allocated or launched. */
#define KAJO_FLAG_AOV_SPECULAR 2048u /* with KAJO_FLAG_AOV only (alone: KAJO_E_INVALID at create, before a device is looked for): the AOVs are
                                   taken at the first NON-DELTA hit -- camera rays are followed through ideal mirrors and glass by the
                                   deterministic chain defined at kajo_hip_read_aov, so that the guides show what the mirror shows. The
                                   same buffers and entry points; another kernel instance (kajo_hip_aov_kernel: ..._spec...). Handles
                                   without the flag launch what they launched before. */
#define KAJO_AOV_MAX_FOLLOW 8     /* the chain's longest: delta surfaces followed per camera sample */
#define KAJO_FLAG_AOV_MATTE 4096u /* with KAJO_FLAG_AOV only (alone: KAJO_E_INVALID at create, before a device is looked for): object-coverage
                                   mattes beside the AOVs -- per pixel a table of KAJO_MATTE_SLOTS (object id, sample count) pairs over the
                                   AOVs' own samples (kajo_hip_read_matte, kajo_hip_matte_mask). create() allocates and empties the tables
                                   (W x H x 64 bytes); the handle launches another instance of the AOV kernel (kajo_hip_aov_kernel:
                                   ..._matte...), still one per render launch and one scene walk per sample. Handles without the flag
                                   launch what they launched before. */
#define KAJO_MATTE_SLOTS 8        /* (id, count) pairs per pixel */
#define KAJO_FLAG_AOV_TILED 8192u /* with KAJO_FLAG_AOV only (alone: KAJO_E_INVALID at create, before a device is looked for): tiled AOVs, for
                                   any tileIndex / tileCount. The handle keeps the AOV sums (and with KAJO_FLAG_AOV_MATTE the coverage tables)
                                   of its OWN tiles only, in the tile layout of the accumulation, and its AOV kernel runs over those tiles;
                                   the whole-frame buffers every AOV reader takes are formed by kajo_hip_compose_aov from the owners'
                                   gathered tile buffers (kajo_hip_aov_tile_buffers). Combines with KAJO_FLAG_AOV_SPECULAR and
                                   KAJO_FLAG_AOV_MATTE; the same kernel instances (kajo_hip_aov_kernel). The frame of such a handle is
                                   at most 524288 x 262144 pixels, a tile at most 524280 a side (KAJO_E_INVALID). Handles without the
                                   flag allocate, launch and refuse what they did before. */
#define KAJO_FLAG_NOISE 16384u /* the per-pixel noise estimate ("The noise estimate" below; kajo_hip_noise): create() allocates and zeroes a
                                   baseline (16 bytes) and a moment record (32 bytes) per slot of the handle's tile buffer, for any tileIndex /
                                   tileCount and in every numerics build. kajo_hip_render then cuts its launches so that none crosses an
                                   absolute multiple of KAJO_NOISE_BATCH_PASSES -- the frame is the same bit for bit, KajoCounters.launches
                                   rises -- and enqueues the update kernel of kajo_amd/csrc/noise.hip behind each launch that ends on one,
                                   outside the timing events. No render, AOV or display kernel is changed for it. Handles without the flag
                                   allocate, launch and return exactly what they did before. */
#define KAJO_FLAG_ADAPTIVE 32768u /* with KAJO_FLAG_NOISE only (alone: KAJO_E_INVALID at create, before a device is looked for): adaptive
                                   sampling ("Adaptive sampling" below; kajo_hip_set_adaptive): units of the frame whose noise estimate has
                                   met a target are retired, and later launches render the others only. create() allocates a state word per
                                   unit; until kajo_hip_set_adaptive is called nothing retires and the handle does what a KAJO_FLAG_NOISE
                                   handle does. No render, AOV or display kernel is changed for it; handles without the flag allocate,
                                   launch and return exactly what they did before. */

typedef struct KajoParams {
    int32_t samplesPerPass; /* S: nominal samples per pixel per pass (reference: 32, Renderer.cpp:21);
                               n = floor(sqrt(S)) strata per axis are traced, the sum is divided by S */
    int32_t depthLimit;     /* reference: 8 (Shader.cpp:24); 0 .. 1000 */
    uint64_t seed;          /* stream seed (reference constant 0715517 = 236367, Random.h:43) */
    uint32_t flags;         /* KAJO_FLAG_* */
    int32_t device;         /* HIP device ordinal */
    int32_t tileW, tileH;   /* tile size in pixels: multiples of 8 with tileW * tileH a multiple of 256; 0 => 64 x 16 */
    int32_t tileIndex;      /* this handle renders tiles t with t % tileCount == tileIndex */
    int32_t tileCount;      /* number of handles sharing the frame (GPUs); 0 => 1 */
    int32_t passesPerLaunch; /* passes fused into one kernel launch; 0 => library default */
} KajoParams;

typedef struct KajoCounters {
    uint64_t passes;         /* passes rendered so far */
    uint64_t paths;          /* camera paths = pixels * n^2 * passes: the NOMINAL count, also on a KAJO_FLAG_ADAPTIVE handle, whose retired
                                units trace none (the paths actually traced: KajoAdaptState.paths) */
    uint64_t traversals;     /* closest-hit scene walks (device counter; 0 without KAJO_FLAG_COUNTERS) */
    uint64_t vertices;       /* shaded path vertices (device counter) */
    uint64_t primitiveTests; /* traversals * (nPlanes + nSpheres): what walking every object costs; with
                                the uniform grid of large scenes the spheres actually tested are fewer */
    uint64_t laneSlots;      /* 64 * wave-iterations of the trace loop: traversals / laneSlots = lane efficiency */
    double kernelMs;         /* summed device time of the render kernels (HIP events on the handle's stream; not the AOV kernel of
                                KAJO_FLAG_AOV, which runs outside them) */
    uint64_t launches;       /* render kernel launches (a KAJO_FLAG_NOISE handle cuts them at every multiple of four passes: more of them) */
    uint64_t shadowQueries;  /* large scenes: shadow rays answered from the lights' visibility lists inside the light loop (they
                                are not among `traversals`, which then counts camera and extension rays only) */
    uint64_t tailGroups;     /* of the last render launch: workgroups beyond one per pixel block -- the cheapest blocks of a large frame
                                of a small scene are rendered as one workgroup per group of four passes of the launch, so that the launch
                                ends on short jobs (FAST / EXACT, launches of 2 .. 8 whole groups; the frame is the same bit for bit;
                                0 = not parted) */
} KajoCounters;

typedef struct KajoHip* kajo_hip_t;

/* Fills *p with the reference's constants -- S = 32, depth 8, seed 236367, one tile set -- and flags = KAJO_FLAG_EXACT: the fastest
   numerics build that meets BASELINE's per-pixel RMSE < 1e-4 against the reference. */
void kajo_hip_default_params(KajoParams* p);

int kajo_hip_create(const KajoScene* scene, int width, int height, const KajoParams* params, kajo_hip_t* out);
int kajo_hip_destroy(kajo_hip_t h); /* NULL is accepted */

/* Enqueue `passes` more passes (pass numbers continue from the handle's count, first = 1; at most 2^31 - 1 in all).
   The frame after P passes is a function of the scene, the parameters and P alone -- not of how the passes were cut into render()
   calls, launches (passesPerLaunch), workgroups or GPUs. STRICT adds the passes' terms radiance / S to a pixel's total one by one, as
   the reference does (Renderer.cpp:70-71); FAST and EXACT (small scenes) add them in groups of four passes by absolute number
   (1-4, 5-8, ...): a group is summed from zero in pass order, then added to the total; a group in progress is added last.
   Across PROCESSES the same holds for a session continued through kajo_hip_checkpoint_save / kajo_hip_checkpoint_restore, at any pass
   count; through kajo_hip_set_pass_count and a restored tile buffer it holds for FAST / EXACT only at pass counts that are multiples of
   four (KAJO_GROUP_PASSES), since the summands of a group in progress are not in that buffer. */
int kajo_hip_render(kajo_hip_t h, int passes);
int kajo_hip_wait(kajo_hip_t h);
/* Zero the accumulation (and the AOV buffers, their sample count and the coverage tables of KAJO_FLAG_AOV_MATTE) and restart the pass
   numbering at 1. */
int kajo_hip_reset(kajo_hip_t h);
/* Continue a progressive session from pass `passesDone`: the next pass rendered is passesDone + 1 (the reference's loop
   `for (pass = 1;; pass++)`, Renderer.cpp:44, has no end). The call does not touch the accumulation buffer and DECLARES
   that it holds the sum of `passesDone` passes: kajo_hip_resolve_* divide by the pass count and kajo_hip_counters reports
   it, so the caller restores the buffer of the session being continued through kajo_hip_tile_buffer() first (or calls
   kajo_hip_reset() and set_pass_count(0)). FAST / EXACT: a passesDone inside a group of four continues from the buffer as
   one sum (the passes of the group so far are not known apart). Pass numbers run to 2^31 - 2. The AOV buffers of KAJO_FLAG_AOV are not
   touched: later passes are traced with their own pass numbers' streams and added to them; nor are the tables of KAJO_FLAG_AOV_MATTE.
   To continue a session exactly -- inside a group, with its noise moments, its AOVs, its counters or its adaptive state -- use
   kajo_hip_checkpoint_save and kajo_hip_checkpoint_restore ("Checkpoints" below) instead. */
int kajo_hip_set_pass_count(kajo_hip_t h, int passesDone);

/* Whole-frame outputs; valid when tileCount == 1, or on a handle that has been composed.
   dst are HOST pointers: width*height uint32 ARGB8 (row 0 = top) / width*height*4 floats
   (sum over passes of radiance / S; divide by the pass count for the estimate). They wait for
   outstanding passes. */
int kajo_hip_resolve_argb8(kajo_hip_t h, uint32_t* dst);
int kajo_hip_read_radiance(kajo_hip_t h, float* dst);
/* Same, into DEVICE memory (e.g. a mapped preview buffer), asynchronous on the handle's stream. */
int kajo_hip_resolve_argb8_device(kajo_hip_t h, void* dst);

/* Multi-GPU plumbing. The tile buffer is ceil(T / tileCount) tiles of tileW*tileH float4 each
   (T = tiles in the frame), identical size on every rank so that one gather moves it. */
int kajo_hip_tile_buffer(kajo_hip_t h, void** devicePtr, size_t* bytes);
/* gathered = DEVICE pointer to tileCount consecutive tile buffers in rank order (what a gather
   to this rank produced); composes them into this handle's whole-frame buffer. With
   tileCount == 1 composition happens implicitly. */
int kajo_hip_compose(kajo_hip_t h, const void* gathered);

/* The ARGB8 image straight from gathered tile buffers (DEVICE pointer, tileCount consecutive buffers in rank order; NULL = this
   handle's own buffer when tileCount == 1), into DEVICE memory, asynchronous on the handle's stream: compose + resolve in
   one pass over the data, without the whole-frame float buffer (renderer/cpu/Renderer.cpp:70-75 per pixel, as
   kajo_hip_resolve_argb8_device). kajo_hip_compose stays for kajo_hip_read_radiance. */
int kajo_hip_resolve_gathered_argb8_device(kajo_hip_t h, const void* gathered, void* dst);

/* First-hit AOVs (KAJO_FLAG_AOV), the buffers a denoiser takes beside the beauty image. The samples are the beauty render's camera samples
   and no others: every pass rendered into the handle, every stratum (sx, sy) of n = floor(sqrt(S)), the same jittered ray from the same
   stream key (include/kajo_stream.h; renderer/cpu/Renderer.cpp:51-64). Per sample, h = the kernels' own closest-hit walk of that ray:
     hit     1 if h hit an object, else 0
     albedo  hit: min(max((diffuse + specular) + transparency, 0), 1) per RGB channel of the hit object's material, in that order of
             operations (the three lobe colours of Shader.cpp:129-131); miss: backgroundColor.rgb, unclamped (what the path returns,
             Shader.cpp:116-117)
     normal  hit: the world-space normal of the hit as kajo_hip_kat_trace reports it (not flipped towards the ray); miss: 0
     depth   hit: the ray's maxDistance (t of the unit-length camera direction); miss: 0
   Per pixel two float4 sums, A = (sum albedo.rgb, sum hit) and B = (sum normal.xyz, sum depth), formed in float32 one sample at a time, in
   pass order and then stratum order sy * n + sx. So the buffers are a function of (scene, parameters, passes rendered), not of how the
   passes were cut into render() calls or launches. The hit count is exact up to 2^24 samples per pixel.
   STRICT handles give the oracle's walk and normals bit for bit; EXACT handles compute the AOVs with STRICT's arithmetic (its walk and
   normals are STRICT's); FAST handles with FAST's.
   albedoHits, normalDepth: HOST pointers to width*height*4 floats (row 0 = top), A and B; either may be NULL. *samples (may be NULL):
   n^2 x the passes rendered into the buffers since create() or kajo_hip_reset() (mean albedo = A.rgb / samples, mean normal =
   B.xyz / samples, mean depth of the hits = B.w / A.w). Waits for outstanding work. KAJO_E_STATE on a handle created without the flag. */
int kajo_hip_read_aov(kajo_hip_t h, float* albedoHits, float* normalDepth, int64_t* samples);
/* With KAJO_FLAG_AOV_SPECULAR a sample's contribution is taken at the end of a deterministic chain instead of at the first hit: same
   camera ray, same stream key (no random number is drawn), same order of summation, one float32 addition per word and sample.
     T = (1, 1, 1);  D = 0;  ray = the camera ray;  h = the closest-hit walk of ray
     at most KAJO_AOV_MAX_FOLLOW times, while h is a hit, with m = the hit object's material:
         tD, tS, tT = x + y + z of m.diffuse, m.specular, m.transparency       (Shader.cpp:130-132)
         pT = tT / (tD + tS + tT);  pD = tD / (tD + tS)                         (Shader.cpp:133,153: the integrator's own coins)
         if      pT >= 0.5:                              d' = the ideal-transmission direction (BSDF.cpp:105-124 with glm::refract,
                                                              ior = m.refractiveIndex, its total-internal-reflection branch included)
         else if m.specularExponent == 0 and pD < 0.5:   d' = reflect(view, normal)   (BSDF.cpp:82-85)
         else stop                   (comparisons with NaN are false: a material with no lobe at all stops the chain)
         if d' == (0, 0, 0): stop
         T = T * min(max(m.specular.rgb, 0), 1)          (both delta lobes carry the SPECULAR colour, Shader.cpp:137-139)
         D = D + h.t
         ray = (h.position + d' * 1e-3, d')              (the integrator's extension ray, Shader.cpp:23,197-198)
         h = the closest-hit walk of ray
     the final h is a hit:   albedo = T * (the albedo above of its material), normal = the world-space normal of the FINAL hit (not
                             flipped), depth = D + h.t (the length of the whole chain), hit = 1
     the final h is a miss:  albedo = T * backgroundColor.rgb, normal = 0, depth = 0, hit = 0
   A chain still on a followed surface after KAJO_AOV_MAX_FOLLOW follows ends there: that surface is the final hit. view, normal and
   position are what the integrator's vertex code forms for the same hit (view = the ray's direction, position = origin + direction * t);
   STRICT and EXACT handles use STRICT's arithmetic for every step, FAST handles FAST's. A scene without such materials gives the
   first-hit buffers bit for bit (T = 1 multiplies exactly, D = 0 adds exactly). In spheres.json the rule picks the mirror wall and the
   glass sphere and nothing else.
   kajo_hip_denoise and kajo_hip_tonemap_argb8(..., denoise) read A and B as before: nothing in the filter's definition changes; its
   albedo, normal and depth edges and its demodulation are then those of what is seen in the mirror or through the glass, the albedo
   tinted by the surfaces looked through and the depth measured along the whole chain. */
/* Name of the AOV kernel instance the handle launches (one per scene class, as the render kernels: the whole scene in LDS; the grid's cell
   lists in LDS or in global memory; with or without visibility lists), or NULL without KAJO_FLAG_AOV. For tests and profiles. */
const char* kajo_hip_aov_kernel(kajo_hip_t h);

/* Object-coverage mattes (KAJO_FLAG_AOV_MATTE with KAJO_FLAG_AOV): which object is in a pixel, and how much of the pixel it covers.
     object id  the one kajo_hip_kat_trace reports: 0 for a miss, 1..nPlanes the planes, then the spheres
     samples    the AOVs' samples and no others: every pass, every stratum, the same camera ray, in pass order and then stratum order
                sy * n + sx. A sample's id is that of the h its albedo is taken from: the first hit, or with KAJO_FLAG_AOV_SPECULAR the
                FINAL hit of the chain above (the object seen in the mirror or through the glass)
     table      per pixel KAJO_MATTE_SLOTS slots (id, count), counts uint32; every slot is empty after create() and kajo_hip_reset()
     per sample if a slot holds the sample's id (0 included), its count grows by 1; otherwise the first empty slot takes the id with
                count 1; otherwise -- eight other ids came first -- the sample is dropped. So dropped(p) = samples - sum of counts(p)
   The table is a function of (scene, parameters, passes rendered), not of how the passes were cut into render() calls or launches: it
   lives in the buffer between launches, as A and B do. kajo_hip_set_pass_count leaves it alone. STRICT and EXACT handles take the ids
   from STRICT's walk, FAST handles from FAST's; everything after the walk is integer arithmetic, the same in every build.
   kajo_hip_read_matte: the tables RANKED -- per pixel the slots by count descending, ties by id ascending, empty slots last as
   (id -1, count 0). ids, counts: HOST pointers to width*height*KAJO_MATTE_SLOTS words (row 0 = top, a pixel's slots consecutive);
   *samples: kajo_hip_read_aov's. Any of the three may be NULL. Waits for outstanding work.
   kajo_hip_matte_mask: mask(p) = float32(sum of the counts of p's slots whose id is among objects[0 .. n)) / float32(samples), one
   division, 0 with no pass rendered; dominant(p) = the id kajo_hip_read_matte puts first, as float32 (-1 for an empty table). objects:
   ids in 0 .. nPlanes + nSpheres, repeats allowed (an id counts once), n == 0 (objects may then be NULL) gives a mask of zeros; mask,
   dominant: HOST pointers to width*height floats, either may be NULL. Waits.
   Both: KAJO_E_INVALID on a NULL handle (kajo_hip_matte_mask also: n < 0, NULL objects with n > 0, an id out of range); KAJO_E_STATE on a
   handle created without the flag. The tables are only read by kernels of their own (kajo_amd/csrc/matte.hip) into scratch allocated on
   the first call; the accumulation, the AOV buffers, the pass count and the counters (kernelMs included) are not touched. */
int kajo_hip_read_matte(kajo_hip_t h, int32_t* ids, uint32_t* counts, int64_t* samples);
int kajo_hip_matte_mask(kajo_hip_t h, const int32_t* objects, int n, float* mask, float* dominant);

/* Tiled AOVs (KAJO_FLAG_AOV_TILED with KAJO_FLAG_AOV). A pixel's AOV sums and its coverage table are formed by one lane, sample after sample in
   pass order and then stratum order, from streams keyed by the pixel's index in the whole frame: they are the same words whoever owns the
   pixel's tile. A tiled handle keeps them for its own tiles:
     the AOV tile buffer    float4 A[slotsPerOwner] (albedo.rgb sums, hits) followed by float4 B[slotsPerOwner] (normal.xyz sums, depth sum)
     the matte tile buffer  (KAJO_FLAG_AOV_MATTE) uint4 ids[slotsPerOwner][2] followed by uint4 counts[slotsPerOwner][2], first-come order
   a pixel at the slot it has in the accumulation's tile buffer (kajo_hip_tile_buffer; slotsPerOwner = its bytes / 16). Both have the same
   size on every owner, padding included; they are zeroed at create and by kajo_hip_reset, and the padding (slots of no pixel: tiles cut by
   the frame's edges, owners with a tile fewer) stays zero. An owner without a tile launches no AOV kernel. kajo_hip_set_pass_count leaves
   them alone.
   kajo_hip_aov_tile_buffers: the DEVICE pointers and sizes, for one gather per buffer: *aovBytes = 2 * slotsPerOwner * 16, *matteBytes =
   slotsPerOwner * 64; without the matte flag *matte = NULL and *matteBytes = 0. Any out pointer may be NULL. KAJO_E_INVALID on a NULL
   handle, KAJO_E_STATE on a handle without KAJO_FLAG_AOV_TILED.
   kajo_hip_compose_aov: on any handle with the flag ("the root"), scatters gathered tile buffers into whole-frame row-major buffers in the
   one-owner handle's layout (W x H x 32 bytes of sums, W x H x 64 bytes of tables, allocated on the root at the first call), with one
   kernel on the handle's stream; asynchronous. gatheredAov / gatheredMatte: DEVICE pointers to tileCount consecutive AOV / matte tile
   buffers in rank order; NULL = the handle's own buffer when tileCount is 1, while with tileCount > 1 a NULL gatheredAov is KAJO_E_INVALID
   and a NULL gatheredMatte on a matte handle composes the sums only (the matte readers then stay KAJO_E_STATE). gatheredMatte is ignored
   without the matte flag. The call DECLARES that the gathered buffers hold the root's own AOV pass count, as kajo_hip_set_pass_count
   declares for the accumulation: *samples of the readers is reported from that count. KAJO_E_INVALID on a NULL handle, KAJO_E_STATE on a
   handle without the flag.
   After it -- and after kajo_hip_compose for the float frame where the accumulation is read (tileCount > 1) -- kajo_hip_read_aov,
   kajo_hip_read_matte, kajo_hip_matte_mask, kajo_hip_denoise and the `denoise` argument of kajo_hip_tonemap_argb8, kajo_hip_glare,
   kajo_hip_display_argb8, kajo_hip_present_argb8, kajo_hip_meter, kajo_hip_present_metered_argb8, kajo_hip_local and
   kajo_hip_present_local_argb8 behave on the root exactly as on a one-owner handle without the flag that rendered the same passes. On a
   tiled handle (tileCount 1 too) they give KAJO_E_STATE before the first kajo_hip_compose_aov and again after any kajo_hip_render of at
   least one pass or kajo_hip_reset that followed the last one. The accumulation, the tile buffers, the pass count and the counters
   (kernelMs included) are not touched by either call; the whole-frame buffers are freed by kajo_hip_destroy. */
int kajo_hip_aov_tile_buffers(kajo_hip_t h, void** aov, size_t* aovBytes, void** matte, size_t* matteBytes);
int kajo_hip_compose_aov(kajo_hip_t h, const void* gatheredAov, const void* gatheredMatte);

/* Edge-aware A-trous denoiser (Dammertz et al. 2010) guided by the first-hit AOVs, its luminance weight scaled by a spatial variance
   estimate (the spatial part of SVGF, Schied et al. 2017). A post-process over the handle's whole frame, in kernels of its own
   (kajo_amd/csrc/denoise.hip) on the handle's stream, in float32 IEEE arithmetic without contraction in every numerics build: only its
   inputs depend on FAST / EXACT / STRICT. Definition -- P = the handle's pass count, s = kajo_hip_read_aov's *samples (1 where no AOV
   sample was taken); per pixel p:
     c = sum.rgb / P                      mean radiance (sum: the accumulation, kajo_hip_read_radiance)
     a = A.rgb / s                        albedo (A, B: kajo_hip_read_aov)
     N = normalize(B.xyz), 0 where |B.xyz| = 0;  z = B.w / A.w, 0 where A.w = 0
     e = c / max(a, 1e-3) per channel     (demodulation; with KAJO_DENOISE_NO_DEMODULATE e = c)
     l(e) = 0.2126 r + 0.7152 g + 0.0722 b
   A pixel COUNTS where e is finite (all three channels). v0(p) = the variance of l over the 3x3 window around p, over the counted
   pixels inside the image (E[l^2] - E[l]^2, formed about the window's mean; 0 at a pixel that does not count). Iteration i = 0 .. K-1,
   step d = 2^i, taps q = p + d (dx, dy), dx, dy in -2..2, h = [1/16, 1/4, 3/8, 1/4, 1/16]:
     w   = h[dx] h[dy] w_z w_n w_l
     w_z = exp(-|z_p - z_q| / (sigmaDepth * max(z_p, z_q, 1e-4) * |(dx, dy)| * d / max(W, H)));  1 at the centre tap
     w_n = max(0, dot(N_p, N_q))^sigmaNormal;  1 where either normal is 0 (no hit)
     w_l = exp(-|l_p - l_q| / (sigmaLuminance * sqrt(g(v_i)(p)) + 1e-6)), g = the 3x3 [1/4, 1/2, 1/4] blur of v_i over the counted
           pixels inside the image, renormalised over them;  1 where p does not count
     (an exp whose numerator is 0 is 1)
     e_{i+1}(p) = sum(w e_i(q)) / sum(w),   v_{i+1}(p) = sum(w^2 v_i(q)) / sum(w)^2
   over the taps inside the image that count (no edge clamping; the weights are renormalised over the taps that remain). A pixel that
   does not count takes the weighted mean of the taps that do, its own tap skipped: the denoiser repairs NaN / Inf pixels and never
   spreads them. Where no tap counts (sum(w) = 0) e is NaN and v 0. Output: e_K * max(a, 1e-3) * P (demodulated) or e_K * P, in the
   units of kajo_hip_read_radiance (sums over passes), .w copied from the accumulation. K = 0: a copy of the accumulation (no
   demodulation), so its ARGB8 equals kajo_hip_resolve_argb8 bit for bit.
   radiance: HOST pointer to width*height*4 floats (row 0 = top); argb8: HOST pointer to width*height words, the output resolved by the
   handle's own resolve kernel with P passes, as kajo_hip_resolve_argb8; either may be NULL. Waits for outstanding work. The
   accumulation, the AOV buffers, the pass count and the counters (kernelMs included) are not touched. Scratch (three float4 frames and
   one ARGB8 frame) is allocated on the first call and freed by kajo_hip_destroy.
   KAJO_E_INVALID: a NULL handle or params, iterations outside 0..8, a negative or non-finite sigma. KAJO_E_STATE: a handle created
   without KAJO_FLAG_AOV, or with no pass rendered.
   NOISE-GUIDED (KAJO_DENOISE_NOISE_GUIDED in flags, iterations >= 1; kajo_amd/csrc/denoise_guided.cpp): the filter above word for word --
   the counted pixels, the guides, g(v), the taps, the weights, the NaN repair, the remodulation and .w -- with another v0: the MEASURED
   variance of the pixel where there is one (SVGF steers this weight by the measured per-pixel variance and keeps the spatial estimate
   for pixels without history). For a counted pixel p let m and se be the float32 words kajo_hip_noise returns for p in its mean and
   stderror planes ("The noise estimate" below: its evaluation in binary64, rounded to float32). p is MEASURED when se >= 0 (n >= 2) and
   m > 0; then
     r = se / m;   t = r * l(e_0(p));   v0(p) = t * t          three float32 operations, not contracted
   the relative error of the luminance carried over to the (demodulated) colour: exact where the albedo is grey, an approximation
   elsewhere (the estimate is of the luminance of the radiance, the filter's l of radiance / albedo per channel). If that v0 is not
   finite, p is not measured. A pixel that is not measured -- black in every batch (m = 0), fewer than two whole batches, a frame of
   fewer than 8 passes -- takes the 3x3 spatial variance above, by the plain filter's expressions in their order: a handle on which no
   pixel is measured gives the plain filter's output bit for bit. As se goes to 0 the luminance weight between pixels of different
   luminance goes to 0: a converged frame is left alone. The records always describe the ACCUMULATION, also where the frame being
   filtered is a despeckled, staged one (kajo_hip_present_argb8 and the chains behind it).
   Where m and se come from: (b) the planes of kajo_hip_denoise_guide_planes while they are of the handle's pass count, else (a) the
   handle's own records, evaluated on the device as kajo_hip_noise evaluates them -- a handle created with KAJO_FLAG_NOISE that owns the
   whole frame (tileCount == 1; an adaptive handle too: retired slots keep their records). The output does not depend on which of the
   two supplied the words. KAJO_E_STATE, from every entry point that takes `denoise`, where neither is at hand: the handle was created
   without the noise flag, the uploaded planes are for another pass count, or the handle holds the records of part of the frame only.
   With iterations == 0 the flag is ignored, as demodulation is. Flag bits other than 1 and 2 are ignored. */
#define KAJO_DENOISE_NO_DEMODULATE 1u /* filter the mean radiance itself instead of radiance / albedo */
#define KAJO_DENOISE_NOISE_GUIDED 2u  /* v0 from the measured per-pixel variance of KAJO_FLAG_NOISE where there is one (above) */
typedef struct KajoDenoiseParams {
    int32_t iterations;   /* K, 0..8 (default 5) */
    uint32_t flags;       /* KAJO_DENOISE_* (default 0) */
    float sigmaLuminance; /* default 4 */
    float sigmaNormal;    /* default 128 */
    float sigmaDepth;     /* default 1 (the quality sweep) */
    float reserved[3];    /* 0 */
} KajoDenoiseParams;
void kajo_hip_default_denoise_params(KajoDenoiseParams* p); /* NULL is accepted */
int kajo_hip_denoise(kajo_hip_t h, const KajoDenoiseParams* p, float* radiance, uint32_t* argb8);
/* The noise-guided filter's m and se for a handle that does not hold the whole frame's records: the root of several owners, which has the
   composed frame and the composed AOVs (KAJO_FLAG_AOV_TILED) but only its own tiles' records. mean, stderror: HOST pointers to
   WHOLE-FRAME row-major planes of width*height floats, as every owner's kajo_hip_noise fills them into the same arrays. They are copied
   into device memory (allocated on the first call, freed by kajo_hip_destroy) and stamped with the handle's current pass count; they
   take precedence over the handle's own records while that stamp equals the pass count, and are dropped by NULL, NULL, kajo_hip_reset
   and kajo_hip_set_pass_count. KAJO_E_INVALID, before the handle is looked at, for exactly one NULL plane; KAJO_E_INVALID for a NULL
   handle. Waits. */
int kajo_hip_denoise_guide_planes(kajo_hip_t h, const float* mean, const float* stderror);

/* Exposure, tone curves and automatic exposure in the image resolve: a post-process over the handle's whole frame, in kernels of its own
   (kajo_amd/csrc/tonemap.inc.hip) on the handle's stream, compiled into each numerics build so that the mean and the display transform are
   the resolve's own expressions (EXACT handles use the STRICT build's, as for the resolve). Definition -- P = the handle's pass count; per
   pixel:
     m = sum.rgb / P                  the build's division, as the resolve forms it (sum: the accumulation, or the denoised frame)
     the pixel COUNTS where all three channels of m are finite
     l(x) = 0.2126 x.r + 0.7152 x.g + 0.0722 x.b
     a = key / Lavg, Lavg = exp(mean of log(1e-4 + max(l(m), 0)) over the counting pixels of the whole frame), with
         KAJO_TONE_AUTO_EXPOSURE; 1 without the flag or where no pixel counts
     s = 2^exposure * a               (exactly 1 with exposure 0 and no automatic exposure)
     x = m * s, then y per curve:
       CLAMP     min(max(x, 0), 1) per channel (NaN gives 0)
       REINHARD  L = l(x), Ld = L (1 + L / white^2) / (1 + L), or L / (1 + L) with white = 0 (Reinhard et al. 2002, eq. 4, on
                 luminance); y = min(max(x Ld / L, 0), 1) where L > 0, else 0
       ACES      min(max(x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14), 0), 1) per channel (Narkowicz 2015, no pre-scale)
     a pixel that does not count is mapped by CLAMP under every curve (NaN / Inf as the resolve maps them)
     out = (int)(pow(y, 1 / 2.2) * 255 + .5) per channel with the build's pow, alpha 255 (the resolve's expression)
   The default parameters are the resolve bit for bit: kajo_hip_resolve_argb8, kajo_hip_resolve_gathered_argb8_device, and with denoise
   kajo_hip_denoise's argb8. The log-average is summed in float64 over fixed 64x16 rectangles of the image in image order and the
   rectangles' sums in a fixed order, with no atomics: image and scale are the same bits from run to run and for any number of tile owners.
   Refusals (KAJO_E_INVALID, before any device work): NULL params or handle; an unknown curve or flag bit; an exposure that is not finite
   or outside -32..32; a white point that is negative or not finite; with KAJO_TONE_AUTO_EXPOSURE a key that is not finite or not above
   0; non-zero reserved words. The accumulation, the AOV buffers, the pass count and the counters (kernelMs included) are not touched;
   scratch (the log-average's partial sums and the scale word) is allocated on first use and freed by kajo_hip_destroy. */
#define KAJO_TONE_CLAMP 0              /* the reference's: clamp to [0, 1] (the default) */
#define KAJO_TONE_REINHARD 1           /* Reinhard et al. 2002, eq. 4, on luminance, with a white point */
#define KAJO_TONE_ACES 2               /* Narkowicz 2015 fit of the ACES RRT + ODT, per channel, no pre-scale */
#define KAJO_TONE_AUTO_EXPOSURE 1u     /* KajoToneParams.flags */
typedef struct KajoToneParams {
    int32_t curve;     /* KAJO_TONE_* (default CLAMP) */
    uint32_t flags;    /* KAJO_TONE_* flags (default 0) */
    float exposure;    /* EV added, -32 .. 32: a linear factor 2^exposure (default 0) */
    float white;       /* REINHARD: the exposed luminance mapped to 1; 0 = none, i.e. L / (1 + L) (default 0) */
    float key;         /* AUTO_EXPOSURE: the grey the log-average luminance is mapped to, > 0 (default 0.18) */
    float reserved[3]; /* 0 */
} KajoToneParams;
void kajo_hip_default_tone_params(KajoToneParams* p); /* NULL is accepted */
/* The whole frame (tileCount 1, or a composed handle, as kajo_hip_resolve_argb8) tone-mapped. denoise == NULL maps the accumulation;
   otherwise the frame kajo_hip_denoise with those parameters produces, formed on the device by the denoiser's kernels (its refusals and
   KAJO_E_STATE rules apply). argb8: HOST pointer to width*height words (row 0 = top); *scale: the s applied; either may be NULL. Waits. */
int kajo_hip_tonemap_argb8(kajo_hip_t h, const KajoToneParams* p, const KajoDenoiseParams* denoise, uint32_t* argb8, float* scale);
/* The tone-mapped twin of kajo_hip_resolve_gathered_argb8_device (the same `gathered` buffers, NULL = the handle's own when tileCount == 1),
   into DEVICE memory, asynchronous on the handle's stream: the log-average reaches the mapping kernel through a device word, no host
   synchronisation. */
int kajo_hip_tonemap_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoToneParams* p, void* dst);
/* The s of the handle's most recent tone mapping; waits for it. KAJO_E_STATE before the first one. */
int kajo_hip_tone_scale(kajo_hip_t h, float* scale);

/* Glare (bloom): a small share of every pixel's energy spread over its neighbourhood, between the frame and the tone curves, so that
   a light far brighter than 1 gets a halo for the curve to roll off instead of a flat disc. A post-process over the handle's whole
   frame, in kernels of its own (kajo_amd/csrc/glare.hip) on the handle's stream, in float32 IEEE arithmetic without contraction in
   every numerics build: only its inputs depend on FAST / EXACT / STRICT. Frame in, frame out, in the units of kajo_hip_read_radiance,
   where the denoiser sits. Definition -- P = the handle's pass count, F = the source frame in sums over passes (the accumulation, or
   the frame kajo_hip_denoise gives), W x H, row 0 at the top; per pixel:
     m  = F.rgb / P                      (float32 division)
     the pixel COUNTS where all three channels of m are finite
     x  = max(m, 0);  l = 0.2126 x.r + 0.7152 x.g + 0.0722 x.b
     B0 = x * k,  k = 1 if threshold == 0 else max(l - threshold, 0) / max(l, 1e-6);   B0 = 0 where the pixel does not count
   reduce, level k -> k+1, size (w+1)/2 x (h+1)/2 (integer division):
     B_{k+1}(X, Y) = sum g_i g_j B_k(2X+i, 2Y+j) / sum g_i g_j,   i, j in {-1, 0, 1, 2},  g = [1, 3, 3, 1] / 8,
     over the taps that lie inside level k (no edge clamping: the weights are renormalised over the taps that remain)
   n = min(levels, the number of reductions after which the level is 1 x 1)
   expand, level k+1 -> k: up(U)(x, y) = per axis the tap at (x >> 1) with weight 3/4 and its neighbour
     (x >> 1) + (x & 1 ? +1 : -1) with weight 1/4; taps outside level k+1 are skipped and the weights renormalised
     U_n = B_n;   U_k = (B_k + (n - k) * up(U_{k+1})) / (n - k + 1)   for k = n-1 .. 1;   G = up(U_1)
     (G is the mean of the n reduced levels, each brought back to full size)
   out.rgb = (m + strength * (G - B0)) * P   where the pixel counts;   F.rgb unchanged where it does not;   out.w = F.w
   With threshold 0 this is a lerp between the frame and its wide blur; with a threshold it removes `strength` of the bright part and
   adds it back spread out: energy is kept either way, up to the renormalisation at the edges (which is what keeps a constant frame
   constant). With strength == 0, levels == 0 or n == 0 (a 1 x 1 frame) the output is F itself, so its ARGB8 is that of the plain
   resolve / tone mapping bit for bit. A NaN or Inf pixel contributes nothing to any level and comes out with the bits it went in
   with: glare never spreads such a pixel. Sums have a fixed order and there are no atomics: the same bits from run to run and for any
   number of tile owners. The accumulation, the AOV buffers, the pass count and the counters (kernelMs included) are not touched.
   Scratch (the pyramid, about 2 x 4/3 float4 frames, and the output frame) is allocated on first use and freed by kajo_hip_destroy.
   Refusals (KAJO_E_INVALID, before any device work and before the handle is looked at): levels outside 0..12; any flag bit; a strength
   that is not finite or outside 0..1; a threshold that is negative or not finite; non-zero reserved words. Then the tone and the denoise
   parameters' own refusals, then the handle's (KAJO_E_STATE with no pass rendered; the denoiser's state rules with `denoise`). */
typedef struct KajoGlareParams {
    int32_t levels;     /* 0..12 (default 6) */
    uint32_t flags;     /* 0: no flag defined yet; any bit is refused */
    float strength;     /* 0..1 (default 0.1) */
    float threshold;    /* >= 0, finite (default 0: every pixel glares in proportion) */
    float reserved[4];  /* 0 */
} KajoGlareParams;      /* 32 bytes */
void kajo_hip_default_glare_params(KajoGlareParams* p); /* NULL is accepted */
/* The frame after glare: radiance = HOST pointer to width*height*4 floats (row 0 = top), sums over passes. denoise == NULL: glare over
   the accumulation (tileCount 1, or a composed handle, as kajo_hip_read_radiance); otherwise over the frame kajo_hip_denoise with those
   parameters produces, formed on the device. g == NULL is refused (KAJO_E_INVALID). Waits. */
int kajo_hip_glare(kajo_hip_t h, const KajoGlareParams* g, const KajoDenoiseParams* denoise, float* radiance);
/* The display chain: denoise (optional, NULL = the accumulation) -> glare (optional, NULL = none) -> tone mapping, which takes the
   glared frame as it takes the denoised one: automatic exposure is measured on the frame after glare. With g == NULL exactly
   kajo_hip_tonemap_argb8. argb8: HOST pointer to width*height words; *scale: the s applied; either may be NULL. Waits. */
int kajo_hip_display_argb8(kajo_hip_t h, const KajoDenoiseParams* denoise, const KajoGlareParams* g, const KajoToneParams* tone,
                           uint32_t* argb8, float* scale);
/* The multi-GPU twin, as kajo_hip_tonemap_gathered_argb8_device is kajo_hip_tonemap_argb8's: gathered tile buffers (NULL = the handle's
   own when tileCount == 1) -> glare (NULL = none) -> tone mapping, into DEVICE memory, asynchronous on the handle's stream, no host
   synchronisation. */
int kajo_hip_display_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoGlareParams* g, const KajoToneParams* tone,
                                           void* dst);

/* Despeckle: repair the pixels that are not a number and bound the single-pixel outliers (fireflies), in front of the display chain.
   The integrator leaves both (the reference's own arithmetic produces NaN samples, Light.cpp:43-46; a firefly is one path that found
   the light through an unlikely chain); the resolve, the tone curves and the glare map a NaN pixel to a black dot, the glare spreads
   a firefly into a halo, and the denoiser lets it through into its neighbours. A post-process over the handle's whole frame, in
   kernels of its own (kajo_amd/csrc/despeckle.hip) on the handle's stream, in float32 IEEE arithmetic without contraction in every
   numerics build and in one fixed order: only its inputs depend on FAST / EXACT / STRICT. Frame in, frame out, in the units of
   kajo_hip_read_radiance. Definition -- P = the handle's pass count, F = the source frame in sums over passes, W x H, row 0 at the top;
   per pixel:
     m = F.rgb / P                       (float32 division)
     the pixel COUNTS where all three channels of m are finite
     l = (0.2126 max(m.r, 0) + 0.7152 max(m.g, 0)) + 0.0722 max(m.b, 0)
   Step 1, clamp (F -> C). N1(p) = the 8 neighbours of p that lie inside the image and count. Where p counts and |N1(p)| >= 3:
     L_(r) = the r-th largest l over N1(p), r = min(rank, |N1(p)|)
     b = factor * max(L_(r), floor)
     if l > b:  C.rgb = (m * (b / l)) * P      (the hue is kept: all three channels are scaled, negative ones included)
   Everywhere else C = F with the bits it had; C.w = F.w. factor == 0 switches the clamp off (C = F).
   Step 2, repair (C -> out). A pixel of C counts where C.rgb / P is finite (the clamp only scales a counting pixel down: these are
   the pixels of F that count). A pixel that counts: out = C. One that does not:
     out.rgb = (sum of C.rgb / P over the counting pixels of N1(p), in row-major order) / |N1(p)| * P
     where N1(p) is empty, the same mean over the counting pixels among the other 24 of the 5 x 5 window around p, in row-major order
     where that is empty too, out = F with the bits it had;   out.w = F.w
   Repair reads the CLAMPED frame, so a firefly beside a NaN pixel is not averaged in at its full height. The counts: pixels clamped
   (C differs from F by the rule above) and pixels repaired (given a mean; a pixel left with its input bits is not counted).
   Properties. A constant frame is unchanged. A k x k block of equal bright pixels, k >= 2, is unchanged at rank 1..3 (every pixel
   of it has three neighbours as bright): lights keep their discs. A light that covers one pixel -- at rank 2 and above, one or two
   -- IS dimmed, to `factor` times its surroundings: the rule cannot tell it from a firefly. The defaults (16, 1, 0.2) are the
   gentlest setting of DESIGN.md section 6f's sweep that still bounds a pixel far above everything around it: at low sample counts
   most pixels several times their neighbours are signal, which the denoiser needs. The output at a pixel depends on the input
   frame only, through image coordinates: no atomics, no order between workgroups, so the frame and the counts are the same bits
   for any number of tile owners, on a second call and on a twin handle. The clamp is biased (it removes energy) and is a display
   decision: kajo_hip_read_radiance and every other existing entry point stay as they are. The accumulation, the AOV buffers, the
   pass count and the counters (kernelMs included) are not touched. Scratch (two float4 frames, one word per workgroup and pass,
   the two counts) is allocated on first use and freed by kajo_hip_destroy.
   Refusals (KAJO_E_INVALID, before any device work and before the handle is looked at): NULL params; a factor that is not finite,
   negative or inside (0, 1); a rank outside 1..4; a floor that is negative or not finite; any flag bit; non-zero reserved words. */
typedef struct KajoDespeckleParams {
    float factor;       /* 0 (no clamp, repair only) or >= 1, finite (default 16) */
    int32_t rank;       /* 1..4 (default 1): the neighbour a pixel is measured against, the rank-th brightest */
    float floor;        /* >= 0, finite (default 0.2): the least luminance the bound is formed from, so that a dim pixel on black stays */
    uint32_t flags;     /* 0: no flag defined yet; any bit is refused */
    float reserved[4];  /* 0 */
} KajoDespeckleParams;  /* 32 bytes */
void kajo_hip_default_despeckle_params(KajoDespeckleParams* p); /* NULL is accepted */
/* The frame after the stage: radiance = HOST pointer to width*height*4 floats (row 0 = top), sums over passes; counts[0] = pixels
   clamped, counts[1] = pixels repaired; either may be NULL. Valid where kajo_hip_read_radiance is (tileCount 1, or a composed handle);
   KAJO_E_STATE with no pass rendered. Waits. */
int kajo_hip_despeckle(kajo_hip_t h, const KajoDespeckleParams* p, float* radiance, int64_t counts[2]);
/* The display chain with the stage in front: despeckle -> denoise -> glare -> tone mapping, every stage but the last optional (NULL).
   With despeckle == NULL exactly kajo_hip_display_argb8's calls. Otherwise the denoiser filters the despeckled frame as if it were
   the accumulation (the stage writes it in the handle's tile layout; no kernel of the denoiser changes), and automatic exposure is
   measured at the end of the chain, as before. Refusals in the order despeckle, glare, tone, denoise, handle. Waits. */
int kajo_hip_present_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                           const KajoToneParams* tone, uint32_t* argb8, float* scale);
/* The multi-GPU twin, as kajo_hip_display_gathered_argb8_device is kajo_hip_display_argb8's: gathered tile buffers (NULL = the handle's
   own when tileCount == 1) -> despeckle (NULL = none) -> glare (NULL = none) -> tone mapping, into DEVICE memory, asynchronous on the
   handle's stream, no host synchronisation: the counts stay on the device. The stage needs no AOVs, so it serves any number of owners. */
int kajo_hip_present_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                           const KajoToneParams* tone, void* dst);
/* The two counts of the handle's most recent despeckle; waits for it. KAJO_E_STATE before the first one. */
int kajo_hip_despeckle_counts(kajo_hip_t h, int64_t counts[2]);

/* Histogram metering: percentile automatic exposure and automatic white point. The log-average of KAJO_TONE_AUTO_EXPOSURE is one number
   that unlit background drags down and a light drags up; a luminance histogram gives the exposure that puts a chosen PERCENTILE of the
   lit pixels at the key, the luminance below which a chosen share of them lies (Reinhard's white), and the range the frame spans. A
   measurement at the end of the display chain, over the frame the tone kernels are handed, in kernels of its own
   (kajo_amd/csrc/meter.hip) on the handle's stream, in float32 IEEE arithmetic without contraction in every numerics build: only its
   inputs depend on FAST / EXACT / STRICT. Definition -- P = the handle's pass count, F = the source frame in sums over passes (after
   whichever of despeckle, denoise and glare are asked for), W x H; per pixel:
     m = F.rgb / P                       (float32 division)
     the pixel COUNTS where all three channels of m are finite
     l = (0.2126 max(m.r, 0) + 0.7152 max(m.g, 0)) + 0.0722 max(m.b, 0)      (despeckle's expression and order)
     u = bits(l) & 0x7fffffff            (max(-0, 0) may leave -0: the sign is masked)
     k = u >> 19                         (the exponent and four bits of the mantissa: 16 bins per stop, linear inside a sixteenth
                                          of a stop; no logarithm is taken)
     base = (127 - 16) << 4
     bin = 0 if k < base (l < 2^-16, zero and denormals included), else min(k - base + 1, 513)
   Bins 1..512 cover 2^-16 .. 2^16; bin 513 is everything from 2^16 up, +Inf included (an l of finite channels can overflow). The lower
   edge of inner bin b is the float with the bits (b - 1 + base) << 19, its centre the mean of its edge and the next (exact in float32);
   the centre of bin 513 is 2^16. The counts are uint32 and exact: integer addition commutes, so the histogram is the same words from
   run to run, for any number of workgroups and for any number of tile owners, with no float sum to order.
     nonfinite = the pixels that do not count       under = bin 0        over = bin 513
     metered n = the sum of bins 1..513 (black does not meter);   nonfinite + the sum of all bins = W * H
   Evaluation, on the host in binary64, pure (kajo_hip_meter_evaluate):
     value(q), q in (0, 1]: rank r = min(n, max(1, ceil((double)q * n))); the bin is the smallest b >= 1 whose cumulative count over
                            bins 1..b reaches r; the value is that bin's centre
     anchorL = value(percentile);  exposure = log2(key / anchorL);  whiteL = value(whitePercentile)
     minBin, maxBin = the first and the last non-empty bin among 1..513
     with n = 0: anchorL 0, exposure 0, whiteL 0, minBin = maxBin = 0
   Refusals (KAJO_E_INVALID, before any device work and before the handle is looked at): NULL params; a percentile or whitePercentile
   that is not finite or outside (0, 1]; a key that is not finite or not above 0; an unknown flag bit; non-zero reserved words. Where
   other stages' parameters are present too, the order is despeckle, glare, meter, tone, denoise, handle. The accumulation, the AOV
   buffers, the matte buffers, the pass count and the counters (kernelMs included) are not touched; scratch (the workgroups' partial
   histograms, under 1 MB at any frame size, and the 514 + 1 words of the result) is allocated on first use and freed by
   kajo_hip_destroy. */
#define KAJO_METER_BINS 514
#define KAJO_METER_AUTO_WHITE 1u       /* KajoMeterParams.flags: kajo_hip_meter_tone also sets Reinhard's white from whiteL */
typedef struct KajoMeterParams {
    float percentile;       /* in (0, 1] (default 0.5: the median of the metered pixels) */
    float key;              /* > 0, finite (default 0.18): the grey the anchor luminance is mapped to */
    float whitePercentile;  /* in (0, 1] (default 0.995) */
    uint32_t flags;         /* KAJO_METER_* (default 0) */
    float reserved[4];      /* 0 */
} KajoMeterParams;          /* 32 bytes */
typedef struct KajoMeterResult {
    int64_t pixels;         /* W * H */
    int64_t nonfinite;      /* pixels that do not count */
    int64_t under;          /* bin 0: below 2^-16, black included */
    int64_t over;           /* bin 513: 2^16 and above */
    int64_t metered;        /* n: the sum of bins 1..513 */
    float anchorL;          /* the luminance at `percentile` */
    float whiteL;           /* the luminance at `whitePercentile` */
    float exposure;         /* log2(key / anchorL), in stops */
    int32_t minBin, maxBin; /* the frame spans (maxBin - minBin + 1) / 16 stops */
    int32_t reserved;       /* 0 */
} KajoMeterResult;          /* 64 bytes */
void kajo_hip_default_meter_params(KajoMeterParams* p); /* NULL is accepted */
/* Pure host, no device and no handle: the fields of *result from a histogram, except pixels and nonfinite, which are left as the
   caller set them. KAJO_E_INVALID: NULL hist or result, or the params' refusals above. */
int kajo_hip_meter_evaluate(const uint32_t hist[KAJO_METER_BINS], const KajoMeterParams* p, KajoMeterResult* result);
/* Pure host: the tone parameters a metered frame is mapped with. *out = *in with exposure = min(max(in.exposure + result.exposure,
   -32), 32) -- the caller's EV is a compensation on top of the metered one, as on a camera -- and, with KAJO_METER_AUTO_WHITE, white =
   whiteL * 2^out.exposure (white is in exposed units; a whiteL of 0 gives 0, i.e. no white point). KAJO_E_INVALID: a NULL argument,
   the params' refusals, or `in` with KAJO_TONE_AUTO_EXPOSURE: that would be two automatic exposures. in and out may be one struct. */
int kajo_hip_meter_tone(const KajoMeterResult* result, const KajoMeterParams* p, const KajoToneParams* in, KajoToneParams* out);
/* Measures the frame kajo_hip_present_argb8 with the same first three stages would hand the tone kernels (NULL = the stage is off; with
   all three NULL the accumulation). hist: HOST pointer to KAJO_METER_BINS words; either of hist and result may be NULL. Valid where
   kajo_hip_read_radiance is (tileCount 1, or a composed handle); KAJO_E_STATE with no pass rendered. Waits. */
int kajo_hip_meter(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                   const KajoMeterParams* meter, uint32_t* hist, KajoMeterResult* result);
/* kajo_hip_present_argb8 with the metering between the chain and the tone curves: the chain is formed once, its last frame is metered,
   the 2 KB histogram is read back and evaluated, kajo_hip_meter_tone patches `tone`, and the tone kernels map that same frame with the
   patched parameters. *result (may be NULL): the measurement. With meter == NULL exactly kajo_hip_present_argb8 (result is not
   written). Refusals in the order despeckle, glare, meter, tone (KAJO_TONE_AUTO_EXPOSURE among them), denoise, handle. Waits. */
int kajo_hip_present_metered_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                                   const KajoMeterParams* meter, const KajoToneParams* tone, uint32_t* argb8, KajoMeterResult* result);
/* The multi-GPU twin over gathered tile buffers (NULL = the handle's own when tileCount == 1), into DEVICE memory. This one call is NOT
   asynchronous end to end: it waits once, for the histogram, then enqueues the tone mapping on the handle's stream and returns. The
   tone kernels take exposure and white BY VALUE from the host, and they are not to change for this: the metered scale has to reach
   the host before they can be launched. With meter == NULL exactly kajo_hip_present_gathered_argb8_device, asynchronous as before. */
int kajo_hip_present_metered_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle,
                                                   const KajoGlareParams* g, const KajoMeterParams* meter, const KajoToneParams* tone, void* dst,
                                                   KajoMeterResult* result);

/* Local tone mapping: an edge-aware base / detail range compression. Every other stage that maps radiance to the display is global:
   one exposure and one curve for the whole frame, so a light of emission 445 in a room whose corners sit near 2^-8 either burns out
   or flattens the floor. This stage compresses the range locally: it splits log luminance into a base layer (an edge-avoiding A-trous
   filter, Dammertz et al. 2010, used as Durand & Dorsey 2002 use the bilateral) and a detail layer, shrinks the base layer's distance
   from a pivot and keeps the detail. A post-process over the handle's whole frame, between the glare and the meter, in kernels of its
   own (kajo_amd/csrc/local.hip) on the handle's stream, in float32 IEEE arithmetic without contraction in every numerics build and in
   one fixed order: only its inputs depend on FAST / EXACT / STRICT. Frame in, frame out, in the units of kajo_hip_read_radiance.
   Definition -- P = the handle's pass count, F = the source frame in sums over passes (after whichever of despeckle, denoise and glare
   are asked for), W x H, row 0 at the top; per pixel:
     m = F.rgb / P                        (float32 division)
     the pixel COUNTS where all three channels of m are finite
     l = (0.2126 max(m.r, 0) + 0.7152 max(m.g, 0)) + 0.0722 max(m.b, 0)      (despeckle's / the meter's expression and order)
     L = log2(min(max(l, 2^-16), 2^16))   (the meter's range; zero, denormals and an overflowed l are clamped, not dropped)
   B_0 = L. Iteration i = 0 .. K-1, step d = 2^i, taps q = p + d (dx, dy), dx, dy in -2..2, h = [1/16, 1/4, 3/8, 1/4, 1/16]:
     w   = (h[dx] h[dy]) w_r,   t = (B_i(p) - B_i(q)) / sigmaRange,   w_r = exp2(-(t t)),  exactly 1 at the centre tap
     B_{i+1}(p) = sum(w B_i(q)) / sum(w)  over the taps inside the image that count, both sums in row-major tap order (dy outer, dx
                  inner); no edge clamping, the weights are renormalised over the taps that remain (the centre tap always remains
                  for a counting p, so sum(w) >= 9/64)
   then
     L' = (pivot + compression (B_K - pivot)) + detail (L - B_K)
     g  = exp2(L' - L)
     out.rgb = (m g) P  where the pixel counts;   F.rgb with the bits it had where it does not;   out.w = F.w
   A pixel that does not count is never a tap and comes out with the bits it went in with: the stage never spreads a NaN or Inf. With
   compression == 1 and detail == 1 the output is F itself and the stage does no device work (as glare does none at strength 0), so
   every ARGB8 is then the existing call's bit for bit. K = 0 gives B = L: a pure power curve on luminance about the pivot, with no
   neighbourhood. No atomics and no order between workgroups: the output at a pixel depends on the input frame only, through image
   coordinates, so the frame is the same bits for any number of tile owners, on a second call and on a twin handle. The accumulation,
   the AOV buffers, the matte tables, the pass count and the counters (kernelMs included) are not touched. Scratch (three float planes
   -- L and the two of the ping-pong -- and the output frame) is allocated on first use and freed by kajo_hip_destroy.
   The pivot is a log2 luminance. With KAJO_LOCAL_PIVOT_METERED the stage takes the meter's histogram (kajo_hip_meter's kernels and
   definition) of its own input frame, reads it back and uses pivot = log2(value(pivotPercentile)), value(q) as
   kajo_hip_meter_evaluate defines it, formed on the host in binary64 and rounded to float; with no metered pixel it falls back to the
   `pivot` field. The range is then compressed about the frame's own median instead of a guess.
   Refusals (KAJO_E_INVALID, before any device work and before the handle is looked at): NULL params; iterations outside 0..8; an
   unknown flag bit; a compression that is not finite or outside (0, 1]; a detail that is not finite or outside 0..4; a sigmaRange that
   is not finite or not above 0; a pivot that is not finite or outside -16..16; a pivotPercentile that is not finite or outside
   (0, 1] (checked with or without the flag); a non-zero reserved word. Where other stages' parameters are present too, the order
   is despeckle, glare, local, meter, tone, denoise, handle; then the handle's own state rules (KAJO_E_STATE with no pass rendered,
   the denoiser's rules with `denoise`). */
#define KAJO_LOCAL_PIVOT_METERED 1u    /* KajoLocalParams.flags: the pivot is the frame's own pivotPercentile-th luminance */
typedef struct KajoLocalParams {
    int32_t iterations;     /* K, 0..8 (default 5) */
    uint32_t flags;         /* KAJO_LOCAL_* (default 0) */
    float compression;      /* (0, 1], finite (default 0.6): the factor on the base layer's distance from the pivot, in stops */
    float detail;           /* 0..4, finite (default 1): the factor on the detail layer */
    float sigmaRange;       /* > 0, finite, in stops (default 2) */
    float pivot;            /* finite, -16..16 (default log2(0.18)) */
    float pivotPercentile;  /* (0, 1] (default 0.5); read only with PIVOT_METERED */
    float reserved;         /* 0 */
} KajoLocalParams;          /* 32 bytes */
void kajo_hip_default_local_params(KajoLocalParams* p); /* NULL is accepted */
/* The frame after the stage: radiance = HOST pointer to width*height*4 floats (row 0 = top), sums over passes; may be NULL. The frame
   kajo_hip_present_argb8 with the same first three stages would hand the tone kernels (NULL = the stage is off; with all three NULL
   the accumulation), then this stage. local == NULL is refused (KAJO_E_INVALID). Valid where kajo_hip_read_radiance is (tileCount 1,
   or a composed handle). Waits. */
int kajo_hip_local(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                   const KajoLocalParams* local, float* radiance);
/* kajo_hip_present_metered_argb8 with the stage between the glare and the meter: despeckle -> denoise -> glare -> local -> meter ->
   tone mapping, every stage but the last optional (NULL). The meter of the chain measures the frame AFTER the stage, so it still
   sees what the tone kernels are handed; *result (may be NULL) is that measurement, written only with meter != NULL. With local ==
   NULL exactly kajo_hip_present_metered_argb8: the stage is not run. Waits. */
int kajo_hip_present_local_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGlareParams* g,
                                 const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone, uint32_t* argb8,
                                 KajoMeterResult* result);
/* The multi-GPU twin over gathered tile buffers (NULL = the handle's own when tileCount == 1), into DEVICE memory; the stage needs no
   AOVs, so it serves any number of owners. Asynchronous on the handle's stream, except that it waits once for the histogram with
   KAJO_LOCAL_PIVOT_METERED, and once more with `meter`, as kajo_hip_present_metered_gathered_argb8_device already does. With local ==
   NULL exactly that call. */
int kajo_hip_present_local_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                                 const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone, void* dst,
                                                 KajoMeterResult* result);
/* The pivot of the handle's most recent run of the stage (the `pivot` field, or the metered one). KAJO_E_STATE before the first one; a
   call in which the stage did no device work (compression == 1 and detail == 1) is not a run. */
int kajo_hip_local_pivot(kajo_hip_t h, float* pivot);

/* Depth of field: a lens blur from the depth AOV, between the denoiser and the glare. Every image of the chain is otherwise taken
   through a pinhole. This stage blurs each pixel by the circle of confusion (CoC) a thin lens focused at focusDistance gives its depth.
   It is an IMAGE-SPACE APPROXIMATION: one depth per pixel -- the depth AOV, B.w / A.w, the mean hit distance over the beauty render's
   own camera samples, with KAJO_FLAG_AOV_SPECULAR the length of the whole chain, so what is seen in a mirror or through glass is
   defocused by its optical distance -- and nothing behind a foreground object can be revealed. A post-process over the handle's whole
   frame in kernels of its own (kajo_amd/csrc/lens.hip) on the handle's stream, in float32 IEEE arithmetic without contraction in every
   numerics build and in one fixed order: only its inputs depend on FAST / EXACT / STRICT. Frame in, frame out, in the units of
   kajo_hip_read_radiance. It comes after the denoiser (whose guides are pinhole-aligned) and before the glare (which models scattering
   behind the lens).
   Definition -- P = the handle's pass count, F = the source frame in sums over passes (after whichever of despeckle and denoise are
   asked for), A and B the whole-frame AOV buffers of kajo_hip_read_aov, W x H, row 0 at the top, Hf = (float)H; per pixel p:
     m = F.rgb / P                          the pixel COUNTS where all three channels are finite
     z = B.w / A.w  where A.w > 0 and the quotient is finite and > 0;  +inf otherwise  (a miss, or a poisoned depth: "far")
     u = |1 - focusDistance / z|            (u = 1 for z = +inf)
     r = min((aperture * Hf) * u, (float)maxRadius)      the CoC's radius in pixels (fminf: a NaN product gives maxRadius)
   the thin lens's CoC with its constants folded into `aperture`: the radius at infinite depth as a fraction of the frame's height, so
   the same parameters give the same picture at any resolution. Taps q = p + (dx, dy), |dx|, |dy| <= maxRadius; only taps inside the
   image that count are used; d = sqrtf((float)(dx*dx + dy*dy)):
     re = r_q               where z_q <= z_p   (q is in front of p or level with it: its disc lies over p)
          min(r_q, r_p)     otherwise          (q is behind p: it cannot bleed over a sharper foreground)
     c  = min(max((re + 1) - d, 0), 1)         a disc with a one-pixel soft edge; exactly 1 at the centre tap
     w  = c / (1 + pi_f * (re * (re + 1)))     pi_f = (float)M_PI; the divisor approximates the lattice sum of c (ratio 1.000 at r = 0,
                                               0.996 .. 1.026 for r up to 16)
     sumW += w;  sum.rgb += w * m_q            row-major tap order (dy outer, dx inner), accumulators start at +0, no FMA
     out.rgb = (sum.rgb / sumW) * P  where p counts;   F.rgb with the bits it had where it does not;   out.w = F.w
   What follows from it: the centre tap always has w > 0 for a counting p, so sumW > 0. A pixel that does not count is never a tap: the
   stage spreads no NaN and repairs none (that is the despeckle's job). A tap with c == 0 adds +-0 to sums that start at +0, so any
   culling that skips only such taps and keeps the order of the rest gives the same bits (the kernel's per-workgroup window bound). With
   aperture == 0 the output is F itself and the stage does no device work (as the glare at strength 0), so every image is then the
   existing call's bit for bit. A frame whose every r is 0 comes out as (F.rgb / P) * P. A constant frame stays constant within
   rounding under any depth field. No atomics and no order between workgroups: the output at a pixel depends on the inputs through image
   coordinates only, so the frame is the same bits on a second call, on a twin handle and on the root of any number of tile owners. The
   accumulation, the AOV buffers, the matte tables, the pass count and the counters (kernelMs included) are not touched. Scratch (the
   planes r and z, the tap records and the output frame) is allocated on first use and freed by kajo_hip_destroy.
   Refusals (KAJO_E_INVALID, before any device work and before the handle is looked at): NULL params; an aperture that is not finite or
   outside 0..1; a focusDistance that is not finite or not above 0; a maxRadius outside 1..KAJO_LENS_MAX_RADIUS; a flag bit; a non-zero
   reserved word. Where other stages' parameters are present too, the order is despeckle, lens, glare, local, meter, tone, denoise,
   handle. Then the handle's state, by the denoiser's rules: KAJO_E_STATE on a handle without KAJO_FLAG_AOV, with no pass rendered, on
   a tiled handle (KAJO_FLAG_AOV_TILED) before kajo_hip_compose_aov or after a later render or reset, and on an owner of part of the
   frame without a composed frame. There is no gathered *_device twin: the stage needs whole-frame AOVs, as the denoiser does; several
   owners are served through the root after kajo_hip_compose and kajo_hip_compose_aov. */
#define KAJO_LENS_MAX_RADIUS 16
typedef struct KajoLensParams {
    float aperture;       /* >= 0, finite, <= 1 (default 0.01) */
    float focusDistance;  /* > 0, finite, in the depth AOV's units (default 10) */
    int32_t maxRadius;    /* 1..KAJO_LENS_MAX_RADIUS (default 16) */
    uint32_t flags;       /* 0: an unknown bit is refused */
    float reserved[4];    /* 0 */
} KajoLensParams;         /* 32 bytes */
void kajo_hip_default_lens_params(KajoLensParams* p); /* NULL is accepted */
/* The frame after the stage: radiance = HOST pointer to width*height*4 floats (row 0 = top), sums over passes; may be NULL. The frame
   kajo_hip_present_argb8 with the same first two stages would hand the glare (NULL = the stage is off; with both NULL the
   accumulation), then this stage. lens == NULL is refused (KAJO_E_INVALID). Waits. */
int kajo_hip_lens(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                  float* radiance);
/* The stage's decisions: the planes r (radius) and z (depth) of the definition, HOST pointers to width*height floats each (row 0 =
   top); either may be NULL. z = +inf is reported as +inf. They do not depend on the frame. What a test holds bit for bit, and the data
   behind a focus-peaking overlay. Waits. */
int kajo_hip_lens_coc(kajo_hip_t h, const KajoLensParams* lens, float* radius, float* depth);
/* The definition's z at one pixel: autofocus on what is under the cursor. +inf means "far". KAJO_E_INVALID outside the frame (after
   the NULL checks, before the handle's state). With focusDistance set to it, r at that pixel is exactly 0. Waits. */
int kajo_hip_lens_depth_at(kajo_hip_t h, int x, int y, float* z);
/* kajo_hip_present_local_argb8 with the stage between the denoiser and the glare: despeckle -> denoise -> lens -> glare -> local ->
   meter -> tone mapping, every stage but the last optional (NULL). With lens == NULL exactly kajo_hip_present_local_argb8: the stage is
   not run and the handle needs no AOVs. *result as there. Waits. */
int kajo_hip_present_lens_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                                const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                uint32_t* argb8, KajoMeterResult* result);

/* The view: crop, zoom and supersampled output, the last stage of the display chain. Every other stage works on scene-linear radiance
   at the handle's W x H; this one sits BEHIND the tone curves: ARGB8 in, ARGB8 out, a separable resampling in linear light. Averaging
   K x K display-referred pixels is what antialiases an edge whose radiance clips under every curve (render K times the size, tone map,
   view down); a source rectangle and an output size give thumbnails, window-sized read-backs and a zoom. Kernels of its own
   (kajo_amd/csrc/view.hip) on the handle's stream, float32 IEEE arithmetic without contraction in every numerics build and in one fixed
   order; the weights and the two transfer tables are formed on the host in binary64, the device only multiplies and adds: a float32
   restatement with the library's own weights and tables gives the same words (tests/view_replay.py).
   Definition -- src = a W x H image of 0xAARRGGBB words, row 0 at the top (what the tone kernels write); the output is outW x outH words,
   alpha 255. The source rectangle [x0, x1) x [y0, y1) is in source pixel units, pixel j spans [j, j + 1); all four edges zero = the whole
   frame. Per axis (the horizontal one; the vertical is the same with y0, y1, outH, H), in binary64 on the host (kajo_hip_view_weights):
     s = (x1 - x0) / outW          source pixels per output pixel;  S = max(s, 1)  the filter's stretch
     u = x0 + (i + 0.5) s          the centre of output pixel i;  t_j = (j + 0.5 - u) / S
     KAJO_VIEW_NEAREST    the one pixel floor(u) (held inside the image), weight 1
     KAJO_VIEW_AREA       w_j = the length of the overlap of [j, j + 1) with the footprint [x0 + i s, x0 + (i + 1) s): the exact area
                          average; an integer ratio K gives K equal weights; when magnifying at most two pixels
     KAJO_VIEW_TRIANGLE   w_j = max(1 - |t_j|, 0)
     KAJO_VIEW_LANCZOS3   w_j = sinc(t_j) sinc(t_j / 3) for |t_j| < 3, 0 otherwise;  sinc(0) = 1, sinc(t) = 0 EXACTLY at every other
                          integer t, sin(pi t) / (pi t) elsewhere (so that an unscaled view is one weight of 1 under this filter too)
   Taps outside 0 .. W - 1 are dropped, not clamped; the rest are divided by their binary64 sum ("renormalised over the taps inside",
   as everywhere in the chain) and rounded to float32. A row of weights is the contiguous run first .. first + count - 1; leading and
   trailing weights that are 0 in float32 are trimmed, never to nothing (a row whose sum is not positive becomes the NEAREST row).
   count <= KAJO_VIEW_MAX_TAPS = 2 * 3 * KAJO_VIEW_MAX_SCALE = 384: LANCZOS3's support is |t| < 3, i.e. the open interval of 6 S <= 384
   source pixels around u, which holds at most 384 pixel centres (AREA needs at most 65, TRIANGLE 128); a longer row, were rounding
   ever to produce one, is refused (KAJO_E_INVALID), not replaced.
   Transfer tables, binary64 rounded to float32 (kajo_hip_view_tables): lin[c] = (c / 255)^2.2, c = 0 .. 255; thresholds
   t[k] = ((k - 0.5) / 255)^2.2, k = 1 .. 255; encode(v) = the number of k with v >= t[k] -- the quantiser of renderer/Image.cpp:14-27
   (pow(1 / 2.2), then int(255 v + .5)) read backwards: no device pow, it clamps below 0 and above 1 by itself, and it is the same in
   FAST, EXACT and STRICT. t[c] < lin[c] < t[c + 1] with room of many float32 ulps, so a constant image comes back constant.
   The resampling, float32, no FMA, accumulators start at +0:
     T[y][i].c = sum over the taps j = first_x[i] .. in increasing j of wx[i][j] * lin[src[y][j].c]      c = r, g, b
     v.c       = sum over the taps y = first_y[o] .. in increasing y of wy[o][y] * T[y][i].c
     out[o][i] = 255 << 24 | encode(v.r) << 16 | encode(v.g) << 8 | encode(v.b)
   The source's alpha is not read. No division on the device, no atomics and no order between workgroups: an output word depends on the
   inputs through image coordinates only, so it is the same on a second call, a twin handle and the root of any number of tile owners.
   THE COPY CASE: outW == W, outH == H and the whole rectangle, under any filter, launches nothing and returns the source words as they
   are (alpha included); under the definition it is the identity too (one weight of 1.0 per axis, encode(lin[c]) == c).
   Refusals (KAJO_E_INVALID, before any device work). Without the handle, in this order: NULL params; an edge that is not finite; unless
   all four edges are zero, not 0 <= x0 < x1 or not 0 <= y0 < y1; outW or outH outside 1..KAJO_VIEW_MAX_OUT; with an explicit rectangle
   a minification (x1 - x0) / outW or (y1 - y0) / outH above KAJO_VIEW_MAX_SCALE; an unknown filter; a flag bit. Where other stages'
   parameters are present, the order is despeckle, lens, glare, local, meter, tone, view, denoise, handle. The checks against the frame
   NEED THE HANDLE and come last, after the denoiser's and the null handle: x1 > W or y1 > H, and the whole frame's minification W / outW
   or H / outH above KAJO_VIEW_MAX_SCALE. The accumulation, the AOVs, the pass count and the counters (kernelMs included) are not
   touched. Scratch (the intermediate T, the weight rows, the tables, an ARGB8 frame for the chain's image and one for the output) is
   allocated on first use, grown when a larger view asks, and freed by kajo_hip_destroy; the weight rows are formed and uploaded (from
   pinned staging, on the handle's stream) only when the parameters differ from the last call's. */
#define KAJO_VIEW_MAX_SCALE 64
#define KAJO_VIEW_MAX_TAPS 384
#define KAJO_VIEW_MAX_OUT 16384
enum { KAJO_VIEW_NEAREST = 0, KAJO_VIEW_AREA = 1, KAJO_VIEW_TRIANGLE = 2, KAJO_VIEW_LANCZOS3 = 3 };
typedef struct KajoViewParams {
    float x0, y0, x1, y1; /* the source rectangle in source pixel units; all zero = the whole frame (default) */
    int32_t outW, outH;   /* 1..KAJO_VIEW_MAX_OUT; the default 0 is refused: the caller names the size */
    uint32_t filter;      /* KAJO_VIEW_* (default KAJO_VIEW_AREA) */
    uint32_t flags;       /* 0: an unknown bit is refused */
} KajoViewParams;         /* 32 bytes */
void kajo_hip_default_view_params(KajoViewParams* p); /* NULL is accepted */
/* The weight rows of one axis: srcN source pixels, the rectangle's edges a0 < a1 on this axis, outN output pixels. Pure host code in
   binary64, no device and no handle. first and count take outN words each; weights takes outN rows of `stride` floats, stride = the
   largest count of the axis, row i at weights + i * stride, zeros behind its count. Returns outN * stride, the number of floats, or a
   negative KAJO_E_INVALID (srcN < 1, outN outside 1..KAJO_VIEW_MAX_OUT, not 0 <= a0 < a1 <= srcN or not finite, a scale above
   KAJO_VIEW_MAX_SCALE, an unknown filter, a capacity below the number of floats). With first, count and weights all NULL it only
   reports the size, as kajo_hip_launch_order does. */
int kajo_hip_view_weights(int32_t srcN, double a0, double a1, int32_t outN, uint32_t filter, int32_t* first, int32_t* count, float* weights,
                          size_t capacity);
/* The two transfer tables of the definition; either may be NULL. Pure host code. */
void kajo_hip_view_tables(float lin[256], float thresholds[255]);
/* The stage over a caller's image: src = HOST pointer to width*height words, dst = HOST pointer to outW*outH words, on the handle's
   device and stream. Needs no pass rendered and touches nothing of the handle but the stage's scratch. Waits. */
int kajo_hip_view_argb8(kajo_hip_t h, const KajoViewParams* view, const uint32_t* src, uint32_t* dst);
/* kajo_hip_present_lens_argb8 into the stage's scratch, then the stage: despeckle -> denoise -> lens -> glare -> local -> meter -> tone
   mapping -> view. argb8 = HOST pointer to outW*outH words (may be NULL). With view == NULL exactly kajo_hip_present_lens_argb8 (argb8
   then holds width*height words). *result as there. Waits. */
int kajo_hip_present_view_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoLensParams* lens,
                                const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                const KajoViewParams* view, uint32_t* argb8, KajoMeterResult* result);
/* The twin of kajo_hip_present_local_gathered_argb8_device with the stage behind it: dst = DEVICE pointer to outW*outH words. The chain's
   image goes into the stage's scratch, the stage writes dst. Asynchronous wherever that call is (it waits only where the chain in front
   does: KAJO_LOCAL_PIVOT_METERED and the meter) ONCE ITS SCRATCH STANDS: the first call with a view allocates, and a later view that
   needs a larger block of rows or a larger intermediate frees the smaller one, which waits for the device as every free does; a call
   whose parameters are the last call's, or need no more than an earlier call's, allocates nothing. A change of view parameters may
   also wait for the previous upload of weight rows to leave the staging block, never for a kernel. With view == NULL exactly that
   call. `result` is not in the view's own list of arguments: it mirrors kajo_hip_present_local_gathered_argb8_device, whose
   measurement would otherwise be lost (*result as there; may be NULL without a meter). */
int kajo_hip_present_view_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGlareParams* g,
                                                const KajoLocalParams* local, const KajoMeterParams* meter, const KajoToneParams* tone,
                                                const KajoViewParams* view, void* dst, KajoMeterResult* result);

/* The grade: white balance, an ASC CDL op over the frame, and per-object regrades by matte. Every other stage of the chain decides how
   bright a pixel is or where it lands; this one changes its colour, and it is what the coverage mattes are for: "regrade one ball or
   dim the lights" without rendering again. Frame in, frame out, in scene-linear radiance (the units of kajo_hip_read_radiance), between
   the denoiser and the lens: a regraded ball is then defocused, haloed and metered with its new colour, and a dimmed light throws a
   dimmer glare. Kernels of its own (kajo_amd/csrc/grade.hip) on the handle's stream; the arithmetic is kajo_amd/csrc/grade_math.h,
   compiled for the device and for kajo_hip_grade_pixels from the same lines, float32 IEEE without contraction in every numerics build
   and in the order written: only the stage's inputs depend on FAST / EXACT / STRICT.
   Definition -- P = the handle's pass count, F = the source frame in sums over passes (after whichever of despeckle and denoise are
   asked for); per pixel:
     m      = F.rgb / P                         the pixel COUNTS where all three are finite; otherwise out = F with the bits it had
     op(v):   t.c = max(v.c * slope.c + offset.c, 0)      one product, one sum; fmaxf, with +0 for -0 (and for a NaN)
              t.c = kajo_powf(t.c, power.c)               only where power.c != 1 (include/kajo_strictmath.h)
              l   = (0.2126f * t.r + 0.7152f * t.g) + 0.0722f * t.b
              t.c = l + saturation * (t.c - l)            only where saturation != 1
     c      = global.op(m)
     for k = 0 .. nRegions-1, in order:
       mask_k = kajo_hip_matte_mask's mask for regions[k].objects: float32(sum of the selected slots' counts) / float32(samples)
       a      = amount_k * mask_k
       c.c    = c.c + a * (op_k(c).c - c.c)
     out.rgb = c * P;   out.w = F.w
   What follows from it: nothing is clamped above. The saturation step can go below 0 and is left so (the next op's max lifts it).
   Each region sees the result of the regions before it. A pixel with mask_k == 0 keeps c bit for bit through region k: a == 0 adds +-0
   to a value (a finite one: where op_k overflows, 0 * inf is a NaN as anywhere). The mattes are antialiased, so a regraded edge is. A
   value that overflows is +inf, and inf - inf under the saturation step is a NaN whose payload is the machine's. White balance has no
   field of its own: it is gains multiplied into the global slope, in binary64, rounded once (kajo_hip_grade_white_balance,
   kajo_hip_grade_neutral).
   THE IDENTITY CASE: the global op at its defaults and nRegions == 0. The stage then does no device work and the output is the source
   image itself (a negative channel included, which the rule would lift to 0), as the lens does at aperture 0: every chain image is then
   the existing call's bit for bit. No atomics and no cross-lane work: a pixel depends on the inputs through image coordinates only,
   so the frame is the same bits on a second call, on a twin handle and on the root of any number of tile owners. The accumulation,
   the AOVs, the matte tables, the pass count and the counters (kernelMs included) are not touched. Scratch (the output frame, the
   parameter block and the regions' id bitsets, uploaded only when the parameters differ from the last call's) is allocated on first
   use and freed by kajo_hip_destroy.
   Refusals (KAJO_E_INVALID, before any device work and without the handle): NULL params; a slope, offset, power, saturation or amount
   that is not finite or outside its range below; nRegions outside 0..KAJO_GRADE_MAX_REGIONS; a flag bit; a non-zero reserved word;
   in a region in use, n outside 1..KAJO_GRADE_REGION_OBJECTS or a negative object id (regions[nRegions..] are not read). Where other
   stages' parameters are present too, the order is despeckle, grade, lens, glare, local, meter, tone, view, denoise, handle. Then, for
   nRegions > 0, the handle: an id above nPlanes + nSpheres (KAJO_E_INVALID; so is a scene whose nRegions bitsets of nPlanes + nSpheres + 1
   bits, in whole words, exceed the 64 KiB the kernel stages: more than 131071 objects with four regions, 524287 with one), and the state by kajo_hip_matte_mask's rules -- KAJO_E_STATE on a handle without KAJO_FLAG_AOV_MATTE,
   with no pass rendered, on a tiled handle (KAJO_FLAG_AOV_TILED) before kajo_hip_compose_aov with the matte tile buffers or after a
   later render or reset, and on an owner of part of the frame without a composed frame. With nRegions == 0 the handle needs no AOVs. */
#define KAJO_GRADE_MAX_REGIONS 4
#define KAJO_GRADE_REGION_OBJECTS 16
typedef struct KajoGradeOp {      /* ASC CDL order: slope, offset, power, then saturation */
    float slope[3];               /* finite, 0 .. 2^16          (default 1) */
    float offset[3];              /* finite, |.| <= 2^16        (default 0) */
    float power[3];               /* finite, 1/8 .. 8           (default 1) */
    float saturation;             /* finite, 0 .. 4             (default 1) */
    float reserved[2];            /* 0 */
} KajoGradeOp;                    /* 48 bytes */
typedef struct KajoGradeRegion {
    KajoGradeOp op;
    int32_t objects[KAJO_GRADE_REGION_OBJECTS]; /* ids as kajo_hip_matte_mask takes them */
    int32_t n;                    /* 1 .. KAJO_GRADE_REGION_OBJECTS */
    float amount;                 /* finite, 0 .. 1 (default 1) */
    uint32_t reserved[2];         /* 0 */
} KajoGradeRegion;                /* 128 bytes */
typedef struct KajoGradeParams {
    KajoGradeOp global;
    int32_t nRegions;             /* 0 .. KAJO_GRADE_MAX_REGIONS (default 0) */
    uint32_t flags;               /* 0: an unknown bit is refused */
    uint32_t reserved[2];         /* 0 */
    KajoGradeRegion regions[KAJO_GRADE_MAX_REGIONS];
} KajoGradeParams;                /* 576 bytes */
/* The identity: every op at its defaults (the regions' too, amount 1, n 0), nRegions 0. NULL is accepted. */
void kajo_hip_default_grade_params(KajoGradeParams* p);
/* The rule above over n pixels of MEANS, pure host code (no handle, no device), compiled from the device's own lines: rgb = n * 3
   floats (m of the definition), masks = n * nRegions floats (pixel-major: mask_k of pixel i at masks[i * nRegions + k]; may be NULL with
   nRegions == 0), out = n * 3 floats (c of the definition; a pixel that does not count is copied with its bits; under the identity
   case every pixel is). KAJO_E_INVALID for what the stage refuses without a handle, a NULL array or n < 0. */
int kajo_hip_grade_pixels(const KajoGradeParams* p, const float* rgb, const float* masks, int64_t n, float* out);
/* White balance for an illuminant of correlated colour temperature `kelvin` (1667 .. 25000) and a green / magenta `tint` (|tint| <= 1,
   in stops of green gain), pure host code in binary64. The Planckian chromaticity by Kim et al. 2002, T = kelvin:
     x = -0.2661239e9/T^3 - 0.2343589e6/T^2 + 0.8776956e3/T + 0.179910    T <= 4000
         -3.0258469e9/T^3 + 2.1070379e6/T^2 + 0.2226347e3/T + 0.240390    above
     y = -1.1063814 x^3 - 1.34811020 x^2 + 2.18555832 x - 0.20219683      T <= 2222
         -0.9549476 x^3 - 1.37418593 x^2 + 2.09137015 x - 0.16748867      T <= 4000
          3.0817580 x^3 - 5.87338670 x^2 + 3.75112997 x - 0.37001483      above
   XYZ = (x / y, 1, (1 - x - y) / y); linear sRGB through the rows (3.2404542, -1.5371385, -0.4985314), (-0.9692660, 1.8760108,
   0.0415560), (0.0556434, -0.2040259, 1.0572252); a channel <= 1e-3 is KAJO_E_INVALID (the illuminant is outside sRGB: below about
   1900 K). g.c = 1 / rgb.c, g.g *= 2^tint, g /= 0.2126 g.r + 0.7152 g.g + 0.0722 g.b, rounded to float32: a surface lit by that
   illuminant comes out grey at its own luminance. Callers multiply the gains into the global slope in binary64 and round once. */
int kajo_hip_grade_white_balance(double kelvin, double tint, float gains[3]);
/* The "click on what should be grey" form: g.c = Y / rgb.c with Y = 0.2126 r + 0.7152 g + 0.0722 b of the pixel, normalised the same
   way, binary64 rounded to float32. A channel that is not finite or <= 0 is KAJO_E_INVALID. A grey pixel gives (1, 1, 1). */
int kajo_hip_grade_neutral(const float rgb[3], float gains[3]);
/* The frame after the stage: radiance = HOST pointer to width*height*4 floats (row 0 = top), sums over passes; may be NULL. The frame
   kajo_hip_lens with the same first two stages would start from, then this stage. grade == NULL is refused (KAJO_E_INVALID). Waits. */
int kajo_hip_grade(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                   float* radiance);
/* The whole chain: despeckle -> denoise -> grade -> lens -> glare -> local -> meter -> tone mapping -> view, every stage but the tone
   mapping optional (NULL). With grade == NULL exactly kajo_hip_present_view_argb8. argb8 and *result as there. Waits. */
int kajo_hip_present_grade_argb8(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                                 const KajoLensParams* lens, const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                                 const KajoToneParams* tone, const KajoViewParams* view, uint32_t* argb8, KajoMeterResult* result);
/* The twin of kajo_hip_present_view_gathered_argb8_device with the stage behind the despeckle: dst = DEVICE pointer to outW*outH words
   (width*height without a view). The global op works for any number of owners; nRegions > 0 is refused here (KAJO_E_INVALID, with the
   stage's other refusals): regions need whole-frame tables, as the lens needs whole-frame AOVs -- several owners are served through the
   root after kajo_hip_compose and kajo_hip_compose_aov. It adds no wait of its own once its scratch stands (a change of parameters may
   wait for the previous upload of the parameter block to leave its staging, never for a kernel). With grade == NULL exactly that call. */
int kajo_hip_present_grade_gathered_argb8_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle,
                                                 const KajoGradeParams* grade, const KajoGlareParams* g, const KajoLocalParams* local,
                                                 const KajoMeterParams* meter, const KajoToneParams* tone, const KajoViewParams* view, void* dst,
                                                 KajoMeterResult* result);

/* The encode: the finished frame as a 10- or 16-bit integer image, a half-float image or a PQ (SMPTE ST 2084) signal, with optional
   dither -- in place of the tone kernels' undithered 8-bit word, behind the same chain. One kernel of its own
   (kajo_amd/csrc/encode.cpp, arithmetic in encode_math.h) on the handle's stream, compiled once with IEEE float32 arithmetic, correctly
   rounded division and no contraction in every numerics build. THE DEVICE EVALUATES NO pow, exp OR log: the transfer functions are tables
   formed on the host in binary64 and rounded once to float32; the kernel looks up, subtracts, multiplies, adds, compares and converts in
   the order written here, so the kernel, kajo_hip_encode_pixels (the host's twin, the same source lines) and a restatement in any IEEE
   arithmetic give the same words. Off by default: no other entry point changes. Definition -- P = the handle's pass count, F = the
   frame the tone kernels would be handed (the accumulation, or what the stages in front left); per pixel (px, py) of the whole frame:
     1  m = F.rgb / P                one division per channel; the pixel COUNTS where all three channels of m are finite
     2  x = m * s                    s = 2^exposure, formed on the host as the tone mapping's
     3  y = curve(x)                 CLAMP, REINHARD or ACES: "Exposure, tone curves" above, the same expressions in the same order, with
                                     max(t, 0) = t > 0 ? t : 0 (NaN and -0 give +0) and min(t, 1) = t < 1 ? t : 1; l(x) is summed left to
                                     right. A pixel that does not count is mapped by CLAMP. y lies in [0, 1].
     4  v = T(y)                     the integer formats; LINEAR: v = y. T is a table of E = 128 knots per binade over [2^-32, 1): knot
                                     y_i is the float32 whose top 16 bits (sign, exponent, 7 bits of mantissa) are (95 << 7) + i and
                                     whose other bits are 0, i = 0 .. 4096 (y_4096 = 1). With T64 the transfer in binary64,
                                       T_i = (float)T64(y_i),  S_i = (float)((T64(y_i+1) - T64(y_i)) / (y_i+1 - y_i))
                                       2^-32 <= y < 1:  v = min(T_i + (y - y_i) * S_i, T_i+1), i from y's top bits; the subtraction is
                                                        exact, the multiply and the add round once each, the min keeps v non-decreasing
                                       y >= 1:          v = T_4096 = (float)T64(1)
                                       y < 2^-32:       v = y * (float)(T64(2^-32) / 2^-32)
                                     T64: GAMMA22 y^(1/2.2) (the resolve's curve); SRGB 12.92 y for y <= 0.0031308, else 1.055 y^(1/2.4)
                                     - 0.055 (IEC 61966-2-1); PQ ((c1 + c2 L^m1) / (1 + c3 L^m1))^m2 with L = y * peakNits / 10000, m1 =
                                     2610/16384, m2 = 2523/4096 * 128, c1 = 3424/4096, c2 = 2413/4096 * 32, c3 = 2392/4096 * 32 (the
                                     ST 2084 inverse EOTF: y = 1 is shown at peakNits). The table stays within 0.1 of a 16-bit code of
                                     T64 for every float32 y (the sweep that chose E).
     5  code = floor(v * M + d), clamped to [0, M]; M = 255, 1023 or 65535; the multiply and the add round once each. d = 0.5 without
        DITHER; with it d = ((float)(hash >> 8) + 0.5) * 2^-24 in float32 (the sum rounds to even from 2^23 on: d lies in (0, 1]), where,
        in uint32 arithmetic, channel = 0, 1, 2 for r, g, b:
              h = py * 0x85EBCA6B;  h ^= channel * 0xC2B2AE35;  h ^= ditherSeed;
              h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16;
              hash = h + px * 0x9E3779B9
        (a scrambled word per row, channel and seed, then a golden-ratio step per pixel along the row). px, py are frame coordinates:
        the image does not depend on who owns which tile.
     6  RGBA16F stores v = y (LINEAR; no other transfer) rounded to the nearest binary16, ties to even, by integer operations; with
        SCENE the curve is skipped and min(max(x, 0), 65504) is stored, NaN giving 0.
   Words: ARGB8 0xFF << 24 | r << 16 | g << 8 | b (the resolve's layout); RGB10A2 3 << 30 | r << 20 | g << 10 | b; RGBA16 four
   little-endian uint16 r, g, b, a = 65535 (8 bytes, one store); RGBA16F four binary16 r, g, b, a = 1.0 (8 bytes). Row-major, row 0 =
   top, width*height words, nothing beyond kajo_hip_encode_bytes.
   ARGB8 + GAMMA22 without dither is NOT the resolve's image bit for bit: the resolve raises to 1/2.2 with its build's own pow, this
   stage reads a table; the two differ by at most one code at a small share of the pixels (DESIGN.md section 6q has the measured figure).
   Refusals of the parameters (KAJO_E_INVALID, before the handle is looked at), in this order: NULL; an unknown format; an unknown
   transfer; an unknown flag bit; a non-zero reserved word; RGBA16F with a transfer other than LINEAR; SCENE with a format other than
   RGBA16F; DITHER with RGBA16F; with PQ a peakNits that is not finite or not in (0, 10000]. They stand where the view's do: behind the
   tone parameters' own refusals (the two automatic exposures among them), in front of the denoiser's. Behind them
   KAJO_TONE_AUTO_EXPOSURE is refused: its scale is formed inside the tone launch, which this stage replaces -- use metered exposure (a
   KajoMeterParams in the chain), which is patched into the tone parameters on the host and works with the encode. The view
   resamples ARGB8 words, so these entry points take none: "The float view" below has the ones that do. The accumulation, the AOVs, the pass
   count and the counters (kernelMs included) are not touched; the table (32776 bytes) is uploaded when the transfer or peakNits differ
   from the last call's, the image buffer is allocated on first use; both are freed by kajo_hip_destroy. */
#define KAJO_ENCODE_ARGB8 0u
#define KAJO_ENCODE_RGB10A2 1u
#define KAJO_ENCODE_RGBA16 2u
#define KAJO_ENCODE_RGBA16F 3u
#define KAJO_TRANSFER_GAMMA22 0u
#define KAJO_TRANSFER_SRGB 1u
#define KAJO_TRANSFER_PQ 2u
#define KAJO_TRANSFER_LINEAR 3u
#define KAJO_ENCODE_DITHER 1u          /* KajoEncodeParams.flags: integer formats only */
#define KAJO_ENCODE_SCENE 2u           /* KajoEncodeParams.flags: RGBA16F only, scene-linear x without the curve */
#define KAJO_ENCODE_TABLE_WORDS 8194   /* floats of a transfer table: (T_i, S_i) interleaved, i = 0 .. 4096; the last pair is (T64(1), the slope below 2^-32) */
typedef struct KajoEncodeParams {
    uint32_t format;      /* KAJO_ENCODE_* (default ARGB8) */
    uint32_t transfer;    /* KAJO_TRANSFER_* (default GAMMA22) */
    uint32_t flags;       /* KAJO_ENCODE_DITHER, KAJO_ENCODE_SCENE (default 0) */
    float peakNits;       /* PQ: the luminance y = 1 is shown at, in (0, 10000] (default 1000) */
    uint32_t ditherSeed;  /* change it per frame for a temporal dither (default 0) */
    uint32_t reserved[3]; /* 0 */
} KajoEncodeParams;       /* 32 bytes */
void kajo_hip_default_encode_params(KajoEncodeParams* p); /* NULL is accepted */
/* *bytes = the size of a width x height image in p's format (4 or 8 bytes a pixel). The parameters' refusals; width, height >= 1. */
int kajo_hip_encode_bytes(const KajoEncodeParams* p, int width, int height, size_t* bytes);
/* The table of a transfer (GAMMA22, SRGB, PQ; peakNits is read for PQ only): KAJO_ENCODE_TABLE_WORDS floats. Pure host code. Returns the
   word count; table may be NULL (the size query), otherwise capacity >= the count. LINEAR has no table (KAJO_E_INVALID). */
int kajo_hip_encode_table(uint32_t transfer, float peakNits, float* table, size_t capacity);
/* The definition over n pixels of MEANS (m of step 1), pure host code compiled from the kernel's own lines: meanRgb = n * 3 floats, the
   pixels row-major in a rectangle rowWidth wide whose first pixel is (x0, y0) of the frame (pixel i: px = x0 + i % rowWidth, py = y0 +
   i / rowWidth; they matter to the dither only). out: n words of the format. The refusals above (tone included); rowWidth >= 1. */
int kajo_hip_encode_pixels(const KajoEncodeParams* encode, const KajoToneParams* tone, const float* meanRgb, int64_t n, int32_t x0, int32_t y0,
                           int32_t rowWidth, void* out);
/* The stage alone over the handle's whole frame (tileCount 1, or a composed handle, as kajo_hip_tonemap_argb8): dst = HOST pointer to
   kajo_hip_encode_bytes bytes, may be NULL. Waits. */
int kajo_hip_encode(kajo_hip_t h, const KajoEncodeParams* encode, const KajoToneParams* tone, void* dst);
/* The whole chain with the encode in place of the 8-bit word: despeckle -> denoise -> grade -> lens -> glare -> local -> meter -> tone
   curve -> encode, every stage but the last two optional (NULL). kajo_hip_present_grade_argb8 without a view up to the tone curve: the
   words are kajo_hip_encode_pixels of the frame those stages leave, with the tone parameters the meter patched. dst = HOST pointer to
   kajo_hip_encode_bytes bytes (may be NULL); *result as there. Waits. (The name starts with the stage, as kajo_hip_encode: the
   kajo_hip_present_* names are the ARGB8 chain's.) */
int kajo_hip_encode_present(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                            const KajoLensParams* lens, const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                            const KajoToneParams* tone, const KajoEncodeParams* encode, void* dst, KajoMeterResult* result);
/* The twin of kajo_hip_present_grade_gathered_argb8_device, its stages but the view: gathered tile buffers (NULL = the handle's own when
   tileCount == 1) into DEVICE memory, dst = kajo_hip_encode_bytes bytes, 8-byte aligned for the 8-byte formats. Asynchronous on the
   handle's stream: no wait beyond the meter's (a change of transfer or peakNits may wait for the previous upload of the table to leave
   its staging, never for a kernel). The image is the same bits for any number of tile owners, dither included. */
int kajo_hip_encode_present_gathered_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle, const KajoGradeParams* grade,
                                            const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                                            const KajoToneParams* tone, const KajoEncodeParams* encode, void* dst, KajoMeterResult* result);

/* The float view: the view's crop, zoom and supersampled output in front of the encode's transfer -- antialiasing, thumbnails and
   window-sized read-backs at more than 8 bits. The entry points below resample the encode's own display-referred float y of step 3,
   before any quantiser has touched it, where the view resamples the tone kernels' 8-bit words. Two kernels
   of their own (kajo_amd/csrc/encode_view.cpp; arithmetic in encode_math.h, weight rows from view_weights.h) on the handle's stream,
   compiled as the encode's kernel is. Off unless asked for: no other entry point changes. Definition -- P, F, the tone and encode
   parameters as in "The encode", the view parameters as in "The view"; outW x outH the view's output size, W x H the frame's:
     1  Front.     For every source pixel (jx, jy): the encode's steps 1-3 as they stand there (a pixel that does not count is mapped by
                   CLAMP). L[jy][jx].c = y.c, finite and in [0, 1]. With SCENE, L is what step 6 would store before the rounding to
                   half: min(max(x, 0), 65504), NaN giving 0.
     2  Resample.  The view's own weight rows, kajo_hip_view_weights of the same rectangle: the same filters, trimming, KAJO_VIEW_MAX_*
                   limits and refusals. float32, no FMA, every accumulator starts at +0:
                     T[jy][i].c = sum of wx[i][j] * L[jy][j].c over the taps j = first_x[i] .., in increasing j
                     r[o][i].c  = sum of wy[o][y] * T[y][i].c  over the taps y = first_y[o] .., in increasing y
     3  Clamp.     q = min(max(r, 0), 1) with the encode's max and min (LANCZOS3 has negative lobes; a row's weights sum to 1 only
                   within count * 2^-24). With SCENE: min(max(r, 0), 65504).
     4  Back.      The encode's steps 4-6 with q in place of y (with SCENE: of the clamped x) and (px, py) = (i, o): the dither runs
                   over OUTPUT pixel coordinates. outW x outH words of the format, kajo_hip_encode_bytes(p, outW, outH) bytes.
   Consequences. The copy case (the whole frame at its own size, any filter) launches the plain encode and returns its words; under the
   definition it is the identity too: one weight of 1.0 per axis, +0 + 1 * y = y for y >= +0, and the clamp is idempotent. NEAREST
   without dither gives the plain encode's words gathered at floor(u). A constant frame comes back within ONE CODE of the plain encode,
   not necessarily bit-equal: at 16 bits a weight sum count * 2^-24 off 1 moves v * 65535 by up to 0.01 code, which can cross a
   rounding boundary. No division but step 1's, no atomics, no order between workgroups: a word depends on the inputs through image
   coordinates only, so one, two, three and eight tile owners give one image, dither included.
   Refusals (KAJO_E_INVALID, before any device work), in the chain's order: the stages in front, the tone parameters, the view's own
   (as kajo_hip_present_view_argb8), the encode's (KAJO_TONE_AUTO_EXPOSURE behind them), the denoiser's, the handle, the view against
   the frame. A NULL view makes every entry point below exactly the encoded entry point it extends. The weight rows, their pinned
   staging (uploaded once per set of view parameters) and the intermediate T are the view's own scratch, shared with it: allocated on
   first use, grown on demand, freed by kajo_hip_destroy. */
/* The stage alone: kajo_hip_encode with a view. dst = HOST pointer to kajo_hip_encode_bytes(encode, outW, outH) bytes, may be NULL.
   Waits. */
int kajo_hip_encode_view(kajo_hip_t h, const KajoEncodeParams* encode, const KajoToneParams* tone, const KajoViewParams* view, void* dst);
/* kajo_hip_encode_present with the float view: its arguments, with the view in front of the encode. Waits. */
int kajo_hip_encode_view_present(kajo_hip_t h, const KajoDespeckleParams* despeckle, const KajoDenoiseParams* denoise, const KajoGradeParams* grade,
                                 const KajoLensParams* lens, const KajoGlareParams* g, const KajoLocalParams* local, const KajoMeterParams* meter,
                                 const KajoToneParams* tone, const KajoViewParams* view, const KajoEncodeParams* encode, void* dst,
                                 KajoMeterResult* result);
/* The gathered twin, kajo_hip_encode_present_gathered_device with the float view: dst = DEVICE pointer to kajo_hip_encode_bytes(encode,
   outW, outH) bytes, 8-byte aligned for the 8-byte formats. Asynchronous under kajo_hip_present_view_gathered_argb8_device's
   conditions: no wait beyond the meter's once the scratch stands; a change of the view parameters, the transfer or peakNits may wait
   for the previous upload to leave its staging, never for a kernel; a larger view grows the scratch, which waits for the device. A
   NULL handle is answered as there ("null argument"). */
int kajo_hip_encode_view_present_gathered_device(kajo_hip_t h, const void* gathered, const KajoDespeckleParams* despeckle,
                                                 const KajoGradeParams* grade, const KajoGlareParams* g, const KajoLocalParams* local,
                                                 const KajoMeterParams* meter, const KajoToneParams* tone, const KajoViewParams* view,
                                                 const KajoEncodeParams* encode, void* dst, KajoMeterResult* result);
/* The definition over a whole width x height frame of MEANS (m of step 1; meanRgb = width * height * 3 floats, row-major), pure host
   code compiled from the kernels' own lines: no device, no handle. out: outW * outH words of the format (width * height with a NULL
   view). The refusals above, then width, height >= 1, NULL arguments, the view against the frame. */
int kajo_hip_encode_view_pixels(const KajoEncodeParams* encode, const KajoToneParams* tone, const KajoViewParams* view, const float* meanRgb,
                                int32_t width, int32_t height, void* out);

/* The noise estimate (KAJO_FLAG_NOISE): how noisy the frame is, pixel by pixel, from the frame's own passes -- batch means, in kernels of
   their own (kajo_amd/csrc/noise.hip) on the handle's stream, float32 / binary64 IEEE arithmetic without contraction in every numerics
   build: only its input, the accumulation, depends on FAST / EXACT / STRICT.
   BATCHES. Batch b >= 1 is passes 4b-3 .. 4b by ABSOLUTE pass number (KAJO_NOISE_BATCH_PASSES = 4 = the group of the FAST / EXACT totals:
   at such a boundary no group is in progress, so the tile buffer alone is the sum kajo_hip_read_radiance returns). Per slot of the owner's
   tile buffer, when batch b completes:
     T_b = the accumulation's float4 after pass 4b
     D_b = T_b - T_(b-1) per channel, one float32 subtraction, T_0 = 0
     y_b = 0.2126f * D.x + 0.7152f * D.y + 0.0722f * D.z          (the meter's weights; float32, left to right, not contracted, no clamp)
     y_b finite:  n += 1;  s1 += (double)y;  s2 += (double)y * (double)y      (one binary64 multiply and one add, not fused)
     otherwise:   bad += 1
     then T_b is the new baseline
   The record (s1, s2, n, bad) -- KajoNoiseMoments, 32 bytes -- is a function of (scene, parameters, passes rendered), as the frame is:
   not of how the passes were cut into render() calls, launches or owners.
   WHICH BATCHES COUNT: those of which this handle rendered all four passes since the last kajo_hip_reset or kajo_hip_set_pass_count.
   kajo_hip_reset zeroes the records and the baseline. kajo_hip_set_pass_count(P) zeroes the records; the baseline is then the buffer as
   it stands at the first boundary >= P (for P % 4 == 0: the buffer in front of the next launch), and the batches after it count.
   EVALUATION (kajo_hip_noise; per pixel in binary64, results rounded to float32):
     m   = s1 / (4 n)                              mean luminance per pass (n = 0: 0)
     v   = max(s2 - s1 * s1 / n, 0) / (n - 1)      variance of the batch sums
     se  = sqrt(v / n) / 4                         standard error of m
     rel = se / (max(m, 0) + floor)                floor > 0 (default 1e-2), so that black pixels do not dominate
     n < 2: se = rel = -1, "unknown"
   HISTOGRAM, KAJO_NOISE_HIST_WORDS = 516 uint32 words: words 0..513 the meter's bins (KAJO_METER_BINS, the same bit-pattern rule) over
   the float32 rel of the KNOWN pixels (n >= 2); word 514 the unknown pixels; word 515 the pixels with bad > 0 (which are counted among
   the known or the unknown ones too). Words 0..514 add up to the owner's pixels. Integer counts: the histograms of several owners add
   word by word to the whole frame's.
   kajo_hip_noise_evaluate, pure host: known = the sum of words 0..513; rank r = min(known, max(1, ceil((double)q * known))); the bin is
   the smallest b >= 0 whose cumulative count over bins 0..b reaches r; *value = that bin's centre -- the meter's centres for bins 1..513
   (bin 513: 2^16), 2^-17 for bin 0 -- or -1 with known = 0.
   Refusals: KAJO_E_INVALID, before a handle or a device is looked for, for NULL params, a floor that is not finite or not above 0 and a
   quantile that is not finite or outside (0, 1]; then KAJO_E_INVALID for a NULL handle and KAJO_E_STATE for a handle created without
   KAJO_FLAG_NOISE. The accumulation, the pass count and the counters (kernelMs included) are not touched. */
#define KAJO_NOISE_BATCH_PASSES 4
#define KAJO_NOISE_HIST_WORDS 516
typedef struct KajoNoiseParams {
    float floor;            /* > 0, finite (default 1e-2) */
    float quantile;         /* in (0, 1] (default 0.95): KajoNoiseResult.quantileValue */
} KajoNoiseParams;          /* 8 bytes */
typedef struct KajoNoiseMoments {
    double s1, s2;          /* sum and sum of squares of the finite batch luminances */
    uint64_t n, bad;        /* batches with a finite, and with a not finite, luminance */
} KajoNoiseMoments;         /* 32 bytes */
typedef struct KajoNoiseResult {
    int64_t pixels;         /* the owner's pixels: known + unknown */
    int64_t known;          /* pixels with n >= 2 */
    int64_t unknown;        /* pixels with n < 2 */
    int64_t bad;            /* pixels with bad > 0 */
    float quantileValue;    /* kajo_hip_noise_evaluate of the histogram at params.quantile; -1 with known = 0 */
    int32_t reserved[3];    /* 0 */
} KajoNoiseResult;          /* 48 bytes */
void kajo_hip_default_noise_params(KajoNoiseParams* p); /* NULL is accepted */
/* Pure host, no device and no handle. KAJO_E_INVALID: NULL hist or value, a quantile that is not finite or outside (0, 1]. */
int kajo_hip_noise_evaluate(const uint32_t hist[KAJO_NOISE_HIST_WORDS], float quantile, float* value);
/* The noise map of the handle's own pixels. mean, stderror, relative (float) and batches (uint32, n saturated at 2^32 - 1): HOST pointers
   to WHOLE-FRAME row-major planes of width*height words, row 0 = top, of which only the pixels of this owner's tiles are written -- a
   caller hands the same arrays to every owner and needs no gather. hist: HOST pointer to KAJO_NOISE_HIST_WORDS words, this owner's
   histogram. Every out pointer may be NULL. An owner without a tile launches nothing and reports zeros. Waits.
   COST: that of the whole FRAME, not of the owner's share of it. The kernel walks every 64x4 rectangle of the frame, every plane asked
   for comes to the host whole (width*height words), and an owner of part of the frame (tileCount > 1) then walks all width*height pixels
   on the host to copy its own out of a staging copy the handle keeps (4 * width*height words, allocated on the first such call). A
   diagnostic to call per refresh, not per launch; NULL planes cost nothing, the histogram alone is 516 words. */
int kajo_hip_noise(kajo_hip_t h, const KajoNoiseParams* params, float* mean, float* stderror, float* relative, uint32_t* batches, uint32_t* hist,
                   KajoNoiseResult* result);
/* For tests: the raw records. records: HOST pointer to a whole-frame row-major array of width*height KajoNoiseMoments, of which only the
   pixels of this owner's tiles are written. KAJO_E_INVALID on a NULL argument, KAJO_E_STATE without KAJO_FLAG_NOISE. Waits. */
int kajo_hip_read_noise_moments(kajo_hip_t h, KajoNoiseMoments* records);

/* Adaptive sampling (KAJO_FLAG_ADAPTIVE with KAJO_FLAG_NOISE): the passes go where the noise is. Kernels of their own
   (kajo_amd/csrc/adapt_kernels.cpp, the rule in adapt_math.h) on the handle's stream, binary64 / float32 IEEE arithmetic without
   contraction in every numerics build; the render kernels are launched over fewer workgroups and are not changed.
   UNITS. A pixel block is 64 consecutive slots of the owner's tile buffer: one 8x8 block, one wave. A unit is the handle's launch block,
   64 * wavesPerBlock consecutive slots (KajoAdaptState.unitSlots: 64, 128 or 256), gridBlocks of them. A unit is ACTIVE or RETIRED;
   retirement is permanent until kajo_hip_reset.
   THE DECISION is taken at the absolute pass numbers P with P % (4 * checkEvery) == 0 and P >= minPasses, behind the noise update of that
   boundary: a function of (scene, parameters, P), not of how the passes are cut into kajo_hip_render calls or launches. Per slot
     rel   = the noise estimate's evaluation of the slot's record in binary64 with THIS floor, rounded to float32 (what kajo_hip_noise's
             `relative` plane holds for the same floor)
     loud  = n < 2, or rel > target; the record's `bad` is ignored, so that a frame's NaN pixels do not hold a block forever. A slot
             outside the image (or outside the owner's tiles) is never loud
     a pixel block is QUIET when at most `allowance` of its pixels are loud; a unit retires when all its pixel blocks are quiet
   The decision reads a unit's own records only: it does not depend on tileCount or on any other unit.
   RENDERING. Launches after a decision cover the active units only: the grid is their number, the order the handle's cost order (image
   order under KAJO_FLAG_NO_REORDER or before the first measurement) with the retired units taken out; launches of the SPLIT kernels
   list the active units' pixel blocks. The launch shape (SPLIT or not, chunks) is chosen from the whole frame's block count, so a handle's
   kernel kind does not change as units retire. With no unit active kajo_hip_render launches no render kernel and still counts the passes
   (KajoCounters.launches stands still). AOV launches (KAJO_FLAG_AOV) stay whole-frame at every pass: the AOV buffers are those of a
   plain handle bit for bit, and their cost does not shrink with the active set.
   WHAT EVERY READER SEES. Behind every launch of an adaptive handle that has retired a unit, not only at boundaries, a retired slot of
   the tile buffer is rewritten as baseline * f per channel (all four), f = (float)((double)P / (double)p), P the handle's pass count
   after the launch, p = 4 n the slot's own pass count (n counts the finite batches only: a slot with bad > 0 holds more passes than 4 n,
   is scaled by more than its due and reports 4 n in kajo_hip_adapt_passes -- its sum is as a rule not finite anyway); one float32
   multiply, not contracted. (A retired slot with n = 0 -- possible only
   with allowance > 0 -- is left as it is.) An active slot is not touched, and at a batch boundary the noise update runs for active slots
   only, in the noise estimate's arithmetic to the bit; retired slots keep their records and their baseline. The tile buffer with pass
   count P is then a uniform-equivalent sum: kajo_hip_resolve_*, kajo_hip_read_radiance, the gathered resolve, the whole present chain,
   kajo_hip_noise and a multi-GPU gather work unchanged and know nothing of the flag.
   BIAS, the known property of every such scheme: stopping on an estimate made from the samples themselves keeps the pixels whose early
   samples happened to agree; a retired pixel is biased slightly toward its early mean. minPasses and allowance bound it.
   An adaptive handle synchronises its stream once per decision (the state words come to the host, the order goes back).
   OTHER CALLS. kajo_hip_reset makes every unit active again. kajo_hip_set_pass_count with a nonzero argument is refused (KAJO_E_STATE):
   a restored buffer says nothing about per-block pass counts -- checkpoints of adaptive sessions are out of scope. */
typedef struct KajoAdaptParams {
    float target;           /* > 0: a pixel with rel <= target is not loud */
    float floor;            /* > 0, finite (default 1e-2): the floor of rel, as KajoNoiseParams.floor */
    int32_t minPasses;      /* >= 0 (default 16): no decision before it; rounded up to a multiple of checkEvery * 4 */
    int32_t checkEvery;     /* 1 .. 65536 (default 4): batches between decisions */
    int32_t allowance;      /* 0 .. 63 (default 0): loud pixels a quiet pixel block may have */
    int32_t reserved[3];    /* 0 */
} KajoAdaptParams;          /* 32 bytes */
typedef struct KajoAdaptState {
    int64_t units;          /* the handle's units */
    int64_t activeUnits;
    int64_t pixels;         /* the owner's pixels */
    int64_t activePixels;   /* ... of active units */
    int64_t paths;          /* camera paths actually traced since the last reset: active pixels * n^2, summed over the passes */
    int32_t lastDecisionPass; /* the pass of the last decision; 0 = none yet */
    int32_t unitSlots;      /* slots of a unit: 64 * wavesPerBlock */
} KajoAdaptState;           /* 48 bytes */
/* target 0 (to be set by the caller) and the defaults above. NULL is accepted. */
void kajo_hip_default_adapt_params(KajoAdaptParams* p);
/* Accepted only while the handle's pass count is 0 (after create or kajo_hip_reset), otherwise KAJO_E_STATE; until it is called an
   adaptive handle retires nothing. KAJO_E_INVALID, before the handle is looked at: NULL params, a target that is not above 0 (or NaN), a
   floor that is not finite or not above 0, minPasses < 0, checkEvery outside 1 .. 65536, allowance outside 0 .. 63, a nonzero reserved
   word. Then KAJO_E_INVALID for a NULL handle and KAJO_E_STATE for a handle created without KAJO_FLAG_ADAPTIVE. */
int kajo_hip_set_adaptive(kajo_hip_t h, const KajoAdaptParams* params);
/* Waits. KAJO_E_INVALID on a NULL argument, KAJO_E_STATE without KAJO_FLAG_ADAPTIVE. */
int kajo_hip_adapt_state(kajo_hip_t h, KajoAdaptState* state);
/* The per-pixel pass count: the handle's pass count for a pixel of an active unit, 4 n for one of a retired unit. plane: HOST pointer to
   a WHOLE-FRAME row-major plane of width*height words, of which only the pixels of this owner's tiles are written, as kajo_hip_noise
   does. Waits. KAJO_E_INVALID on a NULL argument, KAJO_E_STATE without KAJO_FLAG_ADAPTIVE. */
int kajo_hip_adapt_passes(kajo_hip_t h, uint32_t* plane);
/* Pure host, no device and no handle: the kernel's rule (adapt_math.h, the same lines) over `count` records. loud[i] = 1 where record i
   is loud (as a slot inside the image), else 0; *nLoud their number; either may be NULL. KAJO_E_INVALID: NULL records with count > 0,
   count < 0, or the parameters' refusals above. */
int kajo_hip_adapt_evaluate(const KajoNoiseMoments* records, int64_t count, const KajoAdaptParams* params, uint8_t* loud, int64_t* nLoud);
/* Pure host: the launch order of an adaptive handle (adapt_math.h kajoAdaptOrder). order[nUnits]: the handle's order, the most expensive
   unit first (NULL: image order); state[nUnits]: 0 = active, otherwise retired. out receives the active units in that order -- with
   split != 0 their pixel blocks, unit * wavesPerBlock + k -- and may be NULL to ask for the number of words, which is returned; negative
   = error (NULL state with nUnits > 0, wavesPerBlock outside 1 .. 4, an order word >= nUnits, a capacity too small). */
int64_t kajo_hip_adapt_order(const uint32_t* order, uint32_t nUnits, const uint32_t* state, uint32_t wavesPerBlock, int32_t split, uint32_t* out,
                             size_t capacity);

/* Checkpoints (kajo_amd/csrc/checkpoint.cpp, checkpoint_kernels.cpp, the arithmetic in checkpoint_math.h): a handle's whole accumulated state as a
   self-describing blob, and a restore after which every later pass and every reader gives what the uninterrupted handle gives, bit for
   bit -- the cut of the passes across processes. No render, AOV or display kernel is changed for it; a handle that never calls these
   entry points allocates, launches and returns what it did.
   A SECTION is one handle's state. CANONICAL ORDER of a per-pixel plane: the handle's own in-image pixels in image row-major order, y
   ascending then x ascending, without the pixels of tiles the handle does not own; for tileCount 1 the plain W x H row-major frame.
   Padding slots and slots outside the image never reach the blob. Planes (KAJO_CKPT_*), each present exactly when the handle keeps it:
     SUM            4 words per pixel   the accumulation, always
     CARRY          8                   FAST / EXACT, small scenes: the total of the complete groups of four passes, then the group in
                                        progress -- only while the pass count stands inside a group
     AOV            8                   KAJO_FLAG_AOV: A then B (the tile buffers of KAJO_FLAG_AOV_TILED, else the whole-frame sums)
     MATTE          16                  KAJO_FLAG_AOV_MATTE: the 8 ids, then the 8 counts
     NOISE_BASE     4                   KAJO_FLAG_NOISE: the baseline of the batch in progress
     NOISE_MOMENTS  8                   KAJO_FLAG_NOISE: KajoNoiseMoments as 32-bit words
   and, not per pixel: ADAPT (KAJO_FLAG_ADAPTIVE: the parameters of kajo_hip_set_adaptive, whether they were set, the retired count, the
   paths traced, the last decision, then the state word of every unit) and COUNTERS (KAJO_FLAG_COUNTERS: the four device work counters as
   eight 32-bit words). Scalars in the header: the pass count, the AOVs' pass count, whether a noise baseline is owed. kernelMs and
   launches travel in a TRAILER of 16 bytes that belongs neither to the state nor to its digests. Not saved, because they do not affect
   the bits: the launch-order feedback (measured again), every display stage's scratch, uploaded guide planes.
   LAYOUT, little-endian: KajoCheckpointHeader (its magic "KAJOCKPT", KAJO_CKPT_VERSION), nPlanes KajoCheckpointPlane entries (kind, words
   per pixel, byte offset from the blob's start, bytes, digest), the planes at 16-byte aligned offsets, the trailer.
   FINGERPRINT: a 64-bit hash (checkpoint_math.h kajoCkptMix, chained) of the KajoScene -- its fields in front of the two pointers, then the
   sphere and plane arrays -- and of W, H, S, the depth limit, the seed and the flags that choose what is computed (STRICT, EXACT, NO_GRID,
   NO_SHADOW_LISTS, NO_ONE_LIGHT, AOV_SPECULAR), not of the tile layout, passesPerLaunch or the flags that say which planes exist.
   DIGEST of a per-pixel plane of w words per pixel: the sum modulo 2^64 over its words of mix(mix(p * w + j) ^ b), p = y * W + x the
   pixel's index in the WHOLE frame, j the word, b its 32 bits, mix the splitmix64 finaliser. It depends neither on the tile layout nor on
   the order of summation; the digests of the owners of one frame add up to the whole frame's. ADAPT and COUNTERS: word i counts as pixel
   i of one word. kajo_hip_checkpoint_save and kajo_hip_digest compute the per-pixel digests on the device.
   kajo_hip_checkpoint_bytes, _save, _restore and kajo_hip_digest are SYNCHRONOUS: they wait for the handle's stream as kajo_hip_wait does
   and return when the blob (the handle) is complete.
   kajo_hip_checkpoint_info, pure host (no device, no handle): magic, version, sizes and offsets against `bytes`, and every plane's digest
   recomputed; a truncated or altered blob is KAJO_E_INVALID with a message that names the plane.
   kajo_hip_checkpoint_restore runs info's checks, then holds the fingerprint and the set of planes (CARRY aside) against what the handle
   keeps, and only then touches the handle: a refused restore (KAJO_E_INVALID) leaves it as it was. A HIP error behind the checks
   (KAJO_E_HIP) can leave some planes restored and others not, under the pass count of before: reset or destroy such a handle. It accepts a section of the handle's own layout (tile
   shape, index and count), or a WHOLE-FRAME section (tileCount 1), of which it takes its own pixels. A section with an ADAPT block restores
   into the same layout only (units are launch blocks). Afterwards the pass count, the AOVs' pass count, the carry, the owed baseline and
   the adaptive state are the saved ones; the composed frame, the composed AOVs and the launch order are invalid, the guide planes gone.
   kajo_hip_checkpoint_merge, pure host: the n sections of one frame's owners (tileCount n, every tileIndex once, the same fingerprint,
   pass counts and planes) into one whole-frame section, whose digests are the sums of the sections' and which its own info accepts.
   COUNTERS are added. Sections with an ADAPT block are refused. An owner without a pixel may lack CARRY. */
#define KAJO_CKPT_VERSION 1u
#define KAJO_CKPT_SUM 1u
#define KAJO_CKPT_CARRY 2u
#define KAJO_CKPT_AOV 3u
#define KAJO_CKPT_MATTE 4u
#define KAJO_CKPT_NOISE_BASE 5u
#define KAJO_CKPT_NOISE_MOMENTS 6u
#define KAJO_CKPT_ADAPT 7u
#define KAJO_CKPT_COUNTERS 8u
#define KAJO_CKPT_KINDS 9          /* kinds are 1 .. 8 */
#define KAJO_CKPT_ADAPT_WORDS 16   /* words of the ADAPT block in front of the units' state words */
typedef struct KajoCheckpointPlane {
    uint32_t kind;          /* KAJO_CKPT_* */
    uint32_t wordsPerPixel; /* 0: not per pixel */
    uint64_t offset;        /* from the blob's start, a multiple of 16 */
    uint64_t bytes;
    uint64_t digest;
} KajoCheckpointPlane;      /* 32 bytes */
typedef struct KajoCheckpointHeader {
    char magic[8];          /* "KAJOCKPT" */
    uint32_t version;       /* KAJO_CKPT_VERSION */
    uint32_t nPlanes;
    int32_t width, height, tileW, tileH, tileIndex, tileCount;
    uint32_t flags;         /* KajoParams.flags */
    int32_t samplesPerPass, depthLimit;
    int32_t passesDone;
    uint64_t seed;
    uint64_t fingerprint;
    uint64_t pixels;        /* the section's pixels: the owner's in-image pixels */
    int64_t aovPasses;
    int32_t noiseRebase;    /* 1: a noise baseline is owed (kajo_hip_set_pass_count) */
    int32_t reserved;       /* 0 */
    uint64_t bytes;         /* of the whole section, the trailer included */
} KajoCheckpointHeader;     /* 104 bytes */
typedef struct KajoCheckpointTrailer {
    double kernelMs;
    uint64_t launches;
} KajoCheckpointTrailer;    /* 16 bytes */
typedef struct KajoCheckpointInfo {
    KajoCheckpointHeader header;
    KajoCheckpointTrailer trailer;
    KajoCheckpointPlane planes[KAJO_CKPT_KINDS]; /* the first header.nPlanes of them, in the blob's order */
} KajoCheckpointInfo;       /* 408 bytes */
typedef struct KajoDigest {
    uint64_t plane[KAJO_CKPT_KINDS]; /* by kind; 0 where the handle does not keep the plane */
    uint32_t present;                /* bit k: the handle keeps plane k */
    uint32_t reserved;
} KajoDigest;               /* 80 bytes */
int kajo_hip_checkpoint_bytes(kajo_hip_t h, size_t* bytes);
int kajo_hip_checkpoint_save(kajo_hip_t h, void* blob, size_t capacity, size_t* written);
int kajo_hip_checkpoint_restore(kajo_hip_t h, const void* blob, size_t bytes);
int kajo_hip_checkpoint_info(const void* blob, size_t bytes, KajoCheckpointInfo* out);
int kajo_hip_checkpoint_merge(const void* const* blobs, const size_t* bytes, int n, void* out, size_t capacity, size_t* written);
/* The planes' digests of the live handle, no blob involved: two handles hold the same frame bit for bit exactly when their SUM words
   agree (up to the 2^-64 of a 64-bit hash). */
int kajo_hip_digest(kajo_hip_t h, KajoDigest* out);

/* Use an existing HIP stream (hipStream_t passed as void*) instead of the handle's own; NULL is the null stream. The call waits for the
   stream the handle leaves, so work enqueued before it is complete before anything enqueued after it starts, whichever streams the two
   are. The stream stays the caller's: kajo_hip_destroy waits for it and does not destroy it. */
int kajo_hip_set_stream(kajo_hip_t h, void* stream);

int kajo_hip_counters(kajo_hip_t h, KajoCounters* out);

/* Host-only helper (no GPU needed): what create() stages from a scene -- inverse(16) +
   determinant per object, planes first then spheres, 17 floats each (cpu/Scene.cpp:9-13) and
   the camera basis p1, p2, p3, origin (Renderer.cpp:30-34), 12 floats. For tests. */
int kajo_hip_stage_scene(const KajoScene* scene, float* invDet17, float* basis12);

/* Host-only helper (no GPU needed), for tests: the per-light visibility lists create() stages for large scenes whose spheres
   are all world-space balls (kajo_amd/csrc/device_scene.h DShadowLists) -- what a shadow query tests instead of walking the grid.
   Returns the number of list items (0 = the scene gets no lists; negative = error). *binsPerAxis = n of the 6 x n x n cube-map
   bins per light, *nLights = emissive spheres; lightSphere[nLights] their sphere indices; start[nLights * 6 n^2 + 1],
   key[items], index[items] are filled when non-null (call once with nulls for the sizes). */
int kajo_hip_stage_shadow_lists(const KajoScene* scene, int32_t* binsPerAxis, int32_t* nLights, int32_t* lightSphere, uint32_t* start,
                                size_t startCapacity, float* key, uint32_t* index, size_t itemCapacity);

/* Host-only helper (no GPU needed), for tests: what create() decides about a scene's culling structures (kajo_amd/csrc/stage.cpp).
   closedRoom: the planes, all opaque, leave a BOUNDED convex region around the camera -- every ray of every path starts inside it;
   room[6] its bounding box widened to hold every sphere (min xyz, max xyz). grid: the uniform grid is built (>= 48 spheres, all of
   determinant 1, rigid planes); gridReach: rays starting farther than this from gridCenter walk every sphere instead (the grid's
   margins are sized for nearer ones); 0 = no limit (closed room). shadowLists: per-light visibility lists are built (they need the
   closed room: their margins are sized from its extent). */
typedef struct KajoStageInfo {
    int32_t closedRoom, grid, shadowLists, reserved;
    float room[6];
    float gridCenter[3], gridReach;
} KajoStageInfo;
int kajo_hip_stage_info(const KajoScene* scene, KajoStageInfo* out);

/* Host-only helper (no GPU needed), for tests: the order a handle dispatches its workgroups in (kajo_amd/csrc/launch_order.h), from the
   loop trips its first launch measured per wave -- waveTrips[nBlocks * wavesPerBlock] -- on a chip of `waveSlots` resident waves:
   blocks by cost, the most expensive first, and -- parts = 2 .. 8, the groups of four passes of a launch of FAST / EXACT kernels of a
   small scene -- the last *nParted (cheapest) blocks as `parts` consecutive workgroups of one group each. An order word is
   block | part << 28 | parted << 31. Returns the number of words (order may be NULL to ask for it); negative = error. */
int kajo_hip_launch_order(const uint32_t* waveTrips, uint32_t nBlocks, uint32_t wavesPerBlock, uint32_t waveSlots, int32_t parts, uint32_t* order,
                          size_t capacity, uint32_t* nParted);

/* Known-answer hooks: run the kernels' OWN device functions on caller-supplied rays, so that the
   vectors captured from the compiled reference (tests/golden/kat_trace.npz, kat_shade.npz) can be
   checked on the GPU function by function. All pointers are HOST memory; kat_trace takes any scene
   kajo_hip_create accepted, kat_shade refuses scenes whose hot records exceed 48 KiB of LDS.
     kat_trace: closest hit of Raytracer::trace (renderer/cpu/Raytracer.cpp:126-138) per ray: object index
                (0 = miss, planes 1.., then spheres), ray.maxDistance, position, normal, tangent, binormal.
     kat_shade: trace + Shader::shade (renderer/cpu/Shader.cpp:113-178) of one path per ray from the given
                128-bit RNG state (no jitter draw), with the handle's depth limit: RGB and the RNG state
                afterwards (pins the number of draws). */
int kajo_hip_kat_trace(kajo_hip_t h, int n, const float* origins, const float* dirs, int32_t* objIndex, float* t,
                       float* position, float* normal, float* tangent, float* binormal);
int kajo_hip_kat_shade(kajo_hip_t h, int n, const float* origins, const float* dirs, const uint64_t* states, float* rgb,
                       uint64_t* finalStates);
/* include/kajo_strictmath.h evaluated on the device, element-wise: fn 0 sin, 1 cos, 2 asin, 3 acos, 4 pow(x, y); and the two IEEE
   operations the STRICT / EXACT kernels form by hand (the reference's `/` and glm's sqrt, renderer/cpu/Raytracer.cpp:30-44):
   fn 5 x / y, fn 6 sqrt(x), fn 7 the root as the sphere tests of the walks form it (sqrt(x) but for negative subnormal x). */
int kajo_hip_kat_strictmath(kajo_hip_t h, int fn, int n, const float* x, const float* y, float* out);
/* The same functions (fn 0-4, 6 and 7; y is pow's exponent) at EVERY binary32 x, summed on the device. Binade b = sign * 256 + biased
   exponent holds the arguments with bits b << 23 | m; sums[2 b] = sum over m of bits(r), sums[2 b + 1] = sum of bits(r) * (2 m + 1),
   both mod 2^64, a NaN result counted as 0x7fc00000. sums: 1024 words of HOST memory. The host build of kajo_strictmath.h writes the
   same table (tools/strictmath_binades.c). */
int kajo_hip_kat_strictmath_sweep(kajo_hip_t h, int fn, float y, uint64_t* sums);

const char* kajo_hip_last_error(void);
const char* kajo_hip_version(void);

#ifdef __cplusplus
}
#endif

#endif /* KAJO_HIP_H */
