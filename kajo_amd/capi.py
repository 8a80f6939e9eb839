"""ctypes binding of libkajo_hip.so (include/kajo_hip.h). Host plumbing only.

The library is the product's compute path; there is no Python or CPU fallback: a missing or
unloadable library raises ImportError, a missing GPU makes kajo_hip_create fail.
"""
from __future__ import annotations

import ctypes as C
import os

# PyTorch ships its own copy of the HIP runtime (torch/lib/libamdhip64.so, soname
# libamdhip64.so.7). Two HIP runtimes in one process do not share the GPU, so torch must be
# imported BEFORE libkajo_hip.so: the dynamic loader then satisfies the library's
# libamdhip64.so.7 dependency with the copy torch already mapped, and both use one runtime.
import torch  # noqa: F401  (plumbing: device memory, streams, torch.distributed)

from .scene import KajoScene

_HERE = os.path.dirname(os.path.abspath(__file__))
# KAJO_HIP_LIB: a diagnostic twin of the library (e.g. the -DKAJO_PROFILE build of `make prof`); never a CPU path
LIB_PATH = os.environ.get("KAJO_HIP_LIB") or os.path.join(_HERE, "libkajo_hip.so")

KAJO_OK, KAJO_E_INVALID, KAJO_E_HIP, KAJO_E_NO_DEVICE, KAJO_E_STATE = 0, -1, -2, -3, -4

KAJO_FLAG_FAST = 0  # (neither of the two below)
KAJO_FLAG_STRICT = 1
KAJO_FLAG_COUNTERS = 2
KAJO_FLAG_NO_GRID = 4
KAJO_FLAG_NO_REORDER = 8
KAJO_FLAG_NO_SPLIT = 16
KAJO_FLAG_COOP = 32      # experiment library libkajo_hip_r02.so only
KAJO_FLAG_DEFERRED = 64  # experiment library libkajo_hip_exp.so only
KAJO_FLAG_NO_SHADOW_LISTS = 128
KAJO_FLAG_NO_ONE_LIGHT = 256  # every numerics build: the any-number-of-lights instance for a one-light scene (A/B, tests)
KAJO_FLAG_EXACT = 512  # decision-exact numerics: STRICT's decisions, FAST's radiance arithmetic
KAJO_FLAG_AOV = 1024  # first-hit albedo / normal / depth buffers over the beauty render's camera samples (kajo_hip_read_aov)
KAJO_FLAG_AOV_SPECULAR = 2048  # with KAJO_FLAG_AOV: the buffers are taken at the first non-delta hit, through ideal mirrors and glass
KAJO_FLAG_AOV_MATTE = 4096  # with KAJO_FLAG_AOV: per-pixel (object id, sample count) tables over the AOVs' samples (kajo_hip_read_matte)
KAJO_FLAG_AOV_TILED = 8192  # with KAJO_FLAG_AOV: the sums of the handle's own tiles, any tileIndex / tileCount (kajo_hip_compose_aov)
KAJO_FLAG_NOISE = 16384  # the per-pixel noise estimate: batch moments beside the render, in kernels of their own (kajo_hip_noise)
KAJO_FLAG_ADAPTIVE = 32768  # with KAJO_FLAG_NOISE: units whose estimate has met a target retire, launches cover the others (kajo_hip_set_adaptive)
KAJO_NOISE_BATCH_PASSES = 4  # a batch of the noise estimate: passes 4b-3 .. 4b by absolute number
KAJO_NOISE_HIST_WORDS = 516  # the meter's 514 bins over the relative error, the unknown pixels, the pixels with a bad batch
KAJO_MATTE_SLOTS = 8
KAJO_DENOISE_NO_DEMODULATE = 1  # KajoDenoiseParams.flags: filter the mean radiance itself, not radiance / albedo
KAJO_DENOISE_NOISE_GUIDED = 2  # KajoDenoiseParams.flags: v0 from the measured variance of KAJO_FLAG_NOISE where there is one
KAJO_TONE_CLAMP, KAJO_TONE_REINHARD, KAJO_TONE_ACES = 0, 1, 2  # KajoToneParams.curve
KAJO_TONE_AUTO_EXPOSURE = 1  # KajoToneParams.flags: scale the frame's log-average luminance to `key`
KAJO_METER_BINS = 514  # words of a luminance histogram (kajo_hip_meter): bin 0 below 2^-16, 1..512 sixteen per stop, 513 from 2^16 up
KAJO_METER_AUTO_WHITE = 1  # KajoMeterParams.flags: kajo_hip_meter_tone also sets Reinhard's white from whiteL
KAJO_LENS_MAX_RADIUS = 16  # KajoLensParams.maxRadius: the largest circle of confusion, in pixels
KAJO_VIEW_NEAREST, KAJO_VIEW_AREA, KAJO_VIEW_TRIANGLE, KAJO_VIEW_LANCZOS3 = 0, 1, 2, 3  # KajoViewParams.filter
KAJO_VIEW_FILTERS = {"nearest": KAJO_VIEW_NEAREST, "area": KAJO_VIEW_AREA, "triangle": KAJO_VIEW_TRIANGLE, "lanczos3": KAJO_VIEW_LANCZOS3}
KAJO_VIEW_MAX_SCALE, KAJO_VIEW_MAX_TAPS, KAJO_VIEW_MAX_OUT = 64, 384, 16384  # the view's limits: minification, taps of a row, output edge
KAJO_GRADE_MAX_REGIONS, KAJO_GRADE_REGION_OBJECTS = 4, 16  # KajoGradeParams: regions of a grade, object ids of a region
KAJO_ENCODE_ARGB8, KAJO_ENCODE_RGB10A2, KAJO_ENCODE_RGBA16, KAJO_ENCODE_RGBA16F = 0, 1, 2, 3  # KajoEncodeParams.format
KAJO_ENCODE_FORMATS = {"argb8": KAJO_ENCODE_ARGB8, "rgb10a2": KAJO_ENCODE_RGB10A2, "rgba16": KAJO_ENCODE_RGBA16, "rgba16f": KAJO_ENCODE_RGBA16F}
KAJO_TRANSFER_GAMMA22, KAJO_TRANSFER_SRGB, KAJO_TRANSFER_PQ, KAJO_TRANSFER_LINEAR = 0, 1, 2, 3  # KajoEncodeParams.transfer
KAJO_TRANSFERS = {"gamma22": KAJO_TRANSFER_GAMMA22, "srgb": KAJO_TRANSFER_SRGB, "pq": KAJO_TRANSFER_PQ, "linear": KAJO_TRANSFER_LINEAR}
KAJO_ENCODE_DITHER, KAJO_ENCODE_SCENE = 1, 2  # KajoEncodeParams.flags
KAJO_ENCODE_TABLE_WORDS = 8194  # floats of a transfer table (kajo_hip_encode_table)
KAJO_CKPT_VERSION = 1  # checkpoints (kajo_hip_checkpoint_*): the version of a section, its planes' kinds, the words of an ADAPT block's head
KAJO_CKPT_KINDS = 9
KAJO_CKPT_NAMES = ("?", "SUM", "CARRY", "AOV", "MATTE", "NOISE_BASE", "NOISE_MOMENTS", "ADAPT", "COUNTERS")
(KAJO_CKPT_SUM, KAJO_CKPT_CARRY, KAJO_CKPT_AOV, KAJO_CKPT_MATTE, KAJO_CKPT_NOISE_BASE, KAJO_CKPT_NOISE_MOMENTS, KAJO_CKPT_ADAPT,
 KAJO_CKPT_COUNTERS) = range(1, 9)
KAJO_CKPT_ADAPT_WORDS = 16
KAJO_LOCAL_PIVOT_METERED = 1  # KajoLocalParams.flags: the pivot is the frame's own pivotPercentile-th luminance

# every symbol include/kajo_hip.h declares
EXPORTS = [
    "kajo_hip_default_params", "kajo_hip_create", "kajo_hip_destroy", "kajo_hip_render", "kajo_hip_wait",
    "kajo_hip_reset", "kajo_hip_set_pass_count", "kajo_hip_resolve_argb8", "kajo_hip_read_radiance", "kajo_hip_resolve_argb8_device",
    "kajo_hip_tile_buffer", "kajo_hip_compose", "kajo_hip_set_stream", "kajo_hip_counters",
    "kajo_hip_stage_scene", "kajo_hip_last_error", "kajo_hip_version", "kajo_hip_kat_trace", "kajo_hip_kat_shade",
    "kajo_hip_kat_strictmath", "kajo_hip_kat_strictmath_sweep", "kajo_hip_stage_shadow_lists", "kajo_hip_resolve_gathered_argb8_device", "kajo_hip_stage_info",
    "kajo_hip_launch_order", "kajo_hip_read_aov", "kajo_hip_aov_kernel", "kajo_hip_default_denoise_params", "kajo_hip_denoise",
    "kajo_hip_default_tone_params", "kajo_hip_tonemap_argb8", "kajo_hip_tonemap_gathered_argb8_device", "kajo_hip_tone_scale",
    "kajo_hip_default_glare_params", "kajo_hip_glare", "kajo_hip_display_argb8", "kajo_hip_display_gathered_argb8_device",
    "kajo_hip_default_despeckle_params", "kajo_hip_despeckle", "kajo_hip_present_argb8", "kajo_hip_present_gathered_argb8_device",
    "kajo_hip_despeckle_counts", "kajo_hip_read_matte", "kajo_hip_matte_mask",
    "kajo_hip_default_meter_params", "kajo_hip_meter_evaluate", "kajo_hip_meter_tone", "kajo_hip_meter", "kajo_hip_present_metered_argb8",
    "kajo_hip_present_metered_gathered_argb8_device",
    "kajo_hip_default_local_params", "kajo_hip_local", "kajo_hip_present_local_argb8", "kajo_hip_present_local_gathered_argb8_device",
    "kajo_hip_local_pivot",
    "kajo_hip_default_lens_params", "kajo_hip_lens", "kajo_hip_lens_coc", "kajo_hip_lens_depth_at", "kajo_hip_present_lens_argb8",
    "kajo_hip_aov_tile_buffers", "kajo_hip_compose_aov",
    "kajo_hip_default_view_params", "kajo_hip_view_weights", "kajo_hip_view_tables", "kajo_hip_view_argb8", "kajo_hip_present_view_argb8",
    "kajo_hip_present_view_gathered_argb8_device",
    "kajo_hip_default_grade_params", "kajo_hip_grade_pixels", "kajo_hip_grade_white_balance", "kajo_hip_grade_neutral", "kajo_hip_grade",
    "kajo_hip_present_grade_argb8", "kajo_hip_present_grade_gathered_argb8_device",
    "kajo_hip_default_noise_params", "kajo_hip_noise_evaluate", "kajo_hip_noise", "kajo_hip_read_noise_moments",
    "kajo_hip_default_adapt_params", "kajo_hip_set_adaptive", "kajo_hip_adapt_state", "kajo_hip_adapt_passes", "kajo_hip_adapt_evaluate",
    "kajo_hip_adapt_order",
    "kajo_hip_denoise_guide_planes",
    "kajo_hip_default_encode_params", "kajo_hip_encode_bytes", "kajo_hip_encode_table", "kajo_hip_encode_pixels", "kajo_hip_encode",
    "kajo_hip_encode_present", "kajo_hip_encode_present_gathered_device",
    "kajo_hip_encode_view", "kajo_hip_encode_view_present", "kajo_hip_encode_view_present_gathered_device", "kajo_hip_encode_view_pixels",
    "kajo_hip_checkpoint_bytes", "kajo_hip_checkpoint_save", "kajo_hip_checkpoint_restore", "kajo_hip_checkpoint_info",
    "kajo_hip_checkpoint_merge", "kajo_hip_digest",
]


class KajoStageInfo(C.Structure):
    _fields_ = [("closedRoom", C.c_int32), ("grid", C.c_int32), ("shadowLists", C.c_int32), ("reserved", C.c_int32),
                ("room", C.c_float * 6), ("gridCenter", C.c_float * 3), ("gridReach", C.c_float)]


class KajoDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("flags", C.c_uint32), ("sigmaLuminance", C.c_float), ("sigmaNormal", C.c_float),
                ("sigmaDepth", C.c_float), ("reserved", C.c_float * 3)]


class KajoToneParams(C.Structure):
    _fields_ = [("curve", C.c_int32), ("flags", C.c_uint32), ("exposure", C.c_float), ("white", C.c_float), ("key", C.c_float),
                ("reserved", C.c_float * 3)]


class KajoGlareParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("flags", C.c_uint32), ("strength", C.c_float), ("threshold", C.c_float), ("reserved", C.c_float * 4)]


class KajoDespeckleParams(C.Structure):
    _fields_ = [("factor", C.c_float), ("rank", C.c_int32), ("floor", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_float * 4)]


class KajoMeterParams(C.Structure):
    _fields_ = [("percentile", C.c_float), ("key", C.c_float), ("whitePercentile", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_float * 4)]


class KajoMeterResult(C.Structure):
    _fields_ = [("pixels", C.c_int64), ("nonfinite", C.c_int64), ("under", C.c_int64), ("over", C.c_int64), ("metered", C.c_int64),
                ("anchorL", C.c_float), ("whiteL", C.c_float), ("exposure", C.c_float), ("minBin", C.c_int32), ("maxBin", C.c_int32),
                ("reserved", C.c_int32)]


class KajoNoiseParams(C.Structure):
    _fields_ = [("floor", C.c_float), ("quantile", C.c_float)]


class KajoNoiseMoments(C.Structure):
    _fields_ = [("s1", C.c_double), ("s2", C.c_double), ("n", C.c_uint64), ("bad", C.c_uint64)]


class KajoNoiseResult(C.Structure):
    _fields_ = [("pixels", C.c_int64), ("known", C.c_int64), ("unknown", C.c_int64), ("bad", C.c_int64), ("quantileValue", C.c_float),
                ("reserved", C.c_int32 * 3)]


class KajoAdaptParams(C.Structure):
    _fields_ = [("target", C.c_float), ("floor", C.c_float), ("minPasses", C.c_int32), ("checkEvery", C.c_int32), ("allowance", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class KajoAdaptState(C.Structure):
    _fields_ = [("units", C.c_int64), ("activeUnits", C.c_int64), ("pixels", C.c_int64), ("activePixels", C.c_int64), ("paths", C.c_int64),
                ("lastDecisionPass", C.c_int32), ("unitSlots", C.c_int32)]


class KajoLocalParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("flags", C.c_uint32), ("compression", C.c_float), ("detail", C.c_float), ("sigmaRange", C.c_float),
                ("pivot", C.c_float), ("pivotPercentile", C.c_float), ("reserved", C.c_float)]


class KajoLensParams(C.Structure):
    _fields_ = [("aperture", C.c_float), ("focusDistance", C.c_float), ("maxRadius", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_float * 4)]


class KajoViewParams(C.Structure):
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float), ("outW", C.c_int32), ("outH", C.c_int32),
                ("filter", C.c_uint32), ("flags", C.c_uint32)]


class KajoEncodeParams(C.Structure):
    _fields_ = [("format", C.c_uint32), ("transfer", C.c_uint32), ("flags", C.c_uint32), ("peakNits", C.c_float), ("ditherSeed", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class KajoGradeOp(C.Structure):
    _fields_ = [("slope", C.c_float * 3), ("offset", C.c_float * 3), ("power", C.c_float * 3), ("saturation", C.c_float),
                ("reserved", C.c_float * 2)]


class KajoGradeRegion(C.Structure):
    _fields_ = [("op", KajoGradeOp), ("objects", C.c_int32 * KAJO_GRADE_REGION_OBJECTS), ("n", C.c_int32), ("amount", C.c_float),
                ("reserved", C.c_uint32 * 2)]


class KajoGradeParams(C.Structure):
    _fields_ = [("global_", KajoGradeOp), ("nRegions", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2),
                ("regions", KajoGradeRegion * KAJO_GRADE_MAX_REGIONS)]  # (global_: the header's `global`, a keyword here)


class KajoCheckpointPlane(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("wordsPerPixel", C.c_uint32), ("offset", C.c_uint64), ("bytes", C.c_uint64), ("digest", C.c_uint64)]


class KajoCheckpointHeader(C.Structure):
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint32), ("nPlanes", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("tileW", C.c_int32), ("tileH", C.c_int32), ("tileIndex", C.c_int32), ("tileCount", C.c_int32), ("flags", C.c_uint32),
                ("samplesPerPass", C.c_int32), ("depthLimit", C.c_int32), ("passesDone", C.c_int32), ("seed", C.c_uint64),
                ("fingerprint", C.c_uint64), ("pixels", C.c_uint64), ("aovPasses", C.c_int64), ("noiseRebase", C.c_int32),
                ("reserved", C.c_int32), ("bytes", C.c_uint64)]


class KajoCheckpointTrailer(C.Structure):
    _fields_ = [("kernelMs", C.c_double), ("launches", C.c_uint64)]


class KajoCheckpointInfo(C.Structure):
    _fields_ = [("header", KajoCheckpointHeader), ("trailer", KajoCheckpointTrailer), ("planes", KajoCheckpointPlane * KAJO_CKPT_KINDS)]


class KajoDigest(C.Structure):
    _fields_ = [("plane", C.c_uint64 * KAJO_CKPT_KINDS), ("present", C.c_uint32), ("reserved", C.c_uint32)]


class KajoParams(C.Structure):
    _fields_ = [
        ("samplesPerPass", C.c_int32),
        ("depthLimit", C.c_int32),
        ("seed", C.c_uint64),
        ("flags", C.c_uint32),
        ("device", C.c_int32),
        ("tileW", C.c_int32),
        ("tileH", C.c_int32),
        ("tileIndex", C.c_int32),
        ("tileCount", C.c_int32),
        ("passesPerLaunch", C.c_int32),
    ]


class KajoCounters(C.Structure):
    _fields_ = [
        ("passes", C.c_uint64),
        ("paths", C.c_uint64),
        ("traversals", C.c_uint64),
        ("vertices", C.c_uint64),
        ("primitiveTests", C.c_uint64),
        ("laneSlots", C.c_uint64),
        ("kernelMs", C.c_double),
        ("launches", C.c_uint64),
        ("shadowQueries", C.c_uint64),  # (appended in round 4; the experiment libraries of earlier rounds leave it 0)
        ("tailGroups", C.c_uint64),  # (appended in round 5)
    ]


# The display chain. STAGES: a stage's name -> its parameter block, in chain order; kajo_hip_default_<stage>_params fills one.
STAGES = {"despeckle": KajoDespeckleParams, "denoise": KajoDenoiseParams, "grade": KajoGradeParams, "lens": KajoLensParams,
          "glare": KajoGlareParams, "local": KajoLocalParams, "meter": KajoMeterParams, "tone": KajoToneParams, "view": KajoViewParams,
          "encode": KajoEncodeParams}

# Every chain entry point and its arguments, both in the header's order: `h` the handle, `gathered` the owners' tile buffers, a stage's name
# its parameter block (NULL = the stage is off), `dst` what the call fills (image, radiance or histogram), `scale` a float and `result` a
# KajoMeterResult it writes. lib() sets the argtypes from these rows and HipRenderer lays its calls out by them: a new stage is a row here.
CHAIN_ENTRIES = {
    "kajo_hip_tonemap_argb8": "h tone denoise dst scale",
    "kajo_hip_tonemap_gathered_argb8_device": "h gathered tone dst",
    "kajo_hip_glare": "h glare denoise dst",
    "kajo_hip_display_argb8": "h denoise glare tone dst scale",
    "kajo_hip_display_gathered_argb8_device": "h gathered glare tone dst",
    "kajo_hip_present_argb8": "h despeckle denoise glare tone dst scale",
    "kajo_hip_present_gathered_argb8_device": "h gathered despeckle glare tone dst",
    "kajo_hip_meter": "h despeckle denoise glare meter dst result",
    "kajo_hip_present_metered_argb8": "h despeckle denoise glare meter tone dst result",
    "kajo_hip_present_metered_gathered_argb8_device": "h gathered despeckle glare meter tone dst result",
    "kajo_hip_local": "h despeckle denoise glare local dst",
    "kajo_hip_present_local_argb8": "h despeckle denoise glare local meter tone dst result",
    "kajo_hip_present_local_gathered_argb8_device": "h gathered despeckle glare local meter tone dst result",
    "kajo_hip_lens": "h despeckle denoise lens dst",
    "kajo_hip_present_lens_argb8": "h despeckle denoise lens glare local meter tone dst result",
    "kajo_hip_present_view_argb8": "h despeckle denoise lens glare local meter tone view dst result",
    "kajo_hip_present_view_gathered_argb8_device": "h gathered despeckle glare local meter tone view dst result",
    "kajo_hip_grade": "h despeckle denoise grade dst",
    "kajo_hip_present_grade_argb8": "h despeckle denoise grade lens glare local meter tone view dst result",
    "kajo_hip_present_grade_gathered_argb8_device": "h gathered despeckle grade glare local meter tone view dst result",
    "kajo_hip_encode": "h encode tone dst",
    "kajo_hip_encode_present": "h despeckle denoise grade lens glare local meter tone encode dst result",
    "kajo_hip_encode_present_gathered_device": "h gathered despeckle grade glare local meter tone encode dst result",
    "kajo_hip_encode_view": "h encode tone view dst",
    "kajo_hip_encode_view_present": "h despeckle denoise grade lens glare local meter tone view encode dst result",
    "kajo_hip_encode_view_present_gathered_device": "h gathered despeckle grade glare local meter tone view encode dst result",
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(make -C kajo_amd/csrc)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.kajo_hip_last_error.restype = C.c_char_p
        L.kajo_hip_version.restype = C.c_char_p
        L.kajo_hip_create.argtypes = [C.POINTER(KajoScene), C.c_int, C.c_int, C.POINTER(KajoParams), C.POINTER(C.c_void_p)]
        L.kajo_hip_destroy.argtypes = [C.c_void_p]
        L.kajo_hip_render.argtypes = [C.c_void_p, C.c_int]
        L.kajo_hip_wait.argtypes = [C.c_void_p]
        L.kajo_hip_reset.argtypes = [C.c_void_p]
        L.kajo_hip_set_pass_count.argtypes = [C.c_void_p, C.c_int]
        L.kajo_hip_resolve_argb8.argtypes = [C.c_void_p, C.c_void_p]
        L.kajo_hip_read_radiance.argtypes = [C.c_void_p, C.c_void_p]
        L.kajo_hip_resolve_argb8_device.argtypes = [C.c_void_p, C.c_void_p]
        L.kajo_hip_tile_buffer.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.kajo_hip_compose.argtypes = [C.c_void_p, C.c_void_p]
        L.kajo_hip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.kajo_hip_counters.argtypes = [C.c_void_p, C.POINTER(KajoCounters)]
        L.kajo_hip_stage_scene.argtypes = [C.POINTER(KajoScene), C.c_void_p, C.c_void_p]
        L.kajo_hip_default_params.argtypes = [C.POINTER(KajoParams)]
        if hasattr(L, "kajo_hip_resolve_gathered_argb8_device"):
            L.kajo_hip_resolve_gathered_argb8_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "kajo_hip_stage_shadow_lists"):  # (round 4; the experiment libraries of earlier rounds do not have it)
            L.kajo_hip_stage_shadow_lists.argtypes = [C.POINTER(KajoScene), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                                      C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]
        if hasattr(L, "kajo_hip_stage_info"):
            L.kajo_hip_stage_info.argtypes = [C.POINTER(KajoScene), C.POINTER(KajoStageInfo)]
        if hasattr(L, "kajo_hip_launch_order"):  # (round 6)
            L.kajo_hip_launch_order.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
        if hasattr(L, "kajo_hip_read_aov"):  # (the experiment libraries of earlier rounds do not have it)
            L.kajo_hip_read_aov.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
            L.kajo_hip_aov_kernel.argtypes = [C.c_void_p]
            L.kajo_hip_aov_kernel.restype = C.c_char_p
        if hasattr(L, "kajo_hip_denoise"):  # (nor the denoiser)
            L.kajo_hip_denoise.argtypes = [C.c_void_p, C.POINTER(KajoDenoiseParams), C.c_void_p, C.c_void_p]
        if hasattr(L, "kajo_hip_tone_scale"):  # (nor the tone mapping)
            L.kajo_hip_tone_scale.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        if hasattr(L, "kajo_hip_despeckle"):  # (nor the despeckle)
            L.kajo_hip_despeckle.argtypes = [C.c_void_p, C.POINTER(KajoDespeckleParams), C.c_void_p, C.POINTER(C.c_int64)]
            L.kajo_hip_despeckle_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        if hasattr(L, "kajo_hip_meter"):  # (nor the metering)
            L.kajo_hip_meter_evaluate.argtypes = [C.c_void_p, C.POINTER(KajoMeterParams), C.POINTER(KajoMeterResult)]
            L.kajo_hip_meter_tone.argtypes = [C.POINTER(KajoMeterResult), C.POINTER(KajoMeterParams), C.POINTER(KajoToneParams),
                                              C.POINTER(KajoToneParams)]
            L.kajo_meter_groups.argtypes = [C.c_int, C.c_int]
        if hasattr(L, "kajo_hip_local"):  # (nor the local tone mapping)
            L.kajo_hip_local_pivot.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        if hasattr(L, "kajo_hip_lens"):  # (nor the depth of field)
            L.kajo_hip_lens_coc.argtypes = [C.c_void_p, C.POINTER(KajoLensParams), C.c_void_p, C.c_void_p]
            L.kajo_hip_lens_depth_at.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
        if hasattr(L, "kajo_hip_view_argb8"):  # (nor the view)
            L.kajo_hip_view_weights.argtypes = [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t]
            L.kajo_hip_view_tables.argtypes = [C.c_void_p, C.c_void_p]
            L.kajo_hip_view_tables.restype = None
            L.kajo_hip_view_argb8.argtypes = [C.c_void_p, C.POINTER(KajoViewParams), C.c_void_p, C.c_void_p]
        if hasattr(L, "kajo_hip_grade"):  # (nor the grade)
            L.kajo_hip_grade_pixels.argtypes = [C.POINTER(KajoGradeParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
            L.kajo_hip_grade_white_balance.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_float * 3)]
            L.kajo_hip_grade_neutral.argtypes = [C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3)]
        if hasattr(L, "kajo_hip_encode"):  # (nor the encode)
            L.kajo_hip_encode_bytes.argtypes = [C.POINTER(KajoEncodeParams), C.c_int, C.c_int, C.POINTER(C.c_size_t)]
            L.kajo_hip_encode_table.argtypes = [C.c_uint32, C.c_float, C.c_void_p, C.c_size_t]
            L.kajo_hip_encode_pixels.argtypes = [C.POINTER(KajoEncodeParams), C.POINTER(KajoToneParams), C.c_void_p, C.c_int64, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_void_p]
        if hasattr(L, "kajo_hip_encode_view"):  # (nor the float view)
            L.kajo_hip_encode_view_pixels.argtypes = [C.POINTER(KajoEncodeParams), C.POINTER(KajoToneParams), C.POINTER(KajoViewParams),
                                                      C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        # the display chain: the stages' defaults and the entry points' signatures from the two tables
        slots = dict({stage: C.POINTER(pod) for stage, pod in STAGES.items()}, h=C.c_void_p, gathered=C.c_void_p, dst=C.c_void_p,
                     scale=C.POINTER(C.c_float), result=C.POINTER(KajoMeterResult))
        for stage in STAGES:
            default = getattr(L, "kajo_hip_default_%s_params" % stage, None)
            if default is not None:
                default.argtypes, default.restype = [slots[stage]], None
        for name, row in CHAIN_ENTRIES.items():
            if hasattr(L, name):
                getattr(L, name).argtypes = [slots[slot] for slot in row.split()]
        if hasattr(L, "kajo_hip_read_matte"):  # (nor the mattes)
            L.kajo_hip_read_matte.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
            L.kajo_hip_matte_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "kajo_hip_compose_aov"):  # (nor the tiled AOVs)
            L.kajo_hip_aov_tile_buffers.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                                    C.POINTER(C.c_size_t)]
            L.kajo_hip_compose_aov.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "kajo_hip_noise"):  # (nor the noise estimate)
            L.kajo_hip_default_noise_params.argtypes = [C.POINTER(KajoNoiseParams)]
            L.kajo_hip_default_noise_params.restype = None
            L.kajo_hip_noise_evaluate.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float)]
            L.kajo_hip_noise.argtypes = [C.c_void_p, C.POINTER(KajoNoiseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(KajoNoiseResult)]
            L.kajo_hip_read_noise_moments.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "kajo_hip_denoise_guide_planes"):  # (nor the noise-guided denoiser)
            L.kajo_hip_denoise_guide_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "kajo_hip_set_adaptive"):  # (nor adaptive sampling)
            L.kajo_hip_default_adapt_params.argtypes = [C.POINTER(KajoAdaptParams)]
            L.kajo_hip_default_adapt_params.restype = None
            L.kajo_hip_set_adaptive.argtypes = [C.c_void_p, C.POINTER(KajoAdaptParams)]
            L.kajo_hip_adapt_state.argtypes = [C.c_void_p, C.POINTER(KajoAdaptState)]
            L.kajo_hip_adapt_passes.argtypes = [C.c_void_p, C.c_void_p]
            L.kajo_hip_adapt_evaluate.argtypes = [C.c_void_p, C.c_int64, C.POINTER(KajoAdaptParams), C.c_void_p, C.POINTER(C.c_int64)]
            L.kajo_hip_adapt_order.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_size_t]
            L.kajo_hip_adapt_order.restype = C.c_int64
        if hasattr(L, "kajo_hip_checkpoint_save"):  # (nor checkpoints)
            L.kajo_hip_checkpoint_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
            L.kajo_hip_checkpoint_save.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
            L.kajo_hip_checkpoint_restore.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            L.kajo_hip_checkpoint_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(KajoCheckpointInfo)]
            L.kajo_hip_checkpoint_merge.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_void_p, C.c_size_t,
                                                    C.POINTER(C.c_size_t)]
            L.kajo_hip_digest.argtypes = [C.c_void_p, C.POINTER(KajoDigest)]
        L.kajo_hip_kat_trace.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.kajo_hip_kat_shade.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.kajo_hip_kat_strictmath.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kajo_hip_kat_strictmath_sweep.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        _lib = L
    return _lib


class KajoError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("kajo_hip error %d: %s" % (code, message))
        self.code = code


def check(rc):
    if rc != 0:
        raise KajoError(rc, (lib().kajo_hip_last_error() or b"").decode())
