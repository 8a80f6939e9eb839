"""Host-side driver of the HIP backend: the Python counterpart of hip::Scheduler
(kajo_amd/host/HipScheduler.cpp), which in turn stands where cpu::Scheduler stands in the
reference (renderer/cpu/Scheduler.cpp:53-85: own a renderer, run passes, hand pixels to the
Image). Used by the tests, bench.py and the multi-GPU path; all rendering happens in
libkajo_hip.so.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .scene import Scene


NOISE_MOMENTS = np.dtype([("s1", "<f8"), ("s2", "<f8"), ("n", "<u8"), ("bad", "<u8")])  # include/kajo_hip.h KajoNoiseMoments


def noise_evaluate(hist, quantile: float = 0.95) -> float:
    """The `quantile` of the relative error over the known pixels of a noise histogram -- one owner's, or the owners' added word by word
    (include/kajo_hip.h kajo_hip_noise_evaluate; pure host). -1 where no pixel is known."""
    hist = np.ascontiguousarray(hist, np.uint32)
    if hist.shape != (capi.KAJO_NOISE_HIST_WORDS,):
        raise ValueError("a noise histogram has %d words" % capi.KAJO_NOISE_HIST_WORDS)
    value = C.c_float()
    capi.check(capi.lib().kajo_hip_noise_evaluate(hist.ctypes.data_as(C.c_void_p), float(quantile), C.byref(value)))
    return value.value


class AdaptParams:
    """The rule of adaptive sampling (include/kajo_hip.h KajoAdaptParams): a unit retires once every pixel block of it has at most
    `allowance` pixels whose relative error is unknown or above `target`. Fields left None take kajo_hip_default_adapt_params' values
    (floor 1e-2, min_passes 16, check_every 4 batches, allowance 0)."""

    def __init__(self, target: float, floor: float = None, min_passes: int = None, check_every: int = None, allowance: int = None):
        self.target, self.floor, self.min_passes, self.check_every, self.allowance = target, floor, min_passes, check_every, allowance

    def pod(self) -> "capi.KajoAdaptParams":
        p = capi.KajoAdaptParams()
        capi.lib().kajo_hip_default_adapt_params(C.byref(p))
        p.target = float(self.target)
        for field, value in (("floor", self.floor), ("minPasses", self.min_passes), ("checkEvery", self.check_every), ("allowance", self.allowance)):
            if value is not None:
                setattr(p, field, float(value) if field == "floor" else int(value))
        return p


def adapt_evaluate(records, params) -> np.ndarray:
    """Which records are loud under the rule (kajo_hip_adapt_evaluate; pure host, the kernel's own lines): a bool array of records' shape.
    records: NOISE_MOMENTS; params: AdaptParams or a dict of its arguments."""
    records = np.ascontiguousarray(records, NOISE_MOMENTS)
    p = (params if isinstance(params, AdaptParams) else AdaptParams(**params)).pod()
    loud = np.zeros(records.shape, np.uint8)
    capi.check(capi.lib().kajo_hip_adapt_evaluate(records.ctypes.data_as(C.c_void_p), records.size, C.byref(p), loud.ctypes.data_as(C.c_void_p), None))
    return loud.astype(bool)


def adapt_order(order, state, waves_per_block: int, split: bool) -> np.ndarray:
    """The launch order of an adaptive handle (kajo_hip_adapt_order; pure host): `order` (None: image order) without the units whose
    state word is not 0; with split their pixel blocks."""
    state = np.ascontiguousarray(state, np.uint32)
    order = None if order is None else np.ascontiguousarray(order, np.uint32)
    out = np.zeros(state.size * int(waves_per_block), np.uint32)
    n = capi.lib().kajo_hip_adapt_order(None if order is None else order.ctypes.data_as(C.c_void_p), state.size, state.ctypes.data_as(C.c_void_p),
                                        int(waves_per_block), int(bool(split)), out.ctypes.data_as(C.c_void_p), out.size)
    if n < 0:
        capi.check(int(n))
    return out[:n]


def checkpoint_info(blob) -> dict:
    """What a checkpoint section says about itself, after every check that needs no handle -- magic, version, sizes, offsets and every
    plane's digest recomputed (kajo_hip_checkpoint_info; pure host). The header's and the trailer's fields, and `planes`: a dict per plane
    in the section's order (kind, name, wordsPerPixel, offset, bytes, digest). A truncated or altered blob raises KajoError."""
    blob = bytes(blob)
    info = capi.KajoCheckpointInfo()
    capi.check(capi.lib().kajo_hip_checkpoint_info(blob, len(blob), C.byref(info)))
    out = {k: getattr(info.header, k) for k, _ in capi.KajoCheckpointHeader._fields_ if k not in ("magic", "reserved")}
    out.update({k: getattr(info.trailer, k) for k, _ in capi.KajoCheckpointTrailer._fields_})
    out["planes"] = [dict(kind=p.kind, name=capi.KAJO_CKPT_NAMES[p.kind], wordsPerPixel=p.wordsPerPixel, offset=p.offset, bytes=p.bytes,
                          digest=p.digest) for p in info.planes[:info.header.nPlanes]]
    return out


def checkpoint_merge(blobs) -> bytes:
    """The sections of one frame's owners as one whole-frame section (kajo_hip_checkpoint_merge; pure host), which any handle of the same
    scene and parameters restores its own pixels from, whatever its tile layout."""
    blobs = [bytes(b) for b in blobs]
    n = len(blobs)
    if n < 1:
        raise ValueError("no sections to merge")
    keep = [C.create_string_buffer(b, len(b)) for b in blobs]
    ptrs = (C.c_void_p * n)(*[C.cast(k, C.c_void_p) for k in keep])
    sizes = (C.c_size_t * n)(*[len(b) for b in blobs])
    written = C.c_size_t()
    L = capi.lib()
    capi.check(L.kajo_hip_checkpoint_merge(ptrs, sizes, n, None, 0, C.byref(written)))
    out = C.create_string_buffer(written.value)
    capi.check(L.kajo_hip_checkpoint_merge(ptrs, sizes, n, out, written.value, C.byref(written)))
    return out.raw[:written.value]


class HipRenderer:
    def __init__(self, scene: Scene, width: int, height: int, spp: int = 32, depth_limit: int = 8,
                 seed: int = 0o715517, strict: bool = False, exact: bool = False, counters: bool = False, device: int = 0,
                 tile=(64, 16), tile_index: int = 0, tile_count: int = 1, passes_per_launch: int = 0, flags: int = 0,
                 aov: bool = False, aov_specular: bool = False, matte: bool = False, aov_tiled: bool = False, noise: bool = False,
                 adaptive=None):
        L = capi.lib()
        self._L = L
        self.scene = scene
        self.width, self.height = int(width), int(height)
        self.n = int(np.sqrt(float(spp)))  # Renderer.cpp:38
        p = capi.KajoParams()
        L.kajo_hip_default_params(C.byref(p))
        p.samplesPerPass = spp
        p.depthLimit = depth_limit
        p.seed = seed
        p.flags = (capi.KAJO_FLAG_STRICT if strict else 0) | (capi.KAJO_FLAG_EXACT if exact else 0) | (capi.KAJO_FLAG_COUNTERS if counters else 0) | int(flags)
        p.flags |= capi.KAJO_FLAG_AOV if aov else 0
        p.flags |= capi.KAJO_FLAG_AOV_SPECULAR if aov_specular else 0  # (without aov the library refuses it)
        p.flags |= capi.KAJO_FLAG_AOV_MATTE if matte else 0  # (likewise)
        p.flags |= capi.KAJO_FLAG_AOV_TILED if aov_tiled else 0  # (likewise; with it aov takes any tile_index / tile_count)
        p.flags |= capi.KAJO_FLAG_NOISE if noise else 0  # batch moments beside the render: noise(), noise_moments()
        if adaptive is False:
            adaptive = None
        p.flags |= capi.KAJO_FLAG_ADAPTIVE if adaptive is not None else 0  # (without noise the library refuses it): adapt_state(), adapt_passes()
        p.device = device
        p.tileW, p.tileH = tile
        p.tileIndex, p.tileCount = tile_index, tile_count
        p.passesPerLaunch = passes_per_launch
        self.params = p
        self._pod = scene.pod()
        h = C.c_void_p()
        capi.check(L.kajo_hip_create(C.byref(self._pod), self.width, self.height, C.byref(p), C.byref(h)))
        self._h = h
        self.passes = 0
        # adaptive: AdaptParams or a dict of its arguments gives the rule at once; True only sets the flag (set_adaptive() later, or never)
        if adaptive is not None and adaptive is not True:
            try:
                self.set_adaptive(adaptive)
            except Exception:
                self.close()
                raise

    # -- lifecycle -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.kajo_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- rendering -------------------------------------------------------------------------
    def render(self, passes: int = 1, wait: bool = False):
        capi.check(self._L.kajo_hip_render(self._h, int(passes)))
        self.passes += int(passes)
        if wait:
            self.wait()
        return self

    def wait(self):
        capi.check(self._L.kajo_hip_wait(self._h))

    def reset(self):
        capi.check(self._L.kajo_hip_reset(self._h))
        self.passes = 0

    def set_pass_count(self, passes_done: int):
        capi.check(self._L.kajo_hip_set_pass_count(self._h, int(passes_done)))
        self.passes = int(passes_done)

    def set_stream(self, stream_ptr: int):
        capi.check(self._L.kajo_hip_set_stream(self._h, C.c_void_p(stream_ptr)))

    # -- checkpoints -----------------------------------------------------------------------
    def checkpoint(self) -> bytes:
        """The handle's whole accumulated state as one section (kajo_hip_checkpoint_save): a function of (scene, parameters, passes)
        but for its last 16 bytes, the trailer. Waits."""
        size = C.c_size_t()
        capi.check(self._L.kajo_hip_checkpoint_bytes(self._h, C.byref(size)))
        blob = C.create_string_buffer(size.value)
        written = C.c_size_t()
        capi.check(self._L.kajo_hip_checkpoint_save(self._h, blob, size.value, C.byref(written)))
        return blob.raw[:written.value]

    def restore(self, blob):
        """Continue from a section of this handle's layout, or from a whole-frame section (kajo_hip_checkpoint_restore). Every later
        pass and every reader gives what the uninterrupted handle gives. A refused section (KajoError) leaves the handle as it was."""
        blob = bytes(blob)
        capi.check(self._L.kajo_hip_checkpoint_restore(self._h, blob, len(blob)))
        self.passes = checkpoint_info(blob)["passesDone"]
        return self

    def digest(self) -> dict:
        """The 64-bit digests of the planes the handle keeps, by name (kajo_hip_digest): computed on the device, no read-back of the
        planes. The digests of the owners of one frame add up, modulo 2^64, to the whole frame's."""
        d = capi.KajoDigest()
        capi.check(self._L.kajo_hip_digest(self._h, C.byref(d)))
        return {capi.KAJO_CKPT_NAMES[k]: int(d.plane[k]) for k in range(1, capi.KAJO_CKPT_KINDS) if d.present >> k & 1}

    # -- outputs ---------------------------------------------------------------------------
    def radiance(self) -> np.ndarray:
        """(H, W, 4) float32: sum over passes of radiance / S (divide by .passes for the estimate)."""
        out = np.empty((self.height, self.width, 4), np.float32)
        capi.check(self._L.kajo_hip_read_radiance(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def argb8(self) -> np.ndarray:
        """(H, W) uint32 ARGB8, sRGB-encoded, row 0 = top (Image::pixels, renderer/Image.h:18-20)."""
        out = np.empty((self.height, self.width), np.uint32)
        capi.check(self._L.kajo_hip_resolve_argb8(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def counters(self) -> dict:
        c = capi.KajoCounters()
        capi.check(self._L.kajo_hip_counters(self._h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in capi.KajoCounters._fields_}

    def noise(self, floor: float = None, quantile: float = None, out: dict = None) -> dict:
        """The noise map of the handle's own pixels (include/kajo_hip.h "The noise estimate", kajo_hip_noise; the handle needs noise=True):
        mean, stderr, relative (H, W) float32 -- the mean luminance per pass, its standard error and stderr / (max(mean, 0) + floor), -1
        where fewer than two batches of four passes have been counted -- batches (H, W) uint32, hist (516,) uint32 and the result's
        fields pixels, known, unknown, bad, quantile_value. Arguments left None take kajo_hip_default_noise_params' values (floor 1e-2,
        quantile 0.95). out: the dict of an earlier call (another owner's): its planes are written into, this owner's pixels only, so
        that the owners of a frame fill one set of planes; its histogram is not added to."""
        p = capi.KajoNoiseParams()
        self._L.kajo_hip_default_noise_params(C.byref(p))
        if floor is not None:
            p.floor = float(floor)
        if quantile is not None:
            p.quantile = float(quantile)
        shape = (self.height, self.width)
        planes = {k: (out[k] if out is not None else np.zeros(shape, t))
                  for k, t in (("mean", np.float32), ("stderr", np.float32), ("relative", np.float32), ("batches", np.uint32))}
        hist = np.zeros(capi.KAJO_NOISE_HIST_WORDS, np.uint32)
        r = capi.KajoNoiseResult()
        capi.check(self._L.kajo_hip_noise(self._h, C.byref(p), *(planes[k].ctypes.data_as(C.c_void_p) for k in ("mean", "stderr", "relative", "batches")),
                                          hist.ctypes.data_as(C.c_void_p), C.byref(r)))
        return dict(planes, hist=hist, pixels=r.pixels, known=r.known, unknown=r.unknown, bad=r.bad, quantile_value=r.quantileValue)

    def noise_moments(self, out: np.ndarray = None) -> np.ndarray:
        """The raw batch moments (kajo_hip_read_noise_moments): (H, W) records with the fields s1, s2 (float64), n, bad (uint64), of which
        this owner's pixels are written (into `out` where given)."""
        if out is None:
            out = np.zeros((self.height, self.width), NOISE_MOMENTS)
        capi.check(self._L.kajo_hip_read_noise_moments(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_adaptive(self, params):
        """The rule of an adaptive handle (kajo_hip_set_adaptive), accepted while no pass is rendered: AdaptParams or a dict of its arguments."""
        p = (params if isinstance(params, AdaptParams) else AdaptParams(**params)).pod()
        capi.check(self._L.kajo_hip_set_adaptive(self._h, C.byref(p)))

    def adapt_state(self) -> dict:
        """kajo_hip_adapt_state: units, activeUnits, pixels, activePixels, paths (actually traced), lastDecisionPass, unitSlots."""
        s = capi.KajoAdaptState()
        capi.check(self._L.kajo_hip_adapt_state(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in capi.KajoAdaptState._fields_}

    def adapt_passes(self, out: np.ndarray = None) -> np.ndarray:
        """The per-pixel pass count (kajo_hip_adapt_passes): (H, W) uint32, of which this owner's pixels are written (into `out` where given)."""
        if out is None:
            out = np.zeros((self.height, self.width), np.uint32)
        capi.check(self._L.kajo_hip_adapt_passes(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def aov(self) -> dict:
        """First-hit AOVs (include/kajo_hip.h kajo_hip_read_aov; the handle needs aov=True): raw=(A, B), both (H, W, 4) float32 sums --
        A = (albedo.rgb, hits), B = (normal.xyz, depth) -- and the means a denoiser takes: albedo = A.rgb / samples, normal = B.xyz /
        samples, depth = B.w / hits (0 where no sample hit)."""
        A = np.empty((self.height, self.width, 4), np.float32)
        B = np.empty((self.height, self.width, 4), np.float32)
        samples = C.c_int64()
        capi.check(self._L.kajo_hip_read_aov(self._h, A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), C.byref(samples)))
        s = np.float32(max(samples.value, 1))
        hits = A[..., 3].copy()
        depth = np.zeros_like(hits)
        np.divide(B[..., 3], hits, out=depth, where=hits > 0)
        return dict(raw=(A, B), samples=samples.value, albedo=A[..., :3] / s, normal=B[..., :3] / s, depth=depth, hits=hits)

    def matte(self) -> dict:
        """Object-coverage mattes (include/kajo_hip.h kajo_hip_read_matte; the handle needs aov=True, matte=True): ids (H, W, 8) int32 and
        counts (H, W, 8) uint32, a pixel's slots ranked by count (ties by id; empty slots last as id -1, count 0); samples = the AOVs';
        dropped (H, W) int64 = samples - the counts' sum: the samples that met a full table."""
        ids = np.empty((self.height, self.width, capi.KAJO_MATTE_SLOTS), np.int32)
        counts = np.empty((self.height, self.width, capi.KAJO_MATTE_SLOTS), np.uint32)
        samples = C.c_int64()
        capi.check(self._L.kajo_hip_read_matte(self._h, ids.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), C.byref(samples)))
        return dict(ids=ids, counts=counts, samples=samples.value, dropped=samples.value - counts.sum(-1, dtype=np.int64))

    def matte_mask(self, objects):
        """(mask, dominant), both (H, W) float32 (include/kajo_hip.h kajo_hip_matte_mask): the share of the pixel's samples that saw one of
        `objects` (ids as kat_trace reports them: 0 the background, then the planes, then the spheres), and the id that covers most of
        the pixel (-1 before the first pass)."""
        objects = np.ascontiguousarray(objects, np.int32).reshape(-1)
        mask = np.empty((self.height, self.width), np.float32)
        dominant = np.empty((self.height, self.width), np.float32)
        capi.check(self._L.kajo_hip_matte_mask(self._h, objects.ctypes.data_as(C.c_void_p) if objects.size else None, int(objects.size),
                                               mask.ctypes.data_as(C.c_void_p), dominant.ctypes.data_as(C.c_void_p)))
        return mask, dominant

    def _denoise_params(self, iterations: int = 5, sigma_luminance: float = None, sigma_normal: float = None, sigma_depth: float = None,
                        demodulate: bool = True, noise_guided: bool = False):
        p = _stage_params("denoise", sigmaLuminance=sigma_luminance, sigmaNormal=sigma_normal, sigmaDepth=sigma_depth)
        p.iterations = int(iterations)
        p.flags = (0 if demodulate else capi.KAJO_DENOISE_NO_DEMODULATE) | (capi.KAJO_DENOISE_NOISE_GUIDED if noise_guided else 0)
        return p

    def denoise(self, iterations: int = 5, sigma_luminance: float = None, sigma_normal: float = None, sigma_depth: float = None,
                demodulate: bool = True, noise_guided: bool = False) -> dict:
        """Edge-aware A-trous denoise of the frame guided by the first-hit AOVs (include/kajo_hip.h kajo_hip_denoise; the handle needs
        aov=True): radiance = (H, W, 4) float32 sums over passes, as radiance(); argb8 = (H, W) uint32, as argb8(). Sigmas left None take
        kajo_hip_default_denoise_params' values. noise_guided: the luminance weight is scaled by the measured per-pixel variance of the
        noise estimate where there is one (KAJO_DENOISE_NOISE_GUIDED: the handle needs noise=True and the whole frame, or
        denoise_guide_planes()). The accumulation, the AOVs and the noise records are not touched."""
        p = self._denoise_params(iterations, sigma_luminance, sigma_normal, sigma_depth, demodulate, noise_guided)
        radiance = np.empty((self.height, self.width, 4), np.float32)
        argb8 = np.empty((self.height, self.width), np.uint32)
        capi.check(self._L.kajo_hip_denoise(self._h, C.byref(p), radiance.ctypes.data_as(C.c_void_p), argb8.ctypes.data_as(C.c_void_p)))
        return dict(radiance=radiance, argb8=argb8)

    def denoise_guide_planes(self, mean, stderror):
        """The whole frame's noise planes for the noise-guided denoiser of a handle that holds only part of the records
        (kajo_hip_denoise_guide_planes): (H, W) float32 mean and stderr as every owner's noise(out=...) fills them, valid until the pass
        count changes. None, None drops them."""
        if mean is None and stderror is None:
            capi.check(self._L.kajo_hip_denoise_guide_planes(self._h, None, None))
            return
        m, se = (None if a is None else np.ascontiguousarray(a, np.float32) for a in (mean, stderror))
        for a in (m, se):
            if a is not None and a.shape != (self.height, self.width):
                raise ValueError("guide planes must be (height, width)")
        capi.check(self._L.kajo_hip_denoise_guide_planes(self._h, None if m is None else m.ctypes.data_as(C.c_void_p),
                                                         None if se is None else se.ctypes.data_as(C.c_void_p)))

    def tonemap(self, curve: str = "clamp", exposure: float = 0.0, white: float = 0.0, auto_exposure: bool = False, key: float = 0.18,
                denoise: dict = None):
        """Exposure, tone curve and automatic exposure in the resolve (include/kajo_hip.h kajo_hip_tonemap_argb8): -> (argb8, scale), argb8
        = (H, W) uint32 as argb8(), scale = the linear factor s applied to the mean radiance. curve: "clamp" | "reinhard" | "aces".
        denoise: None maps the accumulation; a dict of denoise()'s keyword arguments maps the frame denoise() would give (aov=True). The
        defaults are argb8() bit for bit. The accumulation, the AOVs and the counters are not touched."""
        tone = dict(curve=curve, exposure=exposure, white=white, auto_exposure=auto_exposure, key=key)
        return self._chain("kajo_hip_tonemap_argb8", tone=tone, denoise=denoise)

    def _tone_params(self, curve: str = "clamp", exposure: float = 0.0, white: float = 0.0, auto_exposure: bool = False, key: float = 0.18):
        if curve not in _CURVES:
            raise ValueError("curve must be one of %s" % ", ".join(_CURVES))
        p = _tone_curve(curve, exposure, white)
        p.flags = capi.KAJO_TONE_AUTO_EXPOSURE if auto_exposure else 0
        p.key = float(key)
        return p

    def _glare_params(self, levels: int = None, strength: float = None, threshold: float = None):
        return _stage_params("glare", levels=levels, strength=strength, threshold=threshold)

    def glare(self, levels: int = None, strength: float = None, threshold: float = None, denoise: dict = None) -> np.ndarray:
        """The frame after the glare (bloom) pyramid (include/kajo_hip.h kajo_hip_glare): (H, W, 4) float32 sums over passes, as
        radiance(). Arguments left None take kajo_hip_default_glare_params' values (6 levels, strength 0.1, threshold 0). denoise: None
        glares the accumulation; a dict of denoise()'s keyword arguments glares the frame denoise() would give (aov=True). The
        accumulation, the AOVs and the counters are not touched."""
        return self._chain("kajo_hip_glare", glare=dict(levels=levels, strength=strength, threshold=threshold), denoise=denoise)

    def display(self, denoise: dict = None, glare: dict = None, **tone):
        """The display chain (include/kajo_hip.h kajo_hip_display_argb8): denoise (optional) -> glare (optional) -> tone mapping ->
        (argb8, scale) as tonemap(). denoise: a dict of denoise()'s keyword arguments; glare: a dict of glare()'s levels / strength /
        threshold; tone: tonemap()'s curve, exposure, white, auto_exposure, key. With glare None it is tonemap(denoise=denoise, **tone)."""
        return self._chain("kajo_hip_display_argb8", tone=tone, denoise=denoise, glare=glare)

    def _despeckle_params(self, factor: float = None, rank: int = None, floor: float = None):
        return _stage_params("despeckle", factor=factor, rank=rank, floor=floor)

    def despeckle(self, factor: float = None, rank: int = None, floor: float = None) -> dict:
        """The frame with its NaN / Inf pixels repaired and its fireflies clamped (include/kajo_hip.h kajo_hip_despeckle): radiance =
        (H, W, 4) float32 sums over passes, as radiance(); clamped, repaired = the numbers of pixels the two steps changed. Arguments left
        None take kajo_hip_default_despeckle_params' values (factor 16, rank 1, floor 0.2); factor 0 repairs only. The accumulation, the
        AOVs and the counters are not touched."""
        p = self._despeckle_params(factor, rank, floor)
        out = np.empty((self.height, self.width, 4), np.float32)
        counts = (C.c_int64 * 2)()
        capi.check(self._L.kajo_hip_despeckle(self._h, C.byref(p), out.ctypes.data_as(C.c_void_p), counts))
        return dict(radiance=out, clamped=int(counts[0]), repaired=int(counts[1]))

    def despeckle_counts(self):
        """(clamped, repaired) of the handle's most recent despeckle (include/kajo_hip.h kajo_hip_despeckle_counts)."""
        counts = (C.c_int64 * 2)()
        capi.check(self._L.kajo_hip_despeckle_counts(self._h, counts))
        return int(counts[0]), int(counts[1])

    def _meter_params(self, percentile: float = None, key: float = None, white_percentile: float = None, auto_white: bool = False):
        p = _stage_params("meter", percentile=percentile, key=key, whitePercentile=white_percentile)
        p.flags = capi.KAJO_METER_AUTO_WHITE if auto_white else 0
        return p

    @staticmethod
    def _meter_result(r) -> dict:
        return {k: getattr(r, k) for k, _ in capi.KajoMeterResult._fields_ if k != "reserved"}

    def meter(self, despeckle: dict = None, denoise: dict = None, glare: dict = None, **params):
        """The luminance histogram of the frame present() with the same three stages would tone-map, and what it says (include/kajo_hip.h
        kajo_hip_meter): -> (hist, result), hist = (514,) uint32 -- bin 0 below 2^-16, bins 1..512 sixteen per stop up to 2^16, bin 513
        above -- and result = a dict of KajoMeterResult's fields (pixels, nonfinite, under, over, metered, anchorL, whiteL, exposure in
        stops, minBin, maxBin). params: percentile (0.5), key (0.18), white_percentile (0.995), auto_white. The accumulation, the AOVs
        and the counters are not touched."""
        return self._chain("kajo_hip_meter", meter=params, despeckle=despeckle, denoise=denoise, glare=glare)

    def _local_params(self, compression: float = None, detail: float = None, sigma_range: float = None, iterations: int = None,
                      pivot: float = None, metered: bool = False, pivot_percentile: float = None):
        p = _stage_params("local", compression=compression, detail=detail, sigmaRange=sigma_range, pivot=pivot,
                          pivotPercentile=pivot_percentile, iterations=iterations)
        p.flags = capi.KAJO_LOCAL_PIVOT_METERED if metered else 0
        return p

    def local(self, despeckle: dict = None, denoise: dict = None, glare: dict = None, **params) -> np.ndarray:
        """The frame after the local tone mapping (include/kajo_hip.h kajo_hip_local): (H, W, 4) float32 sums over passes, as radiance().
        params: compression (0.6), detail (1), sigma_range (2 stops), iterations (5), pivot (log2(0.18)), metered (the pivot is the
        frame's own pivot_percentile-th luminance, 0.5); those left out take kajo_hip_default_local_params' values. despeckle, denoise,
        glare: the stages in front, as present(). The accumulation, the AOVs and the counters are not touched."""
        return self._chain("kajo_hip_local", local=params, despeckle=despeckle, denoise=denoise, glare=glare)

    def local_pivot(self) -> float:
        """The pivot (log2 luminance) of the most recent local tone mapping (include/kajo_hip.h kajo_hip_local_pivot)."""
        pivot = C.c_float()
        capi.check(self._L.kajo_hip_local_pivot(self._h, C.byref(pivot)))
        return pivot.value

    def _lens_params(self, aperture: float = None, focus_distance: float = None, max_radius: int = None):
        return _stage_params("lens", aperture=aperture, focusDistance=focus_distance, maxRadius=max_radius)

    def lens(self, despeckle: dict = None, denoise: dict = None, **params) -> np.ndarray:
        """The frame after the depth of field (include/kajo_hip.h kajo_hip_lens): (H, W, 4) float32 sums over passes, as radiance().
        params: aperture (0.01, the circle of confusion's radius at infinite depth as a fraction of the frame's height), focus_distance
        (10, in the depth AOV's units), max_radius (16 pixels); those left out take kajo_hip_default_lens_params' values. despeckle,
        denoise: the stages in front, as present(). Needs aov=True. The accumulation, the AOVs and the counters are not touched."""
        return self._chain("kajo_hip_lens", lens=params, despeckle=despeckle, denoise=denoise)

    def lens_coc(self, **params) -> dict:
        """The depth of field's decisions (include/kajo_hip.h kajo_hip_lens_coc): dict(radius=(H, W) float32 circle of confusion in pixels,
        depth=(H, W) float32, +inf = far). params as lens()."""
        l = self._lens_params(**params)
        radius = np.empty((self.height, self.width), np.float32)
        depth = np.empty((self.height, self.width), np.float32)
        capi.check(self._L.kajo_hip_lens_coc(self._h, C.byref(l), radius.ctypes.data_as(C.c_void_p), depth.ctypes.data_as(C.c_void_p)))
        return dict(radius=radius, depth=depth)

    def lens_depth_at(self, x: int, y: int) -> float:
        """The depth the lens sees at one pixel (include/kajo_hip.h kajo_hip_lens_depth_at): what to focus on; inf = far."""
        z = C.c_float()
        capi.check(self._L.kajo_hip_lens_depth_at(self._h, int(x), int(y), C.byref(z)))
        return z.value

    def _view_params(self, out_w: int = None, out_h: int = None, rect=None, filter=None):
        return view_params(self.width, self.height, out_w, out_h, rect, filter)

    def view(self, image: np.ndarray, **params) -> np.ndarray:
        """The view of a caller's image (include/kajo_hip.h kajo_hip_view_argb8): crop, zoom or supersampled output of an (H, W) uint32
        image of 0xAARRGGBB words, resampled in linear light -> (out_h, out_w) uint32. params: out_w, out_h (the frame's size where
        left out), rect (x0, y0, x1, y1) in source pixels (the whole frame where left out), filter ("nearest", "area" -- the default --,
        "triangle", "lanczos3", or a KAJO_VIEW_* value). Needs no pass rendered; nothing of the handle's state is touched."""
        v = self._view_params(**params)
        src = np.ascontiguousarray(image, np.uint32)
        if src.shape != (self.height, self.width):
            raise ValueError("the image must be (%d, %d), the handle's frame" % (self.height, self.width))
        out = np.empty((v.outH, v.outW), np.uint32)
        capi.check(self._L.kajo_hip_view_argb8(self._h, C.byref(v), src.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def grade(self, despeckle: dict = None, denoise: dict = None, **params) -> np.ndarray:
        """The frame after the grade (include/kajo_hip.h kajo_hip_grade): (H, W, 4) float32 sums over passes, as radiance(). params as
        grade_params(): slope, offset, power (a number or three), saturation, white_balance (gains multiplied into the slope), regions
        (a list of dicts: objects, amount and the op's keys; they need aov=True, matte=True). despeckle, denoise: the stages in front, as
        present(). The accumulation, the AOVs, the matte tables and the counters are not touched."""
        return self._chain("kajo_hip_grade", grade=params, despeckle=despeckle, denoise=denoise)

    def _encoded_array(self, e, v=None):
        h, w = (self.height, self.width) if v is None else (max(v.outH, 0), max(v.outW, 0))
        if e.format in (capi.KAJO_ENCODE_ARGB8, capi.KAJO_ENCODE_RGB10A2):
            return np.empty((h, w), np.uint32)
        return np.empty((h, w, 4), np.float16 if e.format == capi.KAJO_ENCODE_RGBA16F else np.uint16)

    def encode(self, encode: dict = None, view: dict = None, **tone) -> np.ndarray:
        """The encode stage alone over the handle's frame (include/kajo_hip.h kajo_hip_encode): exposure and tone curve as tonemap()'s
        (no automatic exposure), then the transfer, the dither and the format of encode_params(**encode) -> (H, W) uint32 for "argb8"
        and "rgb10a2", (H, W, 4) uint16 for "rgba16", (H, W, 4) float16 for "rgba16f". view: a dict of view()'s params puts the float
        view between the tone curve and the transfer (kajo_hip_encode_view): the array then has the view's shape (out_h, out_w).
        Nothing of the handle's state is touched."""
        return self._chain("kajo_hip_encode" if view is None else "kajo_hip_encode_view", tone=tone, encode=encode or {}, view=view)

    def present(self, despeckle: dict = None, denoise: dict = None, glare: dict = None, meter: dict = None, local: dict = None,
                lens: dict = None, view: dict = None, grade: dict = None, encode: dict = None, **tone):
        """The whole display chain over the handle's frame (include/kajo_hip.h kajo_hip_present_*_argb8, kajo_hip_encode_present), the
        stages in its order, every one but the tone mapping optional (None = the stage is off):
          despeckle  a dict of despeckle()'s factor / rank / floor: NaN / Inf pixels repaired, fireflies clamped
          denoise    a dict of denoise()'s keyword arguments (the handle needs aov=True)
          grade      a dict of grade()'s params (regions need aov=True, matte=True)
          lens       a dict of lens()'s params: the depth of field (aov=True)
          glare      a dict of glare()'s levels / strength / threshold
          local      a dict of local()'s params: the local tone mapping
          meter      a dict of meter()'s params: the frame the stages above leave is metered, `exposure` becomes a compensation on top
                     of the metered one and auto_white sets Reinhard's white
          tone       the keyword arguments left over, tonemap()'s curve, exposure, white, auto_exposure, key
          view       a dict of view()'s params: crop, zoom or supersampled output; the array then has the view's shape (out_h, out_w)
          encode     a dict of encode_params()'s arguments: the transfer, the dither and the format in place of the 8-bit word; a view
                     then runs in float between the tone curve and the transfer
        The call goes to the narrowest entry point that takes every stage given. Without encode -> (argb8, second): argb8 (H, W) uint32
        as argb8(), second the result dict of meter() with a meter, else the scale s as tonemap()'s. With encode -> (array, second): the
        array as encode()'s, second the result dict of meter() with a meter, else None. The accumulation, the AOVs and the counters are
        not touched."""
        stages = dict(tone=tone, encode=encode, despeckle=despeckle, denoise=denoise, grade=grade, lens=lens, glare=glare, local=local,
                      meter=meter, view=view)
        given = {stage for stage, spec in stages.items() if spec is not None}
        if encode is not None:
            entry = "kajo_hip_encode_present" if view is None else "kajo_hip_encode_view_present"
        else:  # (the host present entries are nested: each takes the stages of the one before it and one more)
            entry = next(name for name, row in capi.CHAIN_ENTRIES.items()
                         if name.startswith("kajo_hip_present_") and name.endswith("_argb8") and given <= set(row.split()))
        return self._chain(entry, **stages)

    def _chain(self, entry: str, **stages):
        """The one call site of the chain entry points (capi.CHAIN_ENTRIES): stages = a dict of its builder's arguments per stage (None =
        the stage is off), built in the order given. The output is allocated by what the entry fills, the arguments laid out by the
        entry's row. -> the array; with a `scale` slot (array, scale); with a `result` slot (array, the result dict of meter() with a
        meter, else None for an encoded array and tone_scale() for an 8-bit one)."""
        slots = capi.CHAIN_ENTRIES[entry].split()
        builder = lambda stage: {"grade": grade_params, "encode": encode_params}.get(stage) or getattr(self, "_%s_params" % stage)
        pods = {stage: builder(stage)(**spec) for stage, spec in stages.items() if spec is not None}
        assert set(pods) <= set(slots), (entry, sorted(pods))
        view = pods.get("view")
        if "encode" in slots:
            out = self._encoded_array(pods["encode"], view)
        elif "tone" in slots:
            out = np.empty((self.height, self.width) if view is None else (max(view.outH, 0), max(view.outW, 0)), np.uint32)
        elif "result" in slots:  # (the meter alone)
            out = np.empty(capi.KAJO_METER_BINS, np.uint32)
        else:
            out = np.empty((self.height, self.width, 4), np.float32)
        scale, result = C.c_float(), capi.KajoMeterResult()
        fixed = dict(h=self._h, dst=out.ctypes.data_as(C.c_void_p), scale=C.byref(scale), result=C.byref(result))
        capi.check(getattr(self._L, entry)(*[fixed[slot] if slot in fixed else _ref(pods.get(slot)) for slot in slots]))
        if "scale" in slots:
            return out, scale.value
        if "result" not in slots:
            return out
        if "meter" in pods:
            return out, self._meter_result(result)
        return out, (None if "encode" in slots else self.tone_scale())

    def tone_scale(self) -> float:
        """The scale s of the most recent tone mapping (include/kajo_hip.h kajo_hip_tone_scale)."""
        scale = C.c_float()
        capi.check(self._L.kajo_hip_tone_scale(self._h, C.byref(scale)))
        return scale.value

    def aov_kernel(self):
        """Name of the AOV kernel instance the handle launches (None without aov=True)."""
        name = self._L.kajo_hip_aov_kernel(self._h)
        return name.decode() if name else None

    # -- known-answer hooks ----------------------------------------------------------------
    def kat_trace(self, origins, dirs):
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = o.shape[0]
        idx = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        pos, nor, tan, bi = (np.zeros((n, 3), np.float32) for _ in range(4))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(self._L.kajo_hip_kat_trace(self._h, n, p(o), p(d), p(idx), p(t), p(pos), p(nor), p(tan), p(bi)))
        return dict(idx=idx, t=t, position=pos, normal=nor, tangent=tan, binormal=bi)

    def kat_shade(self, origins, dirs, states):
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        st = np.ascontiguousarray(states, np.uint64)
        n = o.shape[0]
        rgb = np.zeros((n, 3), np.float32)
        fin = np.zeros((n, 2), np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(self._L.kajo_hip_kat_shade(self._h, n, p(o), p(d), p(st), p(rgb), p(fin)))
        return rgb, fin

    def kat_strictmath(self, fn, x, y=None):
        """include/kajo_strictmath.h (fn 0 sin, 1 cos, 2 asin, 3 acos, 4 pow) and the kernels' x / y (5) and sqrt (6), element-wise."""
        x = np.ascontiguousarray(x, np.float32)
        y = x if y is None else np.ascontiguousarray(np.broadcast_to(np.asarray(y, np.float32), x.shape))
        out = np.zeros_like(x)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(self._L.kajo_hip_kat_strictmath(self._h, fn, x.size, p(x), p(y), p(out)))
        return out

    def kat_strictmath_sweep(self, fn, y=0.0):
        """The checksums (A, B) of fn (not 5) over every binary32 argument: a (512, 2) uint64 array, row = sign * 256 + biased exponent."""
        sums = np.zeros((512, 2), np.uint64)
        capi.check(self._L.kajo_hip_kat_strictmath_sweep(self._h, fn, float(y), sums.ctypes.data_as(C.c_void_p)))
        return sums

    # -- multi-GPU plumbing ----------------------------------------------------------------
    def tile_buffer(self):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        capi.check(self._L.kajo_hip_tile_buffer(self._h, C.byref(ptr), C.byref(nbytes)))
        return ptr.value, nbytes.value

    def compose(self, gathered_device_ptr: int):
        capi.check(self._L.kajo_hip_compose(self._h, C.c_void_p(gathered_device_ptr)))

    def aov_tile_buffers(self):
        """(aov_ptr, aov_bytes, matte_ptr, matte_bytes) of a handle with aov_tiled=True (include/kajo_hip.h kajo_hip_aov_tile_buffers):
        device pointers; matte_ptr is None and matte_bytes 0 without matte=True."""
        aov, aov_bytes, matte, matte_bytes = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        capi.check(self._L.kajo_hip_aov_tile_buffers(self._h, C.byref(aov), C.byref(aov_bytes), C.byref(matte), C.byref(matte_bytes)))
        return aov.value, aov_bytes.value, matte.value, matte_bytes.value

    def compose_aov(self, gathered_aov_ptr=None, gathered_matte_ptr=None):
        """The whole-frame AOVs (and coverage tables) of this handle from the owners' gathered tile buffers, device pointers in rank order
        (include/kajo_hip.h kajo_hip_compose_aov); None = the handle's own buffer where it is the frame's one owner."""
        capi.check(self._L.kajo_hip_compose_aov(self._h, C.c_void_p(gathered_aov_ptr), C.c_void_p(gathered_matte_ptr)))


def _ref(p):
    return None if p is None else C.byref(p)


def _stage_params(stage, **fields):
    """The stage's parameter block (capi.STAGES) at its defaults, with the fields that were given (not None) set."""
    p = capi.STAGES[stage]()
    getattr(capi.lib(), "kajo_hip_default_%s_params" % stage)(C.byref(p))
    for field, value in fields.items():
        if value is not None:
            setattr(p, field, type(getattr(p, field))(value))  # int() or float(), by the field
    return p


_CURVES = {"clamp": capi.KAJO_TONE_CLAMP, "reinhard": capi.KAJO_TONE_REINHARD, "aces": capi.KAJO_TONE_ACES}


def _tone_curve(curve, exposure, white):
    """KajoToneParams of a curve's name (KeyError where unknown), an exposure and a white point: no automatic exposure."""
    p = _stage_params("tone")
    p.curve, p.exposure, p.white = _CURVES[curve], float(exposure), float(white)
    return p


def _grade_op(op, slope=None, offset=None, power=None, saturation=None):
    for field, value in (("slope", slope), ("offset", offset), ("power", power)):
        if value is not None:
            getattr(op, field)[:] = [float(v) for v in np.broadcast_to(np.asarray(value, np.float64), (3,))]
    if saturation is not None:
        op.saturation = float(saturation)


def grade_params(slope=None, offset=None, power=None, saturation=None, white_balance=None, regions=()):
    """KajoGradeParams (include/kajo_hip.h): the global op's slope, offset, power (a number or three; those left out keep the defaults 1, 0,
    1) and saturation (1); white_balance = gains (grade_white_balance(), grade_neutral()) multiplied into the slope in binary64 and
    rounded once; regions = up to four dicts of objects (ids as matte_mask() takes them), amount (1) and the op's keys. Nothing is
    checked here: the library refuses what is out of range."""
    p = _stage_params("grade")
    if white_balance is not None:
        base = np.broadcast_to(np.asarray(1.0 if slope is None else slope, np.float64), (3,))
        slope = base * np.asarray(white_balance, np.float64)
    _grade_op(p.global_, slope, offset, power, saturation)
    regions = list(regions)
    p.nRegions = len(regions)
    for r, spec in zip(p.regions, regions):
        spec = dict(spec)
        objects = [int(o) for o in np.asarray(spec.pop("objects"), np.int64).reshape(-1)]
        r.n = len(objects)
        r.objects[:min(r.n, capi.KAJO_GRADE_REGION_OBJECTS)] = objects[:capi.KAJO_GRADE_REGION_OBJECTS]
        if "amount" in spec:
            r.amount = float(spec.pop("amount"))
        _grade_op(r.op, **spec)
    return p


def grade_pixels(rgb, masks=None, **params) -> np.ndarray:
    """Host-only: the grade's rule over pixels of MEANS (include/kajo_hip.h kajo_hip_grade_pixels), the device's own lines compiled for
    the host. rgb (..., 3) float32; masks (..., nRegions) float32, one plane per region; params as grade_params(), or params=a
    KajoGradeParams."""
    p = params["params"] if "params" in params else grade_params(**params)
    rgb = np.ascontiguousarray(rgb, np.float32)
    n = rgb.size // 3
    m = None
    if masks is not None:
        m = np.ascontiguousarray(masks, np.float32)
        if m.size != n * max(p.nRegions, 0):
            raise ValueError("masks must hold nRegions floats per pixel")
    out = np.empty_like(rgb)
    capi.check(capi.lib().kajo_hip_grade_pixels(C.byref(p), rgb.ctypes.data_as(C.c_void_p), None if m is None else m.ctypes.data_as(C.c_void_p), n,
                                                out.ctypes.data_as(C.c_void_p)))
    return out


def grade_white_balance(kelvin: float, tint: float = 0.0) -> np.ndarray:
    """Host-only: the gains (3,) float32 that make a surface lit by a `kelvin` illuminant grey at its own luminance (include/kajo_hip.h
    kajo_hip_grade_white_balance); tint in stops of green gain."""
    g = (C.c_float * 3)()
    capi.check(capi.lib().kajo_hip_grade_white_balance(float(kelvin), float(tint), C.byref(g)))
    return np.array(g[:], np.float32)


def grade_neutral(rgb) -> np.ndarray:
    """Host-only: the gains (3,) float32 that make the pixel `rgb` grey at its own luminance (include/kajo_hip.h kajo_hip_grade_neutral)."""
    src = (C.c_float * 3)(*[float(v) for v in rgb])
    g = (C.c_float * 3)()
    capi.check(capi.lib().kajo_hip_grade_neutral(C.byref(src), C.byref(g)))
    return np.array(g[:], np.float32)


def encode_params(format="argb8", transfer=None, dither: bool = False, scene: bool = False, peak_nits: float = None, dither_seed: int = 0):
    """KajoEncodeParams (include/kajo_hip.h "The encode"): format "argb8" | "rgb10a2" | "rgba16" | "rgba16f", transfer "gamma22" | "srgb" |
    "pq" | "linear" (or the KAJO_ENCODE_* / KAJO_TRANSFER_* values; the transfer defaults to "linear" for "rgba16f", else to "gamma22"),
    dither, scene (scene-linear halves), peak_nits for "pq", dither_seed."""
    p = _stage_params("encode", peakNits=peak_nits)
    p.format = capi.KAJO_ENCODE_FORMATS[format] if isinstance(format, str) else int(format)
    if transfer is None:
        transfer = "linear" if p.format == capi.KAJO_ENCODE_RGBA16F else "gamma22"
    p.transfer = capi.KAJO_TRANSFERS[transfer] if isinstance(transfer, str) else int(transfer)
    p.flags = (capi.KAJO_ENCODE_DITHER if dither else 0) | (capi.KAJO_ENCODE_SCENE if scene else 0)
    p.ditherSeed = int(dither_seed) & 0xFFFFFFFF
    return p


def encode_table(transfer="gamma22", peak_nits: float = 1000.0) -> np.ndarray:
    """The table of a transfer (include/kajo_hip.h kajo_hip_encode_table): (4097, 2) float32 rows (T_i, S_i); the last row is (T64(1),
    the slope below 2^-32). Host code: no device is opened."""
    t = capi.KAJO_TRANSFERS[transfer] if isinstance(transfer, str) else int(transfer)
    out = np.zeros(capi.KAJO_ENCODE_TABLE_WORDS, np.float32)
    n = capi.lib().kajo_hip_encode_table(t, float(peak_nits), out.ctypes.data_as(C.c_void_p), out.size)
    if n < 0:
        capi.check(n)
    return out[:n].reshape(-1, 2)


def encode_pixels(mean_rgb, encode: dict = None, x0: int = 0, y0: int = 0, row_width: int = None, curve: str = "clamp", exposure: float = 0.0,
                  white: float = 0.0) -> np.ndarray:
    """The encode over an array (..., 3) of MEANS on the host, the kernel's own lines (include/kajo_hip.h kajo_hip_encode_pixels) -> n
    words, uint32 or uint64 by the format. The pixels are row-major in a rectangle row_width wide (default: all in one row) whose first
    pixel is (x0, y0) of the frame; that matters to the dither only."""
    e = encode if isinstance(encode, capi.KajoEncodeParams) else encode_params(**(encode or {}))
    t = _tone_curve(curve, exposure, white)
    m = np.ascontiguousarray(mean_rgb, np.float32).reshape(-1, 3)
    wide = e.format in (capi.KAJO_ENCODE_RGBA16, capi.KAJO_ENCODE_RGBA16F)
    out = np.zeros(len(m), np.uint64 if wide else np.uint32)
    capi.check(capi.lib().kajo_hip_encode_pixels(C.byref(e), C.byref(t), m.ctypes.data_as(C.c_void_p), len(m), int(x0), int(y0),
                                                 int(row_width or max(len(m), 1)), out.ctypes.data_as(C.c_void_p)))
    return out


def view_params(width: int, height: int, out_w: int = None, out_h: int = None, rect=None, filter=None):
    """KajoViewParams (include/kajo_hip.h "The view") for a width x height frame, as HipRenderer.view()'s params: out_w, out_h (the frame's
    size where left out), rect (x0, y0, x1, y1) in source pixels (the whole frame where left out), filter (a name or a KAJO_VIEW_* value)."""
    p = _stage_params("view")
    p.outW = int(width) if out_w is None else int(out_w)
    p.outH = int(height) if out_h is None else int(out_h)
    if rect is not None:
        p.x0, p.y0, p.x1, p.y1 = (float(v) for v in rect)
    if filter is not None:
        p.filter = capi.KAJO_VIEW_FILTERS[filter] if isinstance(filter, str) else int(filter)
    return p


def encode_view_pixels(mean_rgb, encode: dict = None, view: dict = None, curve: str = "clamp", exposure: float = 0.0, white: float = 0.0) -> np.ndarray:
    """The float view over a whole frame (H, W, 3) of MEANS on the host, the kernels' own lines (include/kajo_hip.h
    kajo_hip_encode_view_pixels) -> (out_h, out_w) words, uint32 or uint64 by the format. view: view_params()'s arguments (or a
    KajoViewParams); None is the plain encode of the frame."""
    m = np.ascontiguousarray(mean_rgb, np.float32)
    if m.ndim != 3 or m.shape[2] != 3:
        raise ValueError("the means must be (H, W, 3)")
    H, W = m.shape[:2]
    e = encode if isinstance(encode, capi.KajoEncodeParams) else encode_params(**(encode or {}))
    v = view if isinstance(view, capi.KajoViewParams) or view is None else view_params(W, H, **view)
    t = _tone_curve(curve, exposure, white)
    wide = e.format in (capi.KAJO_ENCODE_RGBA16, capi.KAJO_ENCODE_RGBA16F)
    shape = (H, W) if v is None else (max(v.outH, 0), max(v.outW, 0))
    out = np.zeros(shape, np.uint64 if wide else np.uint32)
    capi.check(capi.lib().kajo_hip_encode_view_pixels(C.byref(e), C.byref(t), None if v is None else C.byref(v), m.ctypes.data_as(C.c_void_p),
                                                      W, H, out.ctypes.data_as(C.c_void_p)))
    return out


def view_weights(src_n: int, a0: float, a1: float, out_n: int, filter="area"):
    """Host-only: the view's weight rows of one axis (include/kajo_hip.h kajo_hip_view_weights) -> (first [out_n] int32, count [out_n]
    int32, weights [out_n, stride] float32 with zeros behind a row's count)."""
    L = capi.lib()
    f = capi.KAJO_VIEW_FILTERS[filter] if isinstance(filter, str) else int(filter)
    n = L.kajo_hip_view_weights(src_n, a0, a1, out_n, f, None, None, None, 0)
    if n < 0:
        capi.check(n)
    first = np.zeros(out_n, np.int32)
    count = np.zeros(out_n, np.int32)
    weights = np.zeros((out_n, n // out_n), np.float32)
    rc = L.kajo_hip_view_weights(src_n, a0, a1, out_n, f, first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                                 weights.ctypes.data_as(C.c_void_p), n)
    if rc < 0:
        capi.check(rc)
    return first, count, weights


def view_tables():
    """Host-only: the view's transfer tables (include/kajo_hip.h kajo_hip_view_tables) -> (lin [256], thresholds [255]) float32."""
    lin = np.zeros(256, np.float32)
    thresholds = np.zeros(255, np.float32)
    capi.lib().kajo_hip_view_tables(lin.ctypes.data_as(C.c_void_p), thresholds.ctypes.data_as(C.c_void_p))
    return lin, thresholds


def stage_scene(scene: Scene):
    """Host-only: (inverse+determinant per object [n,17], camera basis [4,3]) as create() stages them."""
    L = capi.lib()
    n = scene.n_planes + scene.n_spheres
    inv = np.zeros((n, 17), np.float32)
    basis = np.zeros((4, 3), np.float32)
    pod = scene.pod()
    capi.check(L.kajo_hip_stage_scene(C.byref(pod), inv.ctypes.data_as(C.c_void_p), basis.ctypes.data_as(C.c_void_p)))
    return inv, basis


def stage_info(scene: Scene) -> dict:
    """Host-only: what create() decides about the scene's culling structures (include/kajo_hip.h KajoStageInfo)."""
    L = capi.lib()
    pod = scene.pod()
    info = capi.KajoStageInfo()
    capi.check(L.kajo_hip_stage_info(C.byref(pod), C.byref(info)))
    return dict(closed_room=bool(info.closedRoom), grid=bool(info.grid), shadow_lists=bool(info.shadowLists), room=np.array(info.room[:], np.float32),
                grid_center=np.array(info.gridCenter[:], np.float32), grid_reach=float(info.gridReach))


def stage_shadow_lists(scene: Scene):
    """Host-only: the per-light visibility lists create() stages for a large scene (device_scene.h DShadowLists), or None when
    the scene gets none. -> dict(n=bins per cube-face axis, lights=[sphere index], start=[nLights * 6 n^2 + 1], key, index)."""
    L = capi.lib()
    pod = scene.pod()
    n, nl = C.c_int32(), C.c_int32()
    items = L.kajo_hip_stage_shadow_lists(C.byref(pod), C.byref(n), C.byref(nl), None, None, 0, None, None, 0)
    if items < 0:
        capi.check(items)
    if n.value == 0:
        return None
    lights = np.zeros(nl.value, np.int32)
    start = np.zeros(nl.value * 6 * n.value * n.value + 1, np.uint32)
    key = np.zeros(items, np.float32)
    index = np.zeros(items, np.uint32)
    rc = L.kajo_hip_stage_shadow_lists(C.byref(pod), C.byref(n), C.byref(nl), lights.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p),
                                       start.size, key.ctypes.data_as(C.c_void_p), index.ctypes.data_as(C.c_void_p), items)
    if rc < 0:
        capi.check(rc)
    return dict(n=n.value, lights=lights, start=start, key=key, index=index)
