#!/usr/bin/env python3
"""The encode stage's numbers for DESIGN.md section 6q, on a GPU: spheres.json at 1920x1080.

  times   kajo_hip_encode_present_gathered_device per format (device to device, on the handle's stream) against
          kajo_hip_tonemap_gathered_argb8_device, the tone mapping of the same frame to ARGB8, both under the ACES curve: an event pair
          around a batch of back-to-back calls (a single launch of some 25 us is too near the events' own granularity and the gaps between
          launches issued from Python), warm-up calls first, the median over the repeats of the batch's time per call.
  codes   distinct codes along a fixed scanline of the floor (green channel): 8-bit, 8-bit dithered (distinct means of 64-pixel windows
          against the undithered windows' means), 10-bit, 16-bit.
  resolve the largest difference between ARGB8 / GAMMA22 without dither and kajo_hip_resolve_argb8, and the share of channels that differ:
          under the default tone parameters (clamp, exposure 0), which are the resolve's; the times and the scanline use ACES.

Prints one JSON line. python tools/encode_report.py [--width W --height H --passes P --repeats N --batch B]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--passes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import torch
    from kajo_amd import capi
    from kajo_amd.renderer import HipRenderer, encode_params
    from kajo_amd.scene import Scene

    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "spheres_a169/", "spheres_a169")
    W, H = a.width, a.height
    L = capi.lib()
    out = {"width": W, "height": H, "passes": a.passes, "batch": a.batch, "repeats": a.repeats}
    with HipRenderer(sc, W, H, exact=True) as r:
        S = torch.cuda.Stream()
        r.set_stream(S.cuda_stream)
        r.render(a.passes).wait()
        tone = r._tone_params("aces")
        dst = torch.zeros(W * H * 2, dtype=torch.int32, device="cuda")
        ptr = C.c_void_p(dst.data_ptr())

        def median_ms(call):
            for _ in range(a.warmup):
                call()
            S.synchronize()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S)
                for _ in range(a.batch):
                    call()
                e1.record(S)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.batch)
            return float(np.median(ms)), float(np.min(ms))

        times = {"tonemap_argb8": median_ms(lambda: capi.check(L.kajo_hip_tonemap_gathered_argb8_device(r._h, None, C.byref(tone), ptr)))}
        cases = {"argb8_gamma22": dict(format="argb8"), "argb8_gamma22_dither": dict(format="argb8", dither=True),
                 "argb8_linear": dict(format="argb8", transfer="linear"), "rgb10a2_srgb": dict(format="rgb10a2", transfer="srgb"),
                 "rgb10a2_pq_dither": dict(format="rgb10a2", transfer="pq", dither=True), "rgba16_gamma22": dict(format="rgba16"),
                 "rgba16_pq": dict(format="rgba16", transfer="pq"), "rgba16f_linear": dict(format="rgba16f"),
                 "rgba16f_scene": dict(format="rgba16f", scene=True)}
        for name, e in cases.items():
            p = encode_params(**e)
            times[name] = median_ms(lambda: capi.check(L.kajo_hip_encode_present_gathered_device(r._h, None, None, None, None, None, None,
                                                                                                  C.byref(tone), C.byref(p), ptr, None)))
        out["median_min_ms"] = {k: [round(v[0], 4), round(v[1], 4)] for k, v in times.items()}
        r.set_stream(None)

        row = int(0.9 * H)
        green8 = lambda w: ((w[row] >> 8) & 255).astype(np.int64)
        plain = green8(r.encode(dict(format="argb8"), curve="aces"))
        dith = green8(r.encode(dict(format="argb8", dither=True), curve="aces"))
        n = W // 64 * 64
        wm = lambda c: c[:n].reshape(-1, 64).mean(1)
        out["scanline"] = {"row": row,
                           "codes_8bit": int(len(np.unique(plain))),
                           "window_means_8bit": int(len(np.unique(wm(plain)))),
                           "window_means_8bit_dithered": int(len(np.unique(wm(dith)))),
                           "codes_10bit": int(len(np.unique((r.encode(dict(format="rgb10a2"), curve="aces")[row] >> 10) & 1023))),
                           "codes_16bit": int(len(np.unique(r.encode(dict(format="rgba16"), curve="aces")[row, :, 1])))}
        a8, res = r.encode(dict(format="argb8")), r.argb8()
        diff = np.stack([np.abs(((a8 >> s) & 255).astype(np.int64) - ((res >> s) & 255).astype(np.int64)) for s in (16, 8, 0)])
        out["argb8_gamma22_vs_resolve"] = {"largest_code_difference": int(diff.max()), "share_of_channels_that_differ": float((diff > 0).mean())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
