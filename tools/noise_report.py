"""The noise estimate of a progressive render as text (include/kajo_hip.h "The noise estimate", kajo_hip_noise): after
every `--every` passes the quantile of the relative error the stop rule looks at, the pixels known and bad, and at the end the
histogram of the relative error, one line per stop.

    python tools/noise_report.py [--scene spheres|caustics] [--size WxH] [--spp N] [--passes N] [--every N] [--quantile Q] [--floor F]
                                 [--build exact|fast|strict] [--cost]

--cost renders nothing to report: it times what the flag adds, for a kernel trace (profiles/r1x_noise.txt: rocprofv3 --kernel-trace
--stats -- python tools/noise_report.py --cost --size 1920x1080). It runs, on one handle each, 16 passes as one launch (the unflagged
default), 16 passes as four launches of four (passes_per_launch 4, still unflagged), the same with the flag (the four update kernels
behind them) -- each `--repeat` times (7) after a first step that pays for the cold start, with the least, the median and the largest
wall time -- then ten device-to-device copies of the tile buffer and ten noise maps, with the wall time of each ten. In the kernel trace, in start order, the
ten consecutive `__amd_rocclr_copyBuffer` calls in front of the first kajo_noise_map (the fill of its histogram between) are the ten
copies: their wall time here is that of enqueueing them."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kajo_amd.renderer import HipRenderer  # noqa: E402
from kajo_amd.scene import Scene  # noqa: E402

BUILDS = {"fast": {}, "exact": dict(exact=True), "strict": dict(strict=True)}


def scene_of(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    key = "caustics_a169" if name == "caustics" else "spheres_a169"
    return Scene.from_npz(z, key + "/", key)


def print_histogram(hist):
    known = max(int(hist[:514].astype(np.int64).sum()), 1)
    print("  below 2^-16: %d    unknown: %d    with a bad batch: %d" % (hist[0], hist[514], hist[515]))
    for stop in range(32):
        count = int(hist[1 + 16 * stop:17 + 16 * stop].astype(np.int64).sum())
        if count:
            print("  2^%+3d .. 2^%+3d %9d %5.1f%% %s" % (stop - 16, stop - 15, count, 100.0 * count / known, "#" * int(round(60.0 * count / known))))


def report(args):
    W, H = (int(v) for v in args.size.lower().split("x"))
    with HipRenderer(scene_of(args.scene), W, H, spp=args.spp, noise=True, **BUILDS[args.build]) as r:
        print("%s %dx%d, %d spp a pass, %s; quantile %g, floor %g" % (args.scene, W, H, args.spp, args.build, args.quantile, args.floor))
        out = None
        for done in range(args.every, args.passes + 1, args.every):
            r.render(args.every)
            out = r.noise(floor=args.floor, quantile=args.quantile)
            print("  pass %5d  relative error at the quantile %10.6g   known %d  unknown %d  bad %d" %
                  (done, out["quantile_value"], out["known"], out["unknown"], out["bad"]))
        if out is not None:
            print_histogram(out["hist"])


def cost(args):
    W, H = (int(v) for v in args.size.lower().split("x"))
    sc = scene_of(args.scene)

    def timed(label, **kw):
        with HipRenderer(sc, W, H, spp=args.spp, **BUILDS[args.build], **kw) as r:
            r.render(16).wait()  # (the cold start and the launch order)
            ms = []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                r.render(16).wait()
                ms.append((time.perf_counter() - t0) * 1e3)
            c = r.counters()
            print("  %-44s wall ms of %d steps: min %.2f median %.2f max %.2f [%s]; %d launches, kernelMs %.2f" %
                  (label, len(ms), min(ms), float(np.median(ms)), max(ms), " ".join("%.2f" % v for v in ms), c["launches"], c["kernelMs"]))

    print("%s %dx%d, %d spp a pass, %s: 16 passes" % (args.scene, W, H, args.spp, args.build))
    timed("one launch of 16 (unflagged)")
    timed("four launches of 4 (unflagged)", passes_per_launch=4)
    timed("four launches of 4 + four updates (flagged)", noise=True)
    with HipRenderer(sc, W, H, spp=args.spp, noise=True, **BUILDS[args.build]) as r:
        import torch
        r.render(16).wait()
        ptr, nbytes = r.tile_buffer()
        other = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
        hip = C.CDLL("libamdhip64.so")
        t0 = time.perf_counter()
        for _ in range(10):
            assert hip.hipMemcpy(C.c_void_p(other.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), C.c_int(3)) == 0
        print("  ten device-to-device copies of the tile buffer  %8.2f ms wall (%d bytes each)" % ((time.perf_counter() - t0) * 1e3, nbytes))
        t0 = time.perf_counter()
        for _ in range(10):
            r.noise()
        print("  ten noise maps with their read-back             %8.2f ms wall" % ((time.perf_counter() - t0) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="spheres", choices=["spheres", "caustics"])
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--passes", type=int, default=64)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--quantile", type=float, default=0.95)
    ap.add_argument("--floor", type=float, default=1e-2)
    ap.add_argument("--build", default="exact", choices=sorted(BUILDS))
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--repeat", type=int, default=7, help="--cost: timed steps of 16 passes per handle, after the first")
    args = ap.parse_args()
    (cost if args.cost else report)(args)


if __name__ == "__main__":
    main()
