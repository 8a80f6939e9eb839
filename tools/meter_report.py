"""The luminance histogram of a rendered frame as text, and the two automatic exposures side by side (include/kajo_hip.h kajo_hip_meter;
DESIGN.md section 6h): the scale the log-average of KAJO_TONE_AUTO_EXPOSURE gives and the scale the histogram's percentile gives, both
for the same key.

    python tools/meter_report.py [--scene spheres|caustics|open_floor|all] [--size WxH] [--spp N] [--passes N] [--percentile Q]
                                 [--white Q] [--key K] [--constant] [--repeat N]

--constant meters a frame of one colour instead of the render (every lane of a wave adds to one LDS counter: the kernel's worst case);
--repeat N runs the log-average tone mapping and the metering N times each, for a kernel trace of the two (profiles/r14_meter.txt:
rocprofv3 --kernel-trace --stats -- python tools/meter_report.py --repeat 20 ...). The histogram is printed one line per stop, sixteen
bins each."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kajo_amd.renderer import HipRenderer  # noqa: E402
from kajo_amd.scene import Scene  # noqa: E402
from kajo_amd.tiles import TileLayout  # noqa: E402


def scene_of(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    if name == "caustics":
        return Scene.from_npz(z, "caustics_a169/", "caustics_a169")
    base = Scene.from_npz(z, "spheres_a169/", "spheres_a169")
    if name == "open_floor":  # spheres.json without its walls and ceiling: most camera rays leave the scene
        return Scene(base.background, base.view, base.proj, base.spheres, base.planes[[0]], "open_floor")
    return base


def upload_constant(r, W, H, passes, rgb=(0.7, 0.25, 1.3)):
    import torch
    from bench import DevicePtr
    r.wait()
    ptr, nbytes = r.tile_buffer()
    buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
    ys, xs = np.mgrid[0:H, 0:W]
    _, slots = TileLayout(W, H, 1).owner_and_slot(xs, ys)
    px = torch.tensor([c * passes for c in rgb] + [1.0], dtype=torch.float32, device="cuda")
    buf[torch.as_tensor(slots.reshape(-1).astype(np.int64), device="cuda")] = px
    torch.cuda.synchronize()
    r.set_pass_count(passes)


def print_histogram(hist, result):
    n = max(int(result["metered"]), 1)
    print("  below 2^-16 (black): %d    not finite: %d    2^16 and above: %d" % (result["under"], result["nonfinite"], result["over"]))
    for stop in range(32):
        count = int(hist[1 + 16 * stop:17 + 16 * stop].astype(np.int64).sum())
        if count:
            print("  2^%+3d .. 2^%+3d %9d %5.1f%% %s" % (stop - 16, stop - 15, count, 100.0 * count / n, "#" * int(round(60.0 * count / n))))


def report(name, args):
    W, H = (int(v) for v in args.size.lower().split("x"))
    with HipRenderer(scene_of(name), W, H, spp=args.spp, exact=True) as r:
        r.render(args.passes).wait()
        if args.constant:
            upload_constant(r, W, H, args.passes)
        params = dict(percentile=args.percentile, white_percentile=args.white, key=args.key)
        for _ in range(max(args.repeat, 1)):
            _, log_scale = r.tonemap(curve="reinhard", auto_exposure=True, key=args.key)
            hist, result = r.meter(**params)
        print("%s %dx%d, %d spp x %d passes%s" % (name, W, H, args.spp, args.passes, ", constant frame" if args.constant else ""))
        print_histogram(hist, result)
        stops = (result["maxBin"] - result["minBin"] + 1) / 16 if result["metered"] else 0.0
        print("  metered %d of %d pixels over %.2f stops; anchor (percentile %g) %.6g, white (percentile %g) %.6g" %
              (result["metered"], result["pixels"], stops, args.percentile, result["anchorL"], args.white, result["whiteL"]))
        print("  scale for key %g: log-average %.6g (%+.3f EV), metered %.6g (%+.3f EV)" %
              (args.key, log_scale, np.log2(log_scale), 2.0 ** result["exposure"], result["exposure"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="spheres", choices=["spheres", "caustics", "open_floor", "all"])
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--percentile", type=float, default=0.5)
    ap.add_argument("--white", type=float, default=0.995)
    ap.add_argument("--key", type=float, default=0.18)
    ap.add_argument("--constant", action="store_true")
    ap.add_argument("--repeat", type=int, default=1)
    args = ap.parse_args()
    for name in (["spheres", "caustics", "open_floor"] if args.scene == "all" else [args.scene]):
        report(name, args)


if __name__ == "__main__":
    main()
