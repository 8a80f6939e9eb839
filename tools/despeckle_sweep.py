"""Quality sweep of the despeckle stage's parameters (include/kajo_hip.h kajo_hip_despeckle).

EXACT, spheres.json 16:9 at 320x180 (the frame of tests/test_hip_denoise.py's quality test): a reference of 64 x 40 = 2560 samples per
pixel and a frame of 4, both with the AOVs. For every (factor, rank, floor) of the grid, RMSE against the reference in clamped display
range [0, 1] over the pixels finite in the reference and the raw frame:
  a  the raw 4-spp frame                      b  despeckled
  c  denoised (default parameters)            d  despeckled, then denoised (what kajo_hip_present_argb8 runs)
  move  how far the stage moves the reference itself;  clamped, repaired: its two counts on the 4-spp frame
Prints one line per setting, smallest d first; after the grid a few gentler settings (factor 16 and 32, floor up to 1).

    python tools/despeckle_sweep.py [--out FILE]
"""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kajo_amd.renderer import HipRenderer  # noqa: E402
from kajo_amd.scene import Scene  # noqa: E402
from kajo_amd.tiles import TileLayout  # noqa: E402

FACTOR = (2.0, 4.0, 8.0)
RANK = (1, 2, 3)
FLOOR = (0.0, 0.05, 0.2)
# beyond the grid: gentler settings, to see where the clamp stops costing the denoiser energy
EXTRA = [(f, r, x) for f in (16.0, 32.0) for r in (1, 2) for x in (0.2, 1.0)]


def rmse(img, ref, mask):
    return float(np.sqrt(np.mean((np.clip(img, 0, 1) - np.clip(ref, 0, 1))[mask] ** 2)))


def upload(r, frame, passes):
    """Write `frame` (H, W, 4) float32 into the handle's accumulation through its tile buffer and declare it the sum of `passes`."""
    import torch
    from bench import DevicePtr
    H, W = frame.shape[:2]
    r.wait()
    ptr, nbytes = r.tile_buffer()
    buf = torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)
    ys, xs = np.mgrid[0:H, 0:W]
    _, slots = TileLayout(W, H, 1).owner_and_slot(xs, ys)
    buf[torch.as_tensor(slots.reshape(-1).astype(np.int64), device="cuda")] = torch.as_tensor(np.ascontiguousarray(frame).reshape(-1, 4), device="cuda")
    torch.cuda.synchronize()
    r.set_pass_count(passes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "spheres_a169/", "spheres_a169")
    W, H = 320, 180
    ref = HipRenderer(sc, W, H, spp=64, exact=True, aov=True, seed=12345)
    ref.render(40)
    truth = ref.radiance()[..., :3] / ref.passes
    r = HipRenderer(sc, W, H, spp=4, exact=True, aov=True)
    r.render(1)
    acc = r.radiance()
    raw = acc[..., :3] / r.passes
    mask = np.isfinite(truth).all(-1) & np.isfinite(raw).all(-1)
    a = rmse(raw, truth, mask)
    c = rmse(r.denoise()["radiance"][..., :3] / r.passes, truth, mask)
    rows = []
    for factor, rank, floor in list(itertools.product(FACTOR, RANK, FLOOR)) + EXTRA:
        kw = dict(factor=factor, rank=rank, floor=floor)
        upload(r, acc, 1)
        ds = r.despeckle(**kw)
        upload(r, ds["radiance"], 1)  # (the denoiser over the despeckled frame, its float output read back)
        d = rmse(r.denoise()["radiance"][..., :3] / r.passes, truth, mask)
        mv = rmse(ref.despeckle(**kw)["radiance"][..., :3] / ref.passes, truth, mask)
        rows.append((d, rmse(ds["radiance"][..., :3] / r.passes, truth, mask), mv, factor, rank, floor, ds["clamped"], ds["repaired"]))
    ref.close()
    r.close()
    rows.sort()
    lines = ["RMSE (clamped, %d pixels): a raw 4-spp %.6f, c denoised %.6f" % (int(mask.sum()), a, c),
             "%-8s %-8s %-8s %-7s %-5s %-6s %-8s %-8s" % ("d", "b", "move", "factor", "rank", "floor", "clamped", "repaired")]
    lines += ["%-8.6f %-8.6f %-8.6f %-7g %-5d %-6g %-8d %-8d" % row for row in rows]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
