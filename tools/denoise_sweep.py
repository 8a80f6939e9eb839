"""Quality sweep of the A-trous denoiser's sigmas (include/kajo_hip.h kajo_hip_denoise).

EXACT, spheres.json 16:9 at 320x180 (the frame of tests/test_hip_denoise.py's quality test): a reference of 64 x 40 = 2560 samples per
pixel and a frame of 4, both with the AOVs. For every (sigmaLuminance, sigmaNormal, sigmaDepth) of the grid and K = 5, demodulated:
  ratio  RMSE(denoised 4-spp frame) / RMSE(raw 4-spp frame), against the reference
  move   RMSE(denoised reference) / RMSE(raw 4-spp frame): how far the filter moves a frame that has no noise left to remove
RMSE in clamped display range [0, 1] over the pixels finite in the reference and the raw frame. Prints one line per setting, best ratio
first among those whose move stays within 0.25.

    python tools/denoise_sweep.py [--aov-specular] [--out FILE]

--aov-specular: both handles take their AOVs at the first non-delta hit (KAJO_FLAG_AOV_SPECULAR).
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

SIGMA_L = (0.25, 0.5, 1.0, 2.0, 4.0)
SIGMA_N = (32.0, 128.0)
SIGMA_D = (1.0, 4.0, 16.0)


def rmse(img, ref, mask):
    return float(np.sqrt(np.mean((np.clip(img, 0, 1) - np.clip(ref, 0, 1))[mask] ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--aov-specular", action="store_true")
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, "spheres_a169/", "spheres_a169")
    W, H = 320, 180
    ref = HipRenderer(sc, W, H, spp=64, exact=True, aov=True, aov_specular=args.aov_specular, seed=12345)
    ref.render(40)
    truth = ref.radiance()[..., :3] / ref.passes
    r = HipRenderer(sc, W, H, spp=4, exact=True, aov=True, aov_specular=args.aov_specular)
    r.render(1)
    raw = r.radiance()[..., :3] / r.passes
    mask = np.isfinite(truth).all(-1) & np.isfinite(raw).all(-1)
    e_raw = rmse(raw, truth, mask)
    rows = []
    for demod, sl, sn, sd in itertools.product((True, False), SIGMA_L, SIGMA_N, SIGMA_D):
        kw = dict(sigma_luminance=sl, sigma_normal=sn, sigma_depth=sd, demodulate=demod)
        dn = r.denoise(**kw)["radiance"][..., :3] / r.passes
        mv = ref.denoise(**kw)["radiance"][..., :3] / ref.passes
        rows.append((rmse(dn, truth, mask) / e_raw, rmse(mv, truth, mask) / e_raw, demod, sl, sn, sd))
    guides = r.aov_kernel()
    ref.close()
    r.close()
    rows.sort(key=lambda t: (t[1] > 0.25, t[0]))
    lines = ["raw 4-spp RMSE %.4f (clamped, %d pixels); K = 5; guides: %s" % (e_raw, int(mask.sum()), guides),
             "%-7s %-7s %-11s %-8s %-8s %-8s" % ("ratio", "move", "demodulate", "sigmaL", "sigmaN", "sigmaD")]
    lines += ["%-7.3f %-7.3f %-11s %-8g %-8g %-8g" % row for row in rows]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
