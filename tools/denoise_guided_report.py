"""What the noise-guided denoiser does and what it costs (include/kajo_hip.h KAJO_DENOISE_NOISE_GUIDED).

QUALITY (--quality): EXACT, a scene of tests/golden/scenes.npz at WxH. The truth is 64 x 40 = 2560 samples per pixel on a handle that
keeps the noise estimate too; the noisy frames are --passes passes of S = 4, one per seed. RMSE in clamped display range [0, 1] over
the pixels finite in both, as tests/test_hip_denoise.py forms it:
  e_ref_plain, e_ref_guided   how far each filter moves the truth itself (a frame with no noise left to remove)
  e_raw, e_plain, e_guided    the noisy frame, raw and after each filter, per seed; s = the relative spread of e_plain across the seeds
COST (--cost): EXACT, S = 4, --passes passes, K = 5, one owner: kajo_hip_denoise with and without the flag on the same handle in the same
run, alternating, the median of --calls calls each with the spread (min .. max) beside it, radiance and ARGB8 both read back as the
tests do -- and the same with planes uploaded in place of the records. Run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel times (the v0 stage is kajo_denoise_guided_v0, the plain filter's kajo_denoise_variance).

    python tools/denoise_guided_report.py [--scene spheres_a169] [--size 320x180] [--passes 16] [--quality] [--cost] [--calls 9] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kajo_amd.renderer import HipRenderer  # noqa: E402
from kajo_amd.scene import Scene  # noqa: E402

SEEDS = (0o715517, 12345, 777, 20240229)


def rmse(img, ref, mask):
    return float(np.sqrt(np.mean((np.clip(img, 0, 1) - np.clip(ref, 0, 1))[mask] ** 2)))


def quality(sc, W, H, passes, say):
    with HipRenderer(sc, W, H, spp=64, exact=True, aov=True, noise=True, seed=12345) as ref:
        ref.render(40)
        truth = ref.radiance()[..., :3] / ref.passes
        plain = ref.denoise()["radiance"][..., :3] / ref.passes
        guided = ref.denoise(noise_guided=True)["radiance"][..., :3] / ref.passes
    fin = np.isfinite(truth).all(-1)
    a, b = rmse(plain, truth, fin), rmse(guided, truth, fin)
    say("quality %dx%d, truth 64 x 40 spp: the truth moves by e_ref_plain %.5f, e_ref_guided %.5f (guided / plain %.3f)" % (W, H, a, b, b / a))
    say("noisy frames: %d passes of S = 4" % passes)
    say("  %-10s %9s %9s %9s %14s %12s" % ("seed", "e_raw", "e_plain", "e_guided", "guided/plain", "measured px"))
    rows = []
    for seed in SEEDS:
        with HipRenderer(sc, W, H, spp=4, exact=True, aov=True, noise=True, seed=seed) as r:
            r.render(passes)
            raw = r.radiance()[..., :3] / r.passes
            plain = r.denoise()["radiance"][..., :3] / r.passes
            guided = r.denoise(noise_guided=True)["radiance"][..., :3] / r.passes
            nz = r.noise()
        mask = fin & np.isfinite(raw).all(-1)
        row = (rmse(raw, truth, mask), rmse(plain, truth, mask), rmse(guided, truth, mask))
        rows.append(row)
        say("  %-10d %9.5f %9.5f %9.5f %14.3f %12d" % ((seed,) + row + (row[2] / row[1], int(((nz["stderr"] >= 0) & (nz["mean"] > 0)).sum()))))
    e = np.array(rows)
    s = (e[:, 1].max() - e[:, 1].min()) / e[:, 1].mean()
    say("  mean       %9.5f %9.5f %9.5f %14.3f;  s = (max - min) / mean of e_plain = %.4f" %
        (e[:, 0].mean(), e[:, 1].mean(), e[:, 2].mean(), e[:, 2].mean() / e[:, 1].mean(), s))


def cost(sc, W, H, passes, calls, say):
    with HipRenderer(sc, W, H, spp=4, exact=True, aov=True, noise=True) as r:
        r.render(passes).wait()
        nz = r.noise()

        def timed(**kw):
            t0 = time.perf_counter()
            r.denoise(iterations=5, **kw)
            return (time.perf_counter() - t0) * 1e3

        def series(label):
            timed(), timed(noise_guided=True)  # (the scratch is allocated, the code objects are loaded)
            t = {False: [], True: []}
            for _ in range(calls):
                for flag in (False, True):
                    t[flag].append(timed(noise_guided=flag))
            med = {k: float(np.median(v)) for k, v in t.items()}
            for flag in (False, True):
                say("  %-28s median %8.3f ms  (min %8.3f, max %8.3f; %d calls)" %
                    (("guided, " + label) if flag else "plain", med[flag], min(t[flag]), max(t[flag]), calls))
            say("  guided / plain = %.3f" % (med[True] / med[False]))

        say("cost %dx%d, K = 5, EXACT, S = 4, %d passes, one owner: kajo_hip_denoise with the read-back of radiance and ARGB8, host wall time" %
            (W, H, passes))
        series("own records")
        r.denoise_guide_planes(nz["mean"], nz["stderr"])
        series("uploaded planes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="spheres_a169")
    ap.add_argument("--size", default="320x180")
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    sc = Scene.from_npz(z, args.scene + "/", args.scene)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("tools/denoise_guided_report.py --scene %s --size %dx%d --passes %d" % (args.scene, W, H, args.passes))
    if args.quality or not args.cost:
        quality(sc, W, H, args.passes, say)
    if args.cost:
        cost(sc, W, H, args.passes, max(args.calls, 7), say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
