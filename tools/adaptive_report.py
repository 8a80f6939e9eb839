"""Adaptive sampling (KAJO_FLAG_ADAPTIVE) as a render proceeds, and what it costs.

    python tools/adaptive_report.py [--scene spheres|caustics] [--size 1920x1080] [--target E|median|quartile] [--passes N] [--spp S]
    python tools/adaptive_report.py --cost [--targets median,quartile] > profiles/r1y_adaptive.txt

A target may be a number or taken from the scene's own estimate, as the tests take theirs: `median` and `quartile` are the median and the
upper quartile of the units' worst relative error at pass 16 (from a KAJO_FLAG_NOISE handle), so that about half and about three
quarters of the units retire at the first decision.

Default mode: one EXACT handle with the rule; after every 16 passes the active share of the units and pixels, the camera paths traced
against the nominal count, and the 95 % quantile of the noise map. Under `rocprofv3 --kernel-trace --stats -- python
tools/adaptive_report.py --target median --passes 64` it is the run that gives the kernels' own times.

--cost, on one GPU at 1920x1080, spheres.json, EXACT; every time is the wall time of four kajo_hip_render(4) calls and a wait, 16 passes:
  a) the stall of a decision: a KAJO_FLAG_NOISE handle against an adaptive handle whose target nothing meets (one decision per 16
     passes, no step kernel), seven steps each, with their spread; the noise handle's render-kernel time of a warmed step is the
     whole-frame reference of b);
  b) for each target: an adaptive run until no unit is active or --passes; per step the active share of the pixels, the wall time, the
     render-kernel time and that time over the whole-frame reference -- expected to follow the active share of the frame's block cost.
     Then q, the 95 % quantile of its final noise map, and the parent's rule: a KAJO_FLAG_NOISE handle rendered in the same steps until
     its 95 % quantile is <= q. Only the render steps are timed in both runs; the noise maps and states looked at between them are not."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kajo_amd.renderer import HipRenderer  # noqa: E402
from kajo_amd.scene import Scene  # noqa: E402
from kajo_amd.tiles import TileLayout  # noqa: E402


def load(name):
    """spheres.json or caustics.json at 16:9, as the tests' fixture holds them"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    key = "caustics_a169" if name == "caustics" else "spheres_a169"
    return Scene.from_npz(z, key + "/", key)


def q95(r):
    return r.noise(quantile=0.95)["quantile_value"]


def scene_targets(sc, W, H, spp):
    """the median and the upper quartile of the units' worst relative error at pass 16"""
    with HipRenderer(sc, W, H, spp=spp, exact=True, noise=True, adaptive=True) as r:
        slots = r.adapt_state()["unitSlots"]
        rel = r.render(16).noise()["relative"]
    ys, xs = np.mgrid[0:H, 0:W]
    _, slot = TileLayout(W, H, 1).owner_and_slot(xs, ys)
    unit = (slot // slots).ravel()
    worst = np.full(unit.max() + 1, -np.inf)
    np.maximum.at(worst, unit, rel.ravel().astype(np.float64))
    worst = worst[np.isfinite(worst)]
    return {"median": float(np.float32(np.quantile(worst, 0.5))), "quartile": float(np.float32(np.quantile(worst, 0.75)))}


def resolve_targets(names, sc, W, H, spp):
    auto = scene_targets(sc, W, H, spp) if any(n in ("median", "quartile") for n in names) else {}
    return [(n, auto[n] if n in auto else float(n)) for n in names]


def progress(sc, W, H, spp, target, passes):
    with HipRenderer(sc, W, H, spp=spp, exact=True, noise=True, adaptive=dict(target=target)) as r:
        n2 = r.n * r.n
        print("target %.6g" % target)
        print("pass  active units  active px  paths traced / nominal   q95(rel)")
        while r.passes < passes:
            for _ in range(4):
                r.render(4)
            r.wait()
            s = r.adapt_state()
            print("%4d  %5.1f %%       %5.1f %%    %6.2f %%                %.4g" % (
                r.passes, 100.0 * s["activeUnits"] / max(s["units"], 1), 100.0 * s["activePixels"] / max(s["pixels"], 1),
                100.0 * s["paths"] / (s["pixels"] * n2 * r.passes), q95(r)))
            if s["activeUnits"] == 0:
                break


def step(r):
    """16 passes as four calls and a wait -> (wall ms, render-kernel ms)"""
    k0 = r.counters()["kernelMs"]
    t = time.perf_counter()
    for _ in range(4):
        r.render(4)
    r.wait()
    wall = (time.perf_counter() - t) * 1e3
    return wall, r.counters()["kernelMs"] - k0


def spread(v):
    return "median %.3f, min %.3f, max %.3f" % (np.median(v), min(v), max(v))


def cost(sc, W, H, spp, targets, limit):
    print("# adaptive sampling: cost at %dx%d, EXACT, spp %d, one GPU; a step is 16 passes as 4 x render(4) and a wait" % (W, H, spp))
    with HipRenderer(sc, W, H, spp=spp, exact=True, noise=True) as twin:
        step(twin)
        base = [step(twin) for _ in range(7)]
    with HipRenderer(sc, W, H, spp=spp, exact=True, noise=True, adaptive=dict(target=1e-30)) as r:
        step(r)
        unmet = [step(r) for _ in range(7)]
    bw, uw = [b[0] for b in base], [u[0] for u in unmet]
    whole = float(np.median([b[1] for b in base]))
    print("a) wall ms of a step over 7: noise handle %s; adaptive handle, target unmet (one decision, no step kernel) %s" % (spread(bw), spread(uw)))
    d = np.median(uw) - np.median(bw)
    print("   difference of the medians %+.3f ms; the seven steps of one handle spread over %.3f ms: the stall of a decision is %s"
          % (d, max(max(bw) - min(bw), max(uw) - min(uw)), "below the spread" if abs(d) <= max(max(bw) - min(bw), max(uw) - min(uw)) else "above the spread"))
    print("   whole-frame reference: render-kernel ms of a warmed step of the noise handle, median %.3f" % whole)
    for i, (name, E) in enumerate(targets):
        print("b%d) target %s = %.6g" % (i + 1, name, E))
        with HipRenderer(sc, W, H, spp=spp, exact=True, noise=True, adaptive=dict(target=E)) as r:
            n2 = r.n * r.n
            total = 0.0
            print("   pass  active px   step wall ms  render-kernel ms  kernel ms / whole-frame reference")
            while r.passes < limit:
                s = r.adapt_state()
                share = s["activePixels"] / s["pixels"]
                wall, k = step(r)
                total += wall
                note = "  (the first step: cold start and the blocks' cost measurement)" if r.passes == 16 else ""
                print("   %4d  %6.2f %%   %9.3f      %9.3f         %.3f%s" % (r.passes, 100 * share, wall, k, k / whole, note))
                if r.adapt_state()["activeUnits"] == 0:
                    break
            s = r.adapt_state()
            q = q95(r)
            adaptive_passes = r.passes
            print("   adaptive: %d passes, %.1f ms in render steps, %.4g G camera paths traced (nominal %.4g G), q95 of the final map %.4g, active units %d / %d"
                  % (r.passes, total, s["paths"] / 1e9, s["pixels"] * n2 * r.passes / 1e9, q, s["activeUnits"], s["units"]))
        with HipRenderer(sc, W, H, spp=spp, exact=True, noise=True) as u:
            total = 0.0
            while u.passes < 4 * max(limit, adaptive_passes):
                total += step(u)[0]
                if q95(u) <= q:
                    break
            print("   uniform until q95 <= %.4g: %d passes, %.1f ms in render steps, %.4g G camera paths, q95 %.4g"
                  % (q, u.passes, total, W * H * n2 * u.passes / 1e9, q95(u)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("spheres", "caustics"), default="spheres")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--target", default="median")
    ap.add_argument("--targets", default="median,quartile")
    ap.add_argument("--passes", type=int, default=128)
    ap.add_argument("--cost", action="store_true")
    a = ap.parse_args()
    W, H = map(int, a.size.split("x"))
    sc = load(a.scene)
    if a.cost:
        cost(sc, W, H, a.spp, resolve_targets(a.targets.split(","), sc, W, H, a.spp), a.passes)
    else:
        progress(sc, W, H, a.spp, resolve_targets([a.target], sc, W, H, a.spp)[0][1], a.passes)


if __name__ == "__main__":
    main()
