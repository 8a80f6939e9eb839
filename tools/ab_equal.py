#!/usr/bin/env python3
"""Do two builds of the library render the same FAST (or STRICT, or EXACT) buffers, bit for bit? Each library in a child process of its own
(it is chosen at import, KAJO_HIP_LIB), frames of spheres.json, the caustics scene and test.json kept as .npy under /tmp and compared.
usage: ab_equal.py libA.so libB.so [fast|strict|exact]"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (scene, W, H, S, passes, depth, passes per launch, the render calls: (passes, wait)). The last case launches the default 16 passes at a
# time: the wait after the first launch records the block order, and the second launch renders its tail in parts (FAST / EXACT).
CASES = [("spheres_a169", 1280, 720, 32, 4, 8, 2, [(4, False)]), ("caustics_a169", 960, 540, 32, 4, 8, 2, [(4, False)]),
         ("test_a1", 512, 512, 16, 3, 8, 2, [(3, False)]), ("spheres_a1", 256, 256, 16, 1, 1, 2, [(1, False)]),
         ("dialect_a1", 400, 300, 9, 2, 5, 2, [(2, False)]), ("spheres_a169", 1920, 1080, 32, 32, 8, 0, [(16, True), (16, False)])]


def child(tag, mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    from kajo_amd.renderer import HipRenderer
    from kajo_amd.scene import Scene
    z = np.load(os.path.join(ROOT, "tests/golden/scenes.npz"))
    for i, (key, W, H, S, passes, depth, per_launch, calls) in enumerate(CASES):
        with HipRenderer(Scene.from_npz(z, key + "/", key), W, H, spp=S, depth_limit=depth, strict=(mode == "strict"), exact=(mode == "exact"),
                         passes_per_launch=per_launch) as r:
            for n, wait in calls:
                r.render(n, wait=wait)
            print("%s %s %s: last launch rendered %d tail workgroups" % (tag, mode, key, r.counters()["tailGroups"]), flush=True)
            np.save("/tmp/ab_%s_%d.npy" % (tag, i), r.radiance())


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    import numpy as np
    a, b = sys.argv[1], sys.argv[2]
    mode = sys.argv[3] if len(sys.argv) > 3 else "fast"
    for tag, lib in (("a", a), ("b", b)):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tag, mode], env=dict(os.environ, KAJO_HIP_LIB=os.path.abspath(lib)), check=True)
    for i, (key, W, H, S, passes, depth, per_launch, calls) in enumerate(CASES):
        x, y = np.load("/tmp/ab_a_%d.npy" % i)[..., :3], np.load("/tmp/ab_b_%d.npy" % i)[..., :3]
        same = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        d = np.abs(x - y)
        print("%s %-14s %4dx%-4d S=%d x%d: %d of %d px differ%s" % (mode, key, W, H, S, passes, int((~same).any(-1).sum()), W * H,
              "" if same.all() else "; max |d| %.3g, median of the differing %.3g" % (float(np.nanmax(d)), float(np.nanmedian(d[~same])))), flush=True)
