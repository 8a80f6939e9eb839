"""The definition of KAJO_FLAG_AOV_SPECULAR (include/kajo_hip.h, under kajo_hip_read_aov) replayed one sample at a time in numpy. TEST
INFRASTRUCTURE ONLY, shared by tests/test_aov_specular_cpu.py (which pins it against the first-hit replay) and
tests/test_hip_aov_specular.py (which holds the STRICT and EXACT kernels to it bit for bit).

Built from three oracle calls and nothing else: oraclelib.camera_ray (the camera ray of a sample), Handle.trace (closest hit: object,
t, position, normal) and Handle.sample with kind 2 (ideal reflector) or 3 (ideal transmission), of which only `hit` and `dir` are read
-- no random number is drawn by either lobe. Everything else -- the coins pT and pD, the throughput, the chain's length, the extension
ray's origin and the two float4 sums -- is float32 numpy arithmetic in the order the header states."""
import numpy as np

from oraclelib import OracleLib, camera_ray

MAX_FOLLOW = 8  # KAJO_AOV_MAX_FOLLOW
F = np.float32
_RAYS = {}


def camera_rays(o, sc, w, h, spp, npass, seed):
    """(O, D) of every pixel's samples of one pass: (n * n, h * w, 3) each. The rays depend on the camera alone: cached by it."""
    key = (sc.view.tobytes(), sc.proj.tobytes(), w, h, spp, npass, seed)
    if key not in _RAYS:
        n = int(np.sqrt(float(spp)))
        O = np.empty((n * n, h * w, 3), F)
        D = np.empty((n * n, h * w, 3), F)
        for s in range(n * n):
            for y in range(h):
                for x in range(w):
                    O[s, y * w + x], D[s, y * w + x], _ = camera_ray(o, w, h, spp, x, y, s, npass=npass, seed=seed)
        if len(_RAYS) > 64:
            _RAYS.clear()
        _RAYS[key] = (O, D)
    return _RAYS[key]


def material_tables(sc):
    """Per object id - 1 (planes first): the lobe to follow (0 none, 2 ideal reflector, 3 ideal transmission), the clamped specular
    colour, the refractive index and the first-hit albedo."""
    mats = np.concatenate([sc.planes[:, 16:38], sc.spheres[:, 16:38]]).astype(F)
    diffuse, specular, transparency = mats[:, 4:7], mats[:, 8:11], mats[:, 16:19]
    exponent, ior = mats[:, 20], mats[:, 21]
    with np.errstate(invalid="ignore", divide="ignore"):
        tD = (diffuse[:, 0] + diffuse[:, 1]) + diffuse[:, 2]
        tS = (specular[:, 0] + specular[:, 1]) + specular[:, 2]
        tT = (transparency[:, 0] + transparency[:, 1]) + transparency[:, 2]
        pT = tT / ((tD + tS) + tT)
        pD = tD / (tD + tS)
        # (comparisons with NaN are false)
        lobe = np.where(pT >= F(0.5), 3, np.where((exponent == 0) & (pD < F(0.5)), 2, 0))
    tint = np.minimum(np.maximum(specular, F(0)), F(1))
    albedo = np.minimum(np.maximum((diffuse + specular) + transparency, F(0)), F(1))
    return lobe, tint, ior, albedo


def replay_specular(sc, passes, w, h, spp, seed, rays_of=None):
    """(A, B, stats) for the passes numbered `passes`: the two (h, w, 4) float32 sums and stats = dict(samples, followed (samples with
    at least one follow), follows (all of them), longest, capped (samples that used all MAX_FOLLOW), followed_per_pixel (h, w))."""
    o = OracleLib("oracle").create(sc, 1)
    n = int(np.sqrt(float(spp)))
    lobe, tint, ior, albedo_of = material_tables(sc)
    bg = sc.background[:3].astype(F)
    eps = F(1e-3)
    zero_state = np.zeros((1, 2), np.uint64)
    A = np.zeros((h * w, 4), F)
    B = np.zeros((h * w, 4), F)
    stats = dict(samples=0, followed=0, follows=0, longest=0, capped=0, followed_per_pixel=np.zeros(h * w, np.int64))
    for p in passes:
        Os, Ds = camera_rays(o, sc, w, h, spp, p, seed)
        for s in range(n * n):
            O, D = Os[s].copy(), Ds[s].copy()
            T = np.ones((h * w, 3), F)
            dist = np.zeros(h * w, F)
            follows = np.zeros(h * w, np.int64)
            t = o.trace(O, D)
            idx, tt, normal = t["idx"].copy(), t["t"].copy(), t["normal"].copy()
            position = t["position"].copy()
            chain = np.ones(h * w, bool)
            for _ in range(MAX_FOLLOW):
                want = np.where(chain & (idx != 0), lobe[np.maximum(idx, 1) - 1], 0)
                chain = np.zeros(h * w, bool)
                nd = np.zeros((h * w, 3), F)
                for obj in np.unique(idx[want != 0]):  # (one call per material: the refractive index is a parameter of the call)
                    sel = np.flatnonzero((idx == obj) & (want != 0))
                    r = o.sample(int(lobe[obj - 1]), O[sel], D[sel], np.repeat(zero_state, sel.size, 0), tint[obj - 1].tolist() + [1.0],
                                 param=float(ior[obj - 1]))
                    assert np.array_equal(r["hit"], idx[sel])  # (sample() walks the same ray to the same object)
                    nd[sel] = r["dir"]
                    chain[sel] = (r["dir"] != 0).any(-1)
                if not chain.any():
                    break
                f = np.flatnonzero(chain)
                T[f] = T[f] * tint[idx[f] - 1]
                dist[f] = dist[f] + tt[f]
                O[f] = position[f] + nd[f] * eps
                D[f] = nd[f]
                follows[f] += 1
                t = o.trace(O[f], D[f])
                idx[f], tt[f], normal[f], position[f] = t["idx"], t["t"], t["normal"], t["position"]
            hit = idx != 0
            albedo = (T * np.where(hit[:, None], albedo_of[np.maximum(idx, 1) - 1], bg[None, :])).astype(F)
            nrm = np.where(hit[:, None], normal, F(0)).astype(F)
            depth = np.where(hit, dist + tt, F(0)).astype(F)
            # one float32 addition per word and sample, in pass and stratum order
            A[:, :3] += albedo
            A[:, 3] += hit.astype(F)
            B[:, :3] += nrm
            B[:, 3] += depth
            stats["samples"] += h * w
            stats["followed"] += int((follows > 0).sum())
            stats["follows"] += int(follows.sum())
            stats["longest"] = max(stats["longest"], int(follows.max()))
            stats["capped"] += int((follows == MAX_FOLLOW).sum())
            stats["followed_per_pixel"] += follows > 0
    stats["followed_per_pixel"] = stats["followed_per_pixel"].reshape(h, w)
    return A.reshape(h, w, 4), B.reshape(h, w, 4), stats


def describe(stats):
    s = stats["samples"]
    return ("%.1f %% of the pixels have a followed sample, %.1f %% of the samples are followed, %.3f follows per sample (%.3f walks), "
            "longest chain %d follows, %.3f %% of the samples reach the cap" %
            (100.0 * (stats["followed_per_pixel"] > 0).mean(), 100.0 * stats["followed"] / s, stats["follows"] / s, 1 + stats["follows"] / s,
             stats["longest"], 100.0 * stats["capped"] / s))


def with_delta_balls(sc, every=7, first=0):
    """`sc` with some of its non-emissive spheres turned into glass and ideal mirrors (every `every`-th one, alternately), by editing the
    22-float material image of their records: glass = spheres.json's (specular .1, transparency #eef-like, ior 2 -> pT 0.9); mirror =
    specular .67, exponent 0, no diffuse. Same geometry, so the scene's class (grid, visibility lists) is unchanged."""
    from kajo_amd.scene import Scene, material
    sp = sc.spheres.copy()
    plain = np.flatnonzero(~np.any(sp[:, 16 + 12:16 + 16] != 0, axis=1))
    for k, i in enumerate(plain[first::every]):
        if k % 2 == 0:
            sp[i, 16:38] = material(specular=[.1, .1, .1], transparency=[.85, .85, .95], ior=2.0)
        else:
            sp[i, 16:38] = material(specular=[.67, .67, .67], exponent=0.0)
    return Scene(sc.background, sc.view, sc.proj, sp, sc.planes, sc.name + "_delta")


def without_delta(sc):
    """`sc` with every material the rule would follow made diffuse (planes and spheres): the chain never starts."""
    from kajo_amd.scene import Scene, material
    lobe = material_tables(sc)[0]
    pl, sp = sc.planes.copy(), sc.spheres.copy()
    for i in np.flatnonzero(lobe):
        rec = pl[i] if i < len(pl) else sp[i - len(pl)]
        rec[16:38] = material(diffuse=[.5, .4, .3])
    return Scene(sc.background, sc.view, sc.proj, sp, pl, sc.name + "_nodelta")
