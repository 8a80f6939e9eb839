"""The definition of KAJO_FLAG_AOV_MATTE (include/kajo_hip.h, at kajo_hip_read_matte) restated in numpy. TEST INFRASTRUCTURE ONLY, shared
by tests/test_matte_cpu.py and tests/test_hip_matte.py.

The ids come from the oracle and nothing else: Handle.trace over the replayed camera rays (aov_specular_replay.camera_rays), and for
KAJO_FLAG_AOV_SPECULAR the chain of aov_specular_replay.replay_specular walked once more with the same three oracle calls, keeping the
FINAL hit's id (test_hip_matte.py checks the walk against replay_specular's own hit counts). The tables, the first-come rule, the rank
order and the mask are integer numpy in the order the header states."""
import numpy as np

from oraclelib import OracleLib

from aov_specular_replay import MAX_FOLLOW, camera_rays, material_tables

SLOTS = 8  # KAJO_MATTE_SLOTS
F = np.float32
_IDS = {}


def sample_ids(sc, passes, w, h, spp, seed, specular=False):
    """The object id of every AOV sample in the order the tables take them: (len(passes) * n * n, h * w) int32, pass order then stratum
    sy * n + sx. specular: the final hit of the chain of KAJO_FLAG_AOV_SPECULAR instead of the first hit."""
    key = (sc.name, sc.n_spheres, sc.n_planes, sc.spheres.tobytes(), sc.planes.tobytes(), tuple(passes), w, h, spp, seed, specular)
    if key in _IDS:
        return _IDS[key]
    o = OracleLib("oracle").create(sc, 1)
    n = int(np.sqrt(float(spp)))
    lobe, tint, ior, _ = material_tables(sc)
    eps = F(1e-3)
    zero_state = np.zeros((1, 2), np.uint64)
    out = []
    for p in passes:
        Os, Ds = camera_rays(o, sc, w, h, spp, p, seed)
        for s in range(n * n):
            O, D = Os[s].copy(), Ds[s].copy()
            t = o.trace(O, D)
            idx, position = t["idx"].copy(), t["position"].copy()
            chain = np.ones(h * w, bool)
            for _ in range(MAX_FOLLOW if specular else 0):
                want = np.where(chain & (idx != 0), lobe[np.maximum(idx, 1) - 1], 0)
                chain = np.zeros(h * w, bool)
                nd = np.zeros((h * w, 3), F)
                for obj in np.unique(idx[want != 0]):
                    sel = np.flatnonzero((idx == obj) & (want != 0))
                    r = o.sample(int(lobe[obj - 1]), O[sel], D[sel], np.repeat(zero_state, sel.size, 0), tint[obj - 1].tolist() + [1.0],
                                 param=float(ior[obj - 1]))
                    nd[sel] = r["dir"]
                    chain[sel] = (r["dir"] != 0).any(-1)
                if not chain.any():
                    break
                f = np.flatnonzero(chain)
                O[f] = position[f] + nd[f] * eps
                D[f] = nd[f]
                t = o.trace(O[f], D[f])
                idx[f], position[f] = t["idx"], t["position"]
            out.append(idx.astype(np.int32))
    if len(_IDS) > 64:
        _IDS.clear()
    _IDS[key] = np.stack(out)
    return _IDS[key]


def tables(ids):
    """The first-come tables after the samples `ids` (samples, pixels): (slot ids (pixels, 8) int64 -- -1 where empty, counts (pixels, 8)
    int64, dropped (pixels) int64), slots in the order they were taken."""
    npix = ids.shape[1]
    slot = -np.ones((npix, SLOTS), np.int64)
    count = np.zeros((npix, SLOTS), np.int64)
    dropped = np.zeros(npix, np.int64)
    rows = np.arange(npix)
    for sample in ids:
        holds = (count > 0) & (slot == sample[:, None])
        has = holds.any(1)
        k = holds.argmax(1)
        count[rows[has], k[has]] += 1
        empty = count == 0
        room = ~has & empty.any(1)
        k = empty.argmax(1)  # the first empty slot
        slot[rows[room], k[room]] = sample[room]
        count[rows[room], k[room]] = 1
        dropped += ~has & ~room
    return slot, count, dropped


def ranked(slot, count):
    """kajo_hip_read_matte's order of a pixel's slots: count descending, ties by id ascending, empty slots last as (-1, 0)
    -> (ids int32, counts uint32), both (pixels, 8)."""
    ids = np.where(count > 0, slot, -1)
    # (lexsort: last key first; the empties' key puts them behind every slot that holds something)
    order = np.lexsort((ids.T, -count.T, (count == 0).T), axis=0).T
    return np.take_along_axis(ids, order, 1).astype(np.int32), np.take_along_axis(count, order, 1).astype(np.uint32)


def restate(sc, passes, w, h, spp, seed, specular=False):
    """dict(ids (h, w, 8) int32, counts (h, w, 8) uint32, dropped (h, w) int64, samples, distinct (h, w): ids seen per pixel, sample_ids)."""
    seq = sample_ids(sc, passes, w, h, spp, seed, specular)
    slot, count, dropped = tables(seq)
    ids, counts = ranked(slot, count)
    distinct = np.array([np.unique(seq[:, i]).size for i in range(w * h)])
    return dict(ids=ids.reshape(h, w, SLOTS), counts=counts.reshape(h, w, SLOTS), dropped=dropped.reshape(h, w), samples=seq.shape[0],
                distinct=distinct.reshape(h, w), sample_ids=seq)


def mask_of(ids, counts, samples, objects):
    """kajo_hip_matte_mask's mask from ranked tables: float32(sum of the selected slots' counts) / float32(samples), 0 with no sample."""
    selected = np.isin(ids, np.asarray(list(objects), np.int64)) & (counts > 0)
    total = np.where(selected, counts, 0).sum(-1, dtype=np.uint32)
    if samples == 0:
        return np.zeros(total.shape, F)
    return total.astype(F) / F(samples)
