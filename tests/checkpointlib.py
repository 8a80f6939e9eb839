"""A restatement in numpy of what include/kajo_hip.h says about checkpoints ("Checkpoints"): the digest, the canonical order and the
layout of a section. Written from the header's words, not from checkpoint_math.h's lines; tests/test_checkpoint_cpu.py and
tests/test_hip_checkpoint.py hold the library against it."""
import struct

import numpy as np

from kajo_amd.tiles import TileLayout

MASK = (1 << 64) - 1
KIND_WORDS = {1: 4, 2: 8, 3: 8, 4: 16, 5: 4, 6: 8, 7: 0, 8: 0}
SUM, CARRY, AOV, MATTE, NOISE_BASE, NOISE_MOMENTS, ADAPT, COUNTERS = range(1, 9)
HEADER = struct.Struct("<8sII6iI3iQQQqiiQ")  # KajoCheckpointHeader, 104 bytes
PLANE = struct.Struct("<IIQQQ")  # KajoCheckpointPlane, 32 bytes
TRAILER = struct.Struct("<dQ")
assert HEADER.size == 104 and PLANE.size == 32 and TRAILER.size == 16


def mix(k):
    """the splitmix64 finaliser over uint64 arrays"""
    with np.errstate(over="ignore"):
        k = k + np.uint64(0x9E3779B97F4A7C15)
        k = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        k = (k ^ (k >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return k ^ (k >> np.uint64(31))


def digest(p, words):
    """p: (n,) global pixel indices y * W + x; words: (n, w) uint32 -> the plane's digest"""
    words = np.ascontiguousarray(words, np.uint32)
    n, w = words.shape
    if n == 0:
        return 0
    with np.errstate(over="ignore"):
        key = np.asarray(p, np.uint64)[:, None] * np.uint64(w) + np.arange(w, dtype=np.uint64)[None, :]
        terms = mix(mix(key) ^ words.astype(np.uint64))
        return int(np.add.reduce(terms.ravel(), dtype=np.uint64))


def digest_words(words):
    """a block that is not per pixel: word i counts as pixel i of one word"""
    words = np.ascontiguousarray(words, np.uint32).ravel()
    return digest(np.arange(words.size), words[:, None])


def owned(W, H, world, rank, tile=(64, 16)):
    """the global indices y * W + x of the owner's pixels in canonical order: y ascending, then x"""
    ys, xs = np.mgrid[0:H, 0:W]
    owner, _ = TileLayout(W, H, world, tile).owner_and_slot(xs, ys)
    return np.flatnonzero(owner.ravel() == rank)


def align(v):
    return (v + 15) & ~15


def section(W, H, planes, tile=(64, 16), index=0, count=1, flags=0, S=4, depth=8, passes=6, seed=7, fingerprint=0x1234, aov_passes=0,
            noise_rebase=0, kernel_ms=0.0, launches=0, magic=b"KAJOCKPT", version=1):
    """A section by hand. planes: {kind: (pixels, w) uint32 for a per-pixel kind, (words,) uint32 for ADAPT / COUNTERS}."""
    p = owned(W, H, count, index, tile)
    kinds = sorted(planes)
    table, at = [], align(HEADER.size + PLANE.size * len(kinds))
    for k in kinds:
        words = np.ascontiguousarray(planes[k], np.uint32)
        w = KIND_WORDS[k]
        d = digest(p, words.reshape(p.size, w)) if w else digest_words(words)
        table.append((k, w, at, words.nbytes, d, words.tobytes()))
        at = align(at + words.nbytes)
    total = at + TRAILER.size
    blob = bytearray(total)
    blob[:HEADER.size] = HEADER.pack(magic, version, len(kinds), W, H, tile[0], tile[1], index, count, flags, S, depth, passes, seed, fingerprint,
                                     p.size, aov_passes, noise_rebase, 0, total)
    for i, (k, w, off, nbytes, d, raw) in enumerate(table):
        blob[HEADER.size + i * PLANE.size:HEADER.size + (i + 1) * PLANE.size] = PLANE.pack(k, w, off, nbytes, d)
        blob[off:off + nbytes] = raw
    blob[at:] = TRAILER.pack(kernel_ms, launches)
    return bytes(blob)


def parse(blob):
    """header fields, the planes {kind: (offset, bytes, digest, uint32 words)} and the trailer of a section the library wrote"""
    f = HEADER.unpack_from(blob, 0)
    names = ("magic", "version", "nPlanes", "width", "height", "tileW", "tileH", "tileIndex", "tileCount", "flags", "samplesPerPass", "depthLimit",
             "passesDone", "seed", "fingerprint", "pixels", "aovPasses", "noiseRebase", "reserved", "bytes")
    h = dict(zip(names, f))
    planes = {}
    for i in range(h["nPlanes"]):
        k, w, off, nbytes, d = PLANE.unpack_from(blob, HEADER.size + i * PLANE.size)
        words = np.frombuffer(blob, np.uint32, nbytes // 4, off)
        planes[k] = dict(offset=off, bytes=nbytes, digest=d, wordsPerPixel=w, words=words.reshape(-1, w) if w else words)
    h["planes"] = planes
    h["kernelMs"], h["launches"] = TRAILER.unpack_from(blob, len(blob) - TRAILER.size)
    return h


def body(blob):
    """the section without its trailer: a function of (scene, parameters, passes)"""
    return bytes(blob)[:-TRAILER.size]
