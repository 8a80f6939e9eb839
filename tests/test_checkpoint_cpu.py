"""Checkpoints (include/kajo_hip.h "Checkpoints") without a GPU: the canonical order against kajo_amd/tiles.py, the digest against a numpy
restatement (tests/checkpointlib.py), kajo_hip_checkpoint_info and kajo_hip_checkpoint_merge over sections crafted by hand with every
refusal, the same host code as a stand-alone program under AddressSanitizer + UBSan (tools/checkpoint_san.cpp: no Python in that process),
what the compiler made of the kernels of kajo_amd/csrc/checkpoint_kernels.cpp (nothing spilled, no scratch, no FLAT instruction, no atomic), and
the entry points and struct sizes as the header and the binding declare them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import checkpointlib as ck
import devicecode
from kajo_amd import capi
from kajo_amd.renderer import checkpoint_info, checkpoint_merge
from kajo_amd.tiles import TileLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")
KERNELS = ("kajo_ckpt_pack", "kajo_ckpt_unpack", "kajo_ckpt_digest", "kajo_ckpt_digest_sum")
FRAMES = [(1, 1), (7, 5), (41, 23), (65, 9), (130, 40)]
TILES = [(64, 16), (16, 16)]
WORLDS = [1, 2, 3, 8]


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("ckpt_san")
    exe = str(d / "checkpoint_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tools", "checkpoint_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(*args):
        p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert p.returncode == 0, "checkpoint_san %s -> %d\n%s\n%s" % (" ".join(map(str, args)), p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        return p.stdout

    run.dir = d
    return run


# ---- the canonical order ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("frame", FRAMES)
def test_rank_is_row_major_order_of_the_owners_pixels(san, frame, tile):
    W, H = frame
    ys, xs = np.mgrid[0:H, 0:W]
    for world in WORLDS:
        out = san.dir / ("rank_%dx%d_%d_%d.bin" % (W, H, tile[0], world))
        san("rank", W, H, tile[0], tile[1], world, out)  # (it holds the inverse and the slot map against kajoTileSlot itself)
        got = np.fromfile(out, np.int32).reshape(world, H, W)
        owner, _ = TileLayout(W, H, world, tile).owner_and_slot(xs, ys)
        for rank in range(world):
            want = np.full(W * H, -1, np.int32)
            mine = np.flatnonzero(owner.ravel() == rank)
            want[mine] = np.arange(mine.size)
            assert np.array_equal(got[rank].ravel(), want), (frame, tile, world, rank)


# ---- the digest -------------------------------------------------------------------------------------------------------------------------

def _planes(rng, pixels, kinds):
    return {k: rng.integers(0, 2 ** 32, (pixels, ck.KIND_WORDS[k]), dtype=np.uint64).astype(np.uint32) for k in kinds}


def test_mix_is_the_splitmix64_finaliser():
    # splitmix64 seeded with 0: its first outputs are mix(0), mix(golden), mix(2 * golden) (Steele, Lea, Flood 2014; Vigna's splitmix64.c)
    g = 0x9E3779B97F4A7C15
    got = [int(v) for v in ck.mix(np.array([0, g, 2 * g & ck.MASK], np.uint64))]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


@pytest.mark.parametrize("kinds", [(ck.SUM,), (ck.SUM, ck.CARRY, ck.AOV, ck.MATTE, ck.NOISE_BASE, ck.NOISE_MOMENTS)])
def test_info_recomputes_the_digests_of_random_words(kinds):
    rng = np.random.default_rng(11)
    W, H = 41, 23
    blob = ck.section(W, H, _planes(rng, W * H, kinds), flags=capi.KAJO_FLAG_EXACT, kernel_ms=2.5, launches=3)
    info = checkpoint_info(blob)  # (accepts only where its own digests are the restatement's)
    assert (info["width"], info["height"], info["pixels"], info["passesDone"], info["kernelMs"], info["launches"]) == (W, H, W * H, 6, 2.5, 3)
    assert [p["kind"] for p in info["planes"]] == list(kinds)
    assert [p["digest"] for p in info["planes"]] == [ck.parse(blob)["planes"][k]["digest"] for k in kinds]


def test_digests_add_over_owners():
    rng = np.random.default_rng(5)
    W, H, world = 130, 40, 3
    whole = rng.integers(0, 2 ** 32, (W * H, 8), dtype=np.uint64).astype(np.uint32)
    total = ck.digest(np.arange(W * H), whole)
    parts = 0
    for rank in range(world):
        p = ck.owned(W, H, world, rank)
        blob = ck.section(W, H, {ck.SUM: whole[p, :4], ck.AOV: whole[p]}, index=rank, count=world)
        info = checkpoint_info(blob)
        assert info["planes"][1]["digest"] == ck.digest(p, whole[p])
        parts = (parts + info["planes"][1]["digest"]) & ck.MASK
    assert parts == total


# ---- info and merge ---------------------------------------------------------------------------------------------------------------------

def _owners(rng, W=130, H=40, world=3, kinds=(ck.SUM, ck.CARRY, ck.NOISE_MOMENTS), counters=True, tile=(64, 16), **kw):
    whole = _planes(rng, W * H, kinds)
    blobs, total = [], np.zeros(4, np.uint64)
    for rank in range(world):
        p = ck.owned(W, H, world, rank, tile)
        planes = {k: v[p] for k, v in whole.items()}
        if counters:
            c = rng.integers(0, 2 ** 62, 4, dtype=np.uint64)
            total = total + c
            planes[ck.COUNTERS] = c.view(np.uint32)
        blobs.append(ck.section(W, H, planes, tile=tile, index=rank, count=world, kernel_ms=1.0 + rank, launches=rank, **kw))
    if counters:
        whole[ck.COUNTERS] = total.view(np.uint32)
    return blobs, ck.section(W, H, whole, tile=tile, **kw)


def test_merge_of_three_owners_is_the_whole_frame_section_byte_for_byte(san):
    rng = np.random.default_rng(3)
    blobs, whole = _owners(rng)
    merged = checkpoint_merge(blobs)
    assert ck.body(merged) == ck.body(whole)
    assert ck.parse(merged)["kernelMs"] == 6.0 and ck.parse(merged)["launches"] == 3
    info = checkpoint_info(merged)
    assert (info["tileIndex"], info["tileCount"], info["pixels"]) == (0, 1, 130 * 40)
    # any order of the sections; a whole-frame section merges to itself
    assert checkpoint_merge(blobs[::-1]) == merged
    assert ck.body(checkpoint_merge([whole])) == ck.body(whole)
    # ... and the stand-alone program under the sanitizers gives the same file
    paths = []
    for i, b in enumerate(blobs):
        paths.append(san.dir / ("own%d.ckpt" % i))
        paths[-1].write_bytes(b)
    out = san.dir / "merged.ckpt"
    assert san("merge", out, *paths).split()[0] == "ok"
    assert out.read_bytes() == merged
    assert san("info", out, *paths).splitlines() == ["ok 5200 4"] + ["ok %d 4" % ck.owned(130, 40, 3, r).size for r in range(3)]


def test_merge_at_another_tile_shape_and_more_owners_than_tiles():
    rng = np.random.default_rng(4)
    blobs, whole = _owners(rng, W=41, H=23, world=8, tile=(16, 16), kinds=(ck.SUM, ck.AOV, ck.MATTE), counters=False)
    assert ck.body(checkpoint_merge(blobs)) == ck.body(whole)


def _refused(blob, *words):
    with pytest.raises(capi.KajoError) as e:
        checkpoint_info(blob)
    assert e.value.code == capi.KAJO_E_INVALID
    for w in words:
        assert w in str(e.value), str(e.value)
    return str(e.value)


def test_info_refusals(san):
    rng = np.random.default_rng(9)
    W, H = 41, 23
    kinds = (ck.SUM, ck.CARRY, ck.AOV, ck.MATTE, ck.NOISE_BASE, ck.NOISE_MOMENTS)
    planes = _planes(rng, W * H, kinds)
    planes[ck.ADAPT] = np.arange(ck.HEADER.size // 4, dtype=np.uint32)[:20]
    planes[ck.COUNTERS] = np.arange(8, dtype=np.uint32)
    good = ck.section(W, H, planes)
    parsed = ck.parse(good)
    assert len(checkpoint_info(good)["planes"]) == 8
    cases = {"good": good}
    _refused(ck.section(W, H, planes, magic=b"KAJOCKPX"), "magic")
    cases["magic"] = ck.section(W, H, planes, magic=b"KAJOCKPX")
    _refused(ck.section(W, H, planes, version=2), "version")
    # every truncation point of the header and the plane table, then one inside every plane, the trailer, and a byte too many
    table_end = ck.HEADER.size + 8 * ck.PLANE.size
    for cut in range(0, table_end + 1):
        msg = _refused(good[:cut], "truncated")
        assert ("header" in msg) if cut < ck.HEADER.size else ("plane table" in msg) if cut < table_end else ("plane SUM" in msg), (cut, msg)
    # a header that states a frame the blob cannot hold is refused before anything is sized by it
    huge = bytearray(good[:table_end])
    huge[16:24] = ck.struct.pack("<ii", 1, 2 ** 31 - 1)
    huge[72:80] = (2 ** 31 - 1).to_bytes(8, "little")
    _refused(bytes(huge), "truncated")
    huge[32:40] = ck.struct.pack("<ii", 0, 2 ** 28)  # ... nor for an owner of eight pixels of 2^28 tile rows
    huge[72:80] = (8).to_bytes(8, "little")
    _refused(bytes(huge), "tile rows")
    for k, p in parsed["planes"].items():
        _refused(good[:p["offset"] + p["bytes"] - 1], "plane " + capi.KAJO_CKPT_NAMES[k], "truncated")
        cases["cut_%d" % k] = good[:p["offset"] + p["bytes"] - 1]
    _refused(good[:-1], "trailer")
    _refused(good + b"\0", "size")
    # one flipped bit in each plane: named
    for k, p in parsed["planes"].items():
        bad = bytearray(good)
        bad[p["offset"] + p["bytes"] // 2] ^= 0x10
        _refused(bytes(bad), "plane " + capi.KAJO_CKPT_NAMES[k], "digest")
        cases["flip_%d" % k] = bytes(bad)
    # a table that does not describe the planes
    for field, value, word in ((1, 5, "words per pixel"), (2, parsed["planes"][ck.SUM]["offset"] + 16, "offset"), (3, 16, "size")):
        entry = list(ck.PLANE.unpack_from(good, ck.HEADER.size))
        entry[field] = value
        bad = bytearray(good)
        bad[ck.HEADER.size:ck.HEADER.size + ck.PLANE.size] = ck.PLANE.pack(*entry)
        _refused(bytes(bad), "plane SUM", word)
    bad = bytearray(good)
    bad[ck.HEADER.size:ck.HEADER.size + 4] = (2).to_bytes(4, "little")  # the first plane is not SUM
    _refused(bytes(bad), "kinds")
    # the same blobs through the stand-alone program: the same verdicts, nothing for the sanitizers to find
    paths = []
    for name, b in cases.items():
        paths.append(san.dir / (name + ".ckpt"))
        paths[-1].write_bytes(b)
    lines = san("info", *paths).splitlines()
    assert [l.split()[0] for l in lines] == ["ok"] + ["refused"] * (len(cases) - 1), lines


def test_merge_refusals():
    rng = np.random.default_rng(2)
    blobs, _ = _owners(rng)

    def refused(sections, *words):
        with pytest.raises(capi.KajoError) as e:
            checkpoint_merge(sections)
        assert e.value.code == capi.KAJO_E_INVALID
        for w in words:
            assert w in str(e.value), str(e.value)

    refused(blobs[:2], "owners")  # a missing owner
    refused([blobs[0], blobs[1], blobs[1]], "twice")  # overlapping owners
    refused(blobs + [blobs[0]], "owners")
    other, _ = _owners(np.random.default_rng(2), passes=7)
    refused([blobs[0], blobs[1], other[2]], "pass count")  # mixed pass counts
    other, _ = _owners(np.random.default_rng(2), fingerprint=0x99)
    refused([blobs[0], other[1], blobs[2]], "fingerprint")
    other, _ = _owners(np.random.default_rng(2), tile=(16, 16))
    refused([blobs[0], blobs[1], other[2]], "tile layout")
    other, _ = _owners(np.random.default_rng(2), counters=False)
    refused([blobs[0], blobs[1], other[2]], "COUNTERS")
    other, _ = _owners(np.random.default_rng(2), kinds=(ck.SUM, ck.NOISE_MOMENTS))
    refused([blobs[0], blobs[1], other[2]], "planes")
    bad = bytearray(blobs[1])
    bad[ck.parse(blobs[1])["planes"][ck.SUM]["offset"]] ^= 1
    refused([blobs[0], bytes(bad), blobs[2]], "section 1", "plane SUM")
    # an ADAPT section
    W, H = 41, 23
    p = _planes(rng, W * H, (ck.SUM, ck.NOISE_BASE, ck.NOISE_MOMENTS))
    p[ck.ADAPT] = np.zeros(ck.KIND_WORDS[ck.MATTE] + 3, np.uint32)
    refused([ck.section(W, H, p)], "ADAPT")


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------

def _compile():
    b = devicecode.build("checkpoint_kernels.cpp")
    assert "--offload-arch=gfx950" in b.cmd
    return b.resources, b.asm


def test_checkpoint_kernels_spill_nothing_and_use_no_scratch_flat_or_atomics():
    res, asm = _compile()
    assert sorted(res) == sorted(KERNELS), sorted(res)
    for k in KERNELS:
        r = res[k]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        body = devicecode.body(asm, k)
        assert not re.search(r"\n\s+flat_\w+", body), (k, re.findall(r"\n\s+(flat_\w+)", body)[:5])
        assert not re.search(r"\n\s+scratch_\w+", body), k
        assert not re.search(r"\n\s+\w*atomic\w*", body), k
    # the records move as 16-byte vectors
    for k in ("kajo_ckpt_pack", "kajo_ckpt_unpack"):
        body = devicecode.body(asm, k)
        assert re.search(r"\n\s+global_load_dwordx4", body) and re.search(r"\n\s+global_store_dwordx4", body), k


def test_makefile_links_the_checkpoints_into_the_product_and_the_tools_twin():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all", "tune"], capture_output=True, text=True, check=True).stdout
    links = [l for l in plan.splitlines() if l.startswith("hipcc") and " -shared " in l]
    assert len(links) == 2 and all("checkpoint_kernels.o" in l for l in links), links


# ---- the header and the binding ---------------------------------------------------------------------------------------------------------

def test_header_exports_and_library_agree():
    header = open(os.path.join(ROOT, "include", "kajo_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("kajo_hip_checkpoint_bytes", "kajo_hip_checkpoint_save", "kajo_hip_checkpoint_restore", "kajo_hip_checkpoint_info",
                 "kajo_hip_checkpoint_merge", "kajo_hip_digest"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in capi.EXPORTS
        assert re.search(r"\bT %s\b" % name, nm), name
    for struct, size in ((capi.KajoCheckpointPlane, 32), (capi.KajoCheckpointHeader, 104), (capi.KajoCheckpointTrailer, 16),
                         (capi.KajoCheckpointInfo, 408), (capi.KajoDigest, 80)):
        assert C.sizeof(struct) == size, struct
        m = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* (\d+) bytes \*/" % (struct.__name__, struct.__name__), header, re.S)
        assert m and int(m.group(2)) == size, struct
        fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)  # `type a, b[N];` statements
        declared = [n for stmt in fields.split(";") for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", stmt.strip())]
        assert declared == [f for f, *_ in struct._fields_], (struct, declared)
    assert C.sizeof(capi.KajoCheckpointHeader) == ck.HEADER.size
    for k, name in enumerate(capi.KAJO_CKPT_NAMES[1:], 1):
        assert re.search(r"#define KAJO_CKPT_%s %du\b" % (name, k), header), name
    assert re.search(r"#define KAJO_CKPT_VERSION %du\b" % capi.KAJO_CKPT_VERSION, header)
    assert re.search(r"#define KAJO_CKPT_ADAPT_WORDS %d\b" % capi.KAJO_CKPT_ADAPT_WORDS, header)


def test_null_arguments_are_refused_without_a_device():
    L = capi.lib()
    size = C.c_size_t()
    assert L.kajo_hip_checkpoint_bytes(None, C.byref(size)) == capi.KAJO_E_INVALID
    assert L.kajo_hip_checkpoint_save(None, None, 0, C.byref(size)) == capi.KAJO_E_INVALID
    assert L.kajo_hip_checkpoint_restore(None, b"x", 1) == capi.KAJO_E_INVALID
    assert L.kajo_hip_digest(None, C.byref(capi.KajoDigest())) == capi.KAJO_E_INVALID
    assert L.kajo_hip_checkpoint_info(None, 0, C.byref(capi.KajoCheckpointInfo())) == capi.KAJO_E_INVALID
    assert L.kajo_hip_checkpoint_merge(None, None, 0, None, 0, C.byref(size)) == capi.KAJO_E_INVALID
