"""What the stage tests share around a frame: its bits, a synthetic frame written into a handle's accumulation through the tile buffer,
the AOV sums written through the AOV tile buffer, and readers of the files the driver writes (PNG, PFM)."""
import struct
import zlib

import numpy as np

from kajo_amd.tiles import TileLayout


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tile_view(ptr, nbytes):
    """a device buffer of float4 records as a torch tensor (-1, 4)"""
    import torch
    from bench import DevicePtr
    return torch.as_tensor(DevicePtr(ptr, nbytes // 4), device="cuda").view(-1, 4)


def slots(W, H, tile=(64, 16)):
    """the slot of every pixel of a one-owner frame in its tile buffer, row by row, on the device"""
    import torch
    ys, xs = np.mgrid[0:H, 0:W]
    _, s = TileLayout(W, H, 1, tile).owner_and_slot(xs, ys)
    return torch.as_tensor(s.reshape(-1).astype(np.int64), device="cuda")


def upload_frame(r, frame, passes, tile=(64, 16)):
    """Write `frame` (H, W, 4) float32 into the handle's accumulation through its tile buffer and declare it the sum of `passes`;
    tile = the tile shape the handle was created with."""
    import torch
    H, W = frame.shape[:2]
    buf = tile_view(*r.tile_buffer())
    buf[slots(W, H, tile)] = torch.as_tensor(np.ascontiguousarray(frame).reshape(-1, 4), device="cuda")
    torch.cuda.synchronize()
    r.set_pass_count(passes)
    assert np.array_equal(bits(r.radiance()), bits(frame))


def upload_aov(r, A, B):
    """Write the AOV sums into the AOV tile buffer of a one-owner handle with tiled AOVs, then compose them."""
    import torch
    H, W = A.shape[:2]
    ptr, nbytes, _, _ = r.aov_tile_buffers()
    buf = tile_view(ptr, nbytes)
    per_owner = buf.shape[0] // 2
    s = slots(W, H)
    buf[s] = torch.as_tensor(np.ascontiguousarray(A).reshape(-1, 4), device="cuda")
    buf[per_owner + s] = torch.as_tensor(np.ascontiguousarray(B).reshape(-1, 4), device="cuda")
    torch.cuda.synchronize()
    r.compose_aov()
    a, b = r.aov()["raw"]
    assert np.array_equal(bits(a), bits(A)) and np.array_equal(bits(b), bits(B))


def read_png(path):
    """an 8-bit RGBA PNG of unfiltered rows -> (h, w, 4) uint8; the signature and every chunk's CRC are checked"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert zlib.crc32(typ + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        if typ == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert depth == 8 and ctype == 6
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 4)


def read_pfm(path):
    """a PFM file -> (h, w, 3) float32 (PF) or (h, w, 1) (Pf), top row first"""
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4")
    c = 3 if kind == b"PF" else 1
    assert kind in (b"PF", b"Pf") and data.size == w * h * c
    return data.reshape(h, w, c)[::-1]  # (rows are stored bottom to top)
