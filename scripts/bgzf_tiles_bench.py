"""Tiles inside a BGZF block on the GPU (csrc/fc2_deflate.hip "Groups", csrc/fc2_bgzf_out.hip) on BAM records:
the record bytes of a BAM file (--bam FILE: its inflated stream after the header; or --records FILE, raw)
compressed in blocks of 0xff00 bytes cut into tiles, timed with HIP events on the launch stream -- the
compressor in one launch over all blocks and in launches of --piece-blocks blocks (the writer's piece), the
framing kernels over the same pieces on their own -- with the finished BGZF stream's size against zlib level 6
over the same blocks, and every piece inflated by zlib and compared.  --tile 0 (or >= 0xff00) is the untiled
writer: fc2_deflate_launch_level and fc2_bgzf_frame_launch, which a parent commit's library has too (--lib
PATH loads that one instead of the tree's).  One JSON line.  Measurement infrastructure (not part of the
product).

usage: python scripts/bgzf_tiles_bench.py (--bam FILE | --records FILE) [--max-bytes N] [--tile T] [--hist H]
                                          [--level 1|2] [--piece-blocks 64] [--reps 5] [--lib PATH]
"""
import argparse
import ctypes
import gzip
import json
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK = 0xff00


def bam_records(path, max_bytes):
    with gzip.open(path) as f:
        data = f.read(max_bytes + (1 << 20) if max_bytes else -1)
    lt, = struct.unpack_from("<i", data, 4)
    o = 8 + lt
    nref, = struct.unpack_from("<i", data, o)
    o += 4
    for _ in range(nref):
        ln, = struct.unpack_from("<i", data, o)
        o += 8 + ln
    return data[o:o + max_bytes] if max_bytes else data[o:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam", default="")
    ap.add_argument("--records", default="")
    ap.add_argument("--max-bytes", type=int, default=64 << 20)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--hist", type=int, default=32768)
    ap.add_argument("--level", type=int, default=1, choices=[1, 2])
    ap.add_argument("--piece-blocks", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default="")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import torch
    data = bam_records(a.bam, a.max_bytes) if a.bam else open(a.records, "rb").read()[:a.max_bytes or None]
    n = len(data)
    tiled = 0 < a.tile < BLOCK
    tile = a.tile if tiled else BLOCK
    hist = a.hist if tiled else 0
    tpg = (BLOCK - 1) // tile + 1
    n_blocks = (n + BLOCK - 1) // BLOCK
    stride = (tile + 16 + 15) & ~15
    if a.lib:
        L = ctypes.CDLL(os.path.abspath(a.lib))
    else:
        from find_circ2_amd import _native as N
        L = N.lib()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    if a.lib:                                       # (a parent's library: the entry points it has)
        L.fc2_deflate_launch_level.argtypes = [vp, u64, u32, vp, u32, vp, vp, vp, vp, ctypes.c_int]
        L.fc2_bgzf_frame_launch.argtypes = [vp, u32, vp, vp, u32, u64, u32, vp, vp, vp, vp]
        L.fc2_deflate_scratch_bytes.restype = u64
        L.fc2_deflate_scratch_bytes.argtypes = [u64, u32]
    dev = torch.device("cuda:0")
    src = torch.tensor(np.frombuffer(data, np.uint8).copy(), device=dev)
    n_tiles = n // BLOCK * tpg + (n % BLOCK + tile - 1) // tile
    slots = torch.empty((n_tiles + 1) * stride, dtype=torch.uint8, device=dev)
    ln = torch.empty(n_tiles, dtype=torch.int32, device=dev)
    cr = torch.empty(n_tiles, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(L.fc2_deflate_scratch_bytes(n, tile)), dtype=torch.uint8, device=dev)
    out = torch.empty(n_blocks * 65536, dtype=torch.uint8, device=dev)
    off = torch.empty(n_blocks + a.piece_blocks + 8, dtype=torch.int32, device=dev)
    totals = torch.zeros((n_blocks + a.piece_blocks - 1) // a.piece_blocks, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)

    def check(rc):
        if rc != 0:
            raise RuntimeError("launch failed: %d" % rc)

    def deflate(b0, b1):                            # blocks [b0, b1)
        x0, x1, t0 = b0 * BLOCK, min(n, b1 * BLOCK), b0 * tpg
        if tiled:
            check(L.fc2_deflate_launch_groups(src.data_ptr() + x0, x1 - x0, BLOCK, tile, hist, slots.data_ptr() + t0 * stride,
                                              stride, ln.data_ptr() + 4 * t0, cr.data_ptr() + 4 * t0,
                                              scratch.data_ptr() + 4 * x0, sp, a.level))
        else:
            check(L.fc2_deflate_launch_level(src.data_ptr() + x0, x1 - x0, BLOCK, slots.data_ptr() + t0 * stride, stride,
                                             ln.data_ptr() + 4 * t0, cr.data_ptr() + 4 * t0, scratch.data_ptr() + 4 * x0, sp,
                                             a.level))

    def frame(b0, b1):                              # the piece of blocks [b0, b1) to out + b0 * 65536
        x0, x1, t0 = b0 * BLOCK, min(n, b1 * BLOCK), b0 * tpg
        t1 = min(n_tiles, b1 * tpg)
        p = b0 // a.piece_blocks
        if tiled:
            check(L.fc2_bgzf_frame_groups_launch(slots.data_ptr() + t0 * stride, stride, ln.data_ptr() + 4 * t0,
                                                 cr.data_ptr() + 4 * t0, t1 - t0, x1 - x0, BLOCK, tile,
                                                 out.data_ptr() + b0 * 65536, off.data_ptr() + 4 * b0, totals.data_ptr() + 4 * p, sp))
        else:
            check(L.fc2_bgzf_frame_launch(slots.data_ptr() + t0 * stride, stride, ln.data_ptr() + 4 * t0, cr.data_ptr() + 4 * t0,
                                          t1 - t0, x1 - x0, BLOCK, out.data_ptr() + b0 * 65536, off.data_ptr() + 4 * b0,
                                          totals.data_ptr() + 4 * p, sp))

    def timed(fn, step):
        every = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for b0 in range(0, n_blocks, step):
                fn(b0, min(n_blocks, b0 + step))
            e1.record(stream)
            torch.cuda.synchronize()
            every.append(round(e0.elapsed_time(e1), 3))
        return every

    pb = a.piece_blocks
    deflate(0, n_blocks)                            # (warm: the kernel's LDS reservation, the first launch)
    torch.cuda.synchronize()
    one = timed(deflate, n_blocks)
    pieces = timed(deflate, pb)
    framing = timed(frame, pb)
    # the finished stream: every piece's total, inflated and compared
    tot = totals.cpu().numpy().view(np.uint32)
    host = out.cpu().numpy()
    bgzf_bytes, bad = int(tot.sum()), 0
    for p, b0 in enumerate(range(0, n_blocks, pb)):
        blob = host[b0 * 65536:b0 * 65536 + int(tot[p])].tobytes()
        try:
            bad += gzip.decompress(blob) != data[b0 * BLOCK:(b0 + pb) * BLOCK] or not blob
        except (OSError, zlib.error, EOFError):
            bad += 1
    z6 = 0
    for x0 in range(0, n, BLOCK):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        z6 += 26 + len(c.compress(data[x0:x0 + BLOCK])) + len(c.flush())
    ms1, msp, msf = min(one), min(pieces), min(framing)
    print(json.dumps({
        "tag": a.tag, "lib": a.lib or "tree", "record_bytes": n, "blocks": n_blocks, "level": a.level, "tile": tile, "hist": hist,
        "tiles_per_block": tpg, "piece_blocks": pb, "n_pieces": len(tot), "bad_pieces": int(bad),
        "bgzf_bytes": bgzf_bytes, "zlib6_bgzf_bytes": z6, "bgzf_over_zlib6": round(bgzf_bytes / z6, 4),
        "deflate_one_launch_ms_every": one, "deflate_pieces_ms_every": pieces, "frame_pieces_ms_every": framing,
        "deflate_one_launch_ms": ms1, "deflate_one_launch_GBps": round(n / ms1 / 1e6, 2),
        "deflate_pieces_ms": msp, "deflate_pieces_GBps": round(n / msp / 1e6, 2),
        "deflate_ms_per_piece": round(msp / len(tot), 4), "frame_ms_per_piece": round(msf / len(tot), 4),
        "frame_share_of_pieces": round(msf / (msf + msp), 4)}))


if __name__ == "__main__":
    main()
