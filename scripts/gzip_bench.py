"""GPU DEFLATE (csrc/fc2_deflate.hip) against the CPU on the text of spliced_reads.fastq.gz: the reads
text the command line writes for scripts/gen_reads' --reads input (or --text FILE) compressed by
fc2_deflate_launch in one launch and in launches of --piece bytes (the writer's piece), timed with
HIP events on the launch stream; with both copies (fc2_gpu_gzip: pinned staging, upload, kernel,
download, members assembled) on the wall clock; every tile's stream checked with zlib.  The CPU legs
are libdeflate level 1 (the default writer; fc2_deflate.h) and zlib level 1 on one core over the same
bytes, and zlib level 6 over each tile alone (what a BGZF writer at its default makes of the same cuts).
--level 2 runs the compressor's second level (fc2_deflate_launch_level).  --hist H gives every tile the H
bytes before it in its launch as a window (fc2_deflate_launch_hist, fc2_gpu_gzip_hist): a launch is then one
DEFLATE stream, checked whole -- the piece launches' streams are the ones inflated -- and zlib level 6's
figure stays that of tiles cut alone.  One JSON line.  Measurement infrastructure (not part of the product).

usage: python scripts/gzip_bench.py [--reads N | --text FILE] [--tile T] [--piece P] [--reps R] [--level 1|2] [--hist H]
"""
import argparse
import ctypes
import gzip
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def reads_text(n_reads):
    from cli_steady import prepare, run_cli
    d = tempfile.mkdtemp(prefix="fc2_gzip_")
    fa, bams, _, _ = prepare(d, [n_reads])
    out = os.path.join(d, "out")
    run_cli(fa, bams[n_reads], out, 0, env_extra={"FC2_GPU_GZIP": "0"})
    with gzip.open(os.path.join(out, "spliced_reads.fastq.gz")) as f:
        return f.read()


def libdeflate_level1(text):
    """(bytes, seconds) of libdeflate_gzip_compress at level 1, or None without the library."""
    try:
        ld = ctypes.CDLL("libdeflate.so.0")
    except OSError:
        return None
    ld.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    ld.libdeflate_gzip_compress_bound.restype = ctypes.c_size_t
    ld.libdeflate_gzip_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    ld.libdeflate_gzip_compress.restype = ctypes.c_size_t
    ld.libdeflate_gzip_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_size_t]
    ld.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    c = ctypes.c_void_p(ld.libdeflate_alloc_compressor(1))
    piece, total = 4 << 20, 0
    out = ctypes.create_string_buffer(ld.libdeflate_gzip_compress_bound(c, piece))
    t0 = time.time()
    for b0 in range(0, len(text), piece):           # the writer's pieces, one member each
        total += ld.libdeflate_gzip_compress(c, text[b0:b0 + piece], min(piece, len(text) - b0), out, len(out))
    s = time.time() - t0
    ld.libdeflate_free_compressor(c)
    return total, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--text", default="")
    ap.add_argument("--tile", type=int, default=32768)
    ap.add_argument("--piece", type=int, default=4 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=int, default=1, choices=[1, 2])
    ap.add_argument("--hist", type=int, default=0)
    a = ap.parse_args()
    import torch
    from find_circ2_amd import _native as N
    text = open(a.text, "rb").read() if a.text else reads_text(a.reads)
    n, tile = len(text), a.tile
    tiles = (n + tile - 1) // tile
    stride = (tile + 16 + 15) & ~15
    L = N.lib()
    dev = torch.device("cuda:0")
    src = torch.tensor(np.frombuffer(text, np.uint8).copy(), device=dev)
    dst = torch.empty(tiles * stride, dtype=torch.uint8, device=dev)
    ln = torch.empty(tiles, dtype=torch.int32, device=dev)
    cr = torch.empty(tiles, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(L.fc2_deflate_scratch_bytes(n, tile)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    per = max(1, a.piece // tile)                    # tiles per piece

    def launch(t0, t1):
        b0, b1 = t0 * tile, min(n, t1 * tile)
        if a.hist:
            N.check(L.fc2_deflate_launch_hist(src.data_ptr() + b0, b1 - b0, tile, a.hist, dst.data_ptr() + t0 * stride,
                                              stride, ln.data_ptr() + 4 * t0, cr.data_ptr() + 4 * t0,
                                              scratch.data_ptr() + 4 * b0, ctypes.c_void_p(stream.cuda_stream), a.level))
            return
        N.check(L.fc2_deflate_launch_level(src.data_ptr() + b0, b1 - b0, tile, dst.data_ptr() + t0 * stride, stride,
                                           ln.data_ptr() + 4 * t0, cr.data_ptr() + 4 * t0, scratch.data_ptr() + 4 * b0,
                                           ctypes.c_void_p(stream.cuda_stream), a.level))

    spread = {}                                     # every repetition's ms, by tiles per launch

    def timed(step):
        best, every = None, []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for t0 in range(0, tiles, step):
                launch(t0, min(tiles, t0 + step))
            e1.record(stream)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            every.append(round(ms, 3))
            best = ms if best is None else min(best, ms)
        spread[step] = every
        return best

    if a.hist:                                      # checked as the writer launches: a stream per piece
        for t0 in range(0, tiles, per):
            launch(t0, min(tiles, t0 + per))
    else:
        launch(0, tiles)
    torch.cuda.synchronize()
    lens = ln.cpu().numpy().view(np.uint32)
    crcs = cr.cpu().numpy().view(np.uint32)
    out = dst.cpu().numpy()
    bad = 0
    for t0 in range(0, tiles if a.hist else 0, per):
        t1 = min(tiles, t0 + per)
        want = text[t0 * tile:t1 * tile]
        z = zlib.decompressobj(-15)
        try:
            ok = z.decompress(b"".join(out[i * stride:i * stride + int(lens[i])].tobytes() for i in range(t0, t1))) == want \
                and z.eof and not z.unused_data
        except zlib.error:
            ok = False
        bad += (t1 - t0) if not ok else sum(int(crcs[i]) != zlib.crc32(text[i * tile:(i + 1) * tile]) for i in range(t0, t1))
    stream_bytes = int(lens.sum())
    for i in range(0 if a.hist else tiles):
        want = text[i * tile:(i + 1) * tile]
        z = zlib.decompressobj(-15)
        try:
            ok = z.decompress(out[i * stride:i * stride + int(lens[i])].tobytes()) == want and z.eof
        except zlib.error:
            ok = False
        bad += not (ok and int(crcs[i]) == zlib.crc32(want))
    ms_all, ms_piece = timed(tiles), timed(per)
    # with both copies: the writer's host path
    cap = int(L.fc2_gpu_gzip_bound(n, tile))
    buf = (ctypes.c_uint8 * cap)()
    got = ctypes.c_uint64(0)
    wall = None
    for _ in range(max(2, a.reps)):
        t0 = time.time()
        if a.hist:
            N.check(L.fc2_gpu_gzip_hist(0, text, n, tile, a.hist, a.level, buf, cap, ctypes.byref(got)))
        else:
            N.check(L.fc2_gpu_gzip_level(0, text, n, tile, a.level, buf, cap, ctypes.byref(got)))
        s = time.time() - t0
        wall = s if wall is None else min(wall, s)
    host_ok = gzip.decompress(bytes(bytearray(buf)[:got.value])) == text
    ld = libdeflate_level1(text)
    t0 = time.time()
    zl = sum(len(zlib.compress(text[b0:b0 + (4 << 20)], 1)) for b0 in range(0, n, 4 << 20))
    zl_s = time.time() - t0
    z6 = 0
    for b0 in range(0, n, tile):                    # raw streams, as the GPU's are counted
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        z6 += len(c.compress(text[b0:b0 + tile])) + len(c.flush())
    print(json.dumps({
        "text_bytes": n, "level": a.level, "tile": tile, "hist": a.hist, "tiles": tiles, "bad_tiles": int(bad), "host_path_ok": bool(host_ok),
        "gpu_stream_bytes": stream_bytes, "gpu_gzip_bytes": int(got.value),
        "gpu_ratio": round(int(got.value) / n, 4),
        "zlib6_per_tile_stream_bytes": z6, "gpu_over_zlib6_per_tile": round(stream_bytes / z6, 4),
        "gpu_one_launch_ms_every": spread[tiles], "gpu_pieces_ms_every": spread[per],
        "gpu_one_launch_ms": round(ms_all, 3), "gpu_one_launch_GBps": round(n / ms_all / 1e6, 2),
        "gpu_piece_bytes": per * tile, "gpu_pieces_ms": round(ms_piece, 3), "gpu_pieces_GBps": round(n / ms_piece / 1e6, 2),
        "gpu_with_copies_s": round(wall, 4), "gpu_with_copies_GBps": round(n / wall / 1e9, 3),
        "libdeflate1_bytes": ld[0] if ld else None, "libdeflate1_ratio": round(ld[0] / n, 4) if ld else None,
        "libdeflate1_1core_GBps": round(n / ld[1] / 1e9, 3) if ld else None,
        "zlib1_bytes": zl, "zlib1_ratio": round(zl / n, 4), "zlib1_1core_GBps": round(n / zl_s / 1e9, 3),
        "gpu_over_libdeflate1_size": round(int(got.value) / ld[0], 3) if ld else None}))


if __name__ == "__main__":
    main()
