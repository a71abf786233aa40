"""Level 2's search effort on the GPU (csrc/fc2_deflate.hip "Search effort", fc2_deflate_launch_deep) measured beside
level 2 itself in one process: the record bytes of a BAM file (--bam FILE: its inflated stream after the header)
in blocks of 0xff00 bytes, untiled and cut into tiles (--tile 16320 --hist 32768), and the text of a gzip file
(--gz FILE) in tiles of 32768 bytes without and with 32768 bytes of history.  For every shape: level 2 through its
existing entry (fc2_deflate_launch_level, _groups, _hist), then every (depth, nice) of --grid through
fc2_deflate_launch_deep -- or, for an entry depth:nice:passes, through fc2_deflate_launch_priced (csrc/fc2_deflate.hip
"Priced passes").  Timed with HIP events on the launch stream, --reps launches of every piece (the writers'
pieces: 64 blocks of records, 4 MiB of text), min and max of a whole pass and per piece; the streams' bytes (for
records: as BGZF, 26 bytes a block more) against zlib level 6 over the same blocks; every stream inflated by zlib
and compared; at (8, 32) and at 8:32:1 the slots compared with level 2's.  --lib PATH: the existing entries of another build of
the library (a parent commit's) timed in the same process, first and last, and its slots compared.  One JSON line a
row.  Measurement infrastructure (not part of the product).

usage: python scripts/deflate_search_bench.py [--bam FILE] [--gz FILE] [--max-bytes N] [--grid 8:258,16:258,...]
                                              [--tile 16320] [--hist 32768] [--reps 7] [--lib PATH]
"""
import argparse
import ctypes
import gzip
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
BLOCK = 0xff00
GRID = "8:32,8:258,16:258,32:258,64:258,128:258,32:32"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam", default="")
    ap.add_argument("--gz", default="")
    ap.add_argument("--max-bytes", type=int, default=64 << 20)
    ap.add_argument("--grid", default=GRID)
    ap.add_argument("--tile", type=int, default=16320)
    ap.add_argument("--hist", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lib", default="")
    a = ap.parse_args()
    import torch
    from bgzf_tiles_bench import bam_records
    from find_circ2_amd import _native as N
    L = N.lib()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    P = None
    if a.lib:                                       # (a parent's library: the entries it has)
        P = ctypes.CDLL(os.path.abspath(a.lib))
        P.fc2_deflate_launch_level.argtypes = [vp, u64, u32, vp, u32, vp, vp, vp, vp, ctypes.c_int]
        P.fc2_deflate_launch_hist.argtypes = [vp, u64, u32, u32, vp, u32, vp, vp, vp, vp, ctypes.c_int]
        P.fc2_deflate_launch_groups.argtypes = [vp, u64, u32, u32, u32, vp, u32, vp, vp, vp, vp, ctypes.c_int]
    grid = [tuple(int(v) for v in g.split(":")) for g in a.grid.split(",")]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)

    def check(rc):
        if rc != 0:
            raise RuntimeError("launch failed: %d %s" % (rc, L.fc2_last_error()))

    def shape(name, data, piece, group, tile, hist, overhead):
        """One launch shape over data cut into pieces: rows for level 2 and every grid setting."""
        n = len(data)
        tpg = (group - 1) // tile + 1 if group else 1
        stride = (tile + 16 + 15) & ~15
        src = torch.tensor(np.frombuffer(data, np.uint8).copy(), device=dev)
        starts = list(range(0, n, piece))

        def tiles_of(k):
            return (k // group * tpg + (k % group + tile - 1) // tile) if group else (k + tile - 1) // tile

        first = [0]
        for x0 in starts:
            first.append(first[-1] + tiles_of(min(piece, n - x0)))
        n_tiles = first[-1]
        slots = torch.zeros((n_tiles + 1) * stride, dtype=torch.uint8, device=dev)
        ln = torch.zeros(n_tiles, dtype=torch.int32, device=dev)
        cr = torch.zeros(n_tiles, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(L.fc2_deflate_scratch_bytes(n, tile)) + 4 * tile, dtype=torch.uint8, device=dev)
        # what zlib level 6 makes of the same streams (a stream: a block of records, or a piece or tile of text)
        unit = group if group else (piece if hist else tile)
        z6 = 0
        for x0 in range(0, n, unit):
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            z6 += overhead + len(c.compress(data[x0:x0 + unit])) + len(c.flush())

        def launch(lib, setting, p):
            x0, k, t0 = starts[p], min(piece, n - starts[p]), first[p]
            args = (slots.data_ptr() + t0 * stride, stride, ln.data_ptr() + 4 * t0, cr.data_ptr() + 4 * t0,
                    scratch.data_ptr() + 4 * x0, sp)
            if setting is not None and len(setting) == 3:
                check(L.fc2_deflate_launch_priced(src.data_ptr() + x0, k, group, tile, hist, *args, *setting))
            elif setting is not None:
                check(L.fc2_deflate_launch_deep(src.data_ptr() + x0, k, group, tile, hist, *args, setting[0], setting[1]))
            elif group:
                check(lib.fc2_deflate_launch_groups(src.data_ptr() + x0, k, group, tile, hist, *args, 2))
            elif hist:
                check(lib.fc2_deflate_launch_hist(src.data_ptr() + x0, k, tile, hist, *args, 2))
            else:
                check(lib.fc2_deflate_launch_level(src.data_ptr() + x0, k, tile, *args, 2))

        def run(tag, lib, setting):
            for p in range(len(starts)):            # (warm: the kernel's LDS reservation, the first launch)
                launch(lib, setting, p)
            torch.cuda.synchronize()
            passes, per_piece = [], []
            for _ in range(a.reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(starts) + 1)]
                ev[0].record(stream)
                for p in range(len(starts)):
                    launch(lib, setting, p)
                    ev[p + 1].record(stream)
                torch.cuda.synchronize()
                passes.append(round(ev[0].elapsed_time(ev[-1]), 3))
                if len(starts[:-1]):                # whole pieces only
                    per_piece += [ev[p].elapsed_time(ev[p + 1]) for p in range(len(starts) - 1)]
            lens = ln.cpu().numpy().view(np.uint32)
            host = slots.cpu().numpy()
            streams = [host[i * stride:i * stride + int(lens[i])].tobytes() for i in range(n_tiles)]
            bad, i = 0, 0
            for x0 in range(0, n, unit):            # every stream inflates to its bytes
                part = data[x0:x0 + unit]
                cnt = tiles_of(len(part)) if (group or hist) else 1
                try:
                    z = zlib.decompressobj(-15)
                    bad += z.decompress(b"".join(streams[i:i + cnt])) != part or not z.eof
                except zlib.error:
                    bad += 1
                i += cnt
            total = int(lens.astype(np.uint64).sum()) + overhead * len(range(0, n, unit))
            row = {"shape": name, "tag": tag, "depth": setting[0] if setting else 8, "nice": setting[1] if setting else 32,
                   "passes": setting[2] if setting and len(setting) == 3 else 1,
                   "entry": ("priced" if len(setting) == 3 else "deep") if setting else "level2", "bytes_in": n, "tile": tile, "hist": hist, "group": group,
                   "pieces": len(starts), "piece_bytes": piece, "bad_streams": int(bad), "bytes_out": total,
                   "zlib6_bytes": z6, "over_zlib6": round(total / z6, 4), "pass_ms_every": passes,
                   "pass_ms_min": min(passes), "pass_ms_max": max(passes),
                   "piece_ms_min": round(min(per_piece), 4) if per_piece else None,
                   "piece_ms_max": round(max(per_piece), 4) if per_piece else None,
                   "GBps_at_min": round(n / min(passes) / 1e6, 2)}
            return row, streams

        rows = []
        if P is not None:
            r, parent = run("parent", P, None)
            rows.append(r)
        r, base = run("tree", L, None)
        rows.append(r)
        if P is not None:
            r["slots_equal_parent"] = base == parent
        for g in grid:
            r, s = run("tree", L, g)
            r["bytes_over_level2"] = round(r["bytes_out"] / rows[1 if P is not None else 0]["bytes_out"], 4)
            r["pass_ms_over_level2"] = round(r["pass_ms_min"] / rows[1 if P is not None else 0]["pass_ms_min"], 3)
            if g in ((8, 32), (8, 32, 1)):
                r["slots_equal_level2"] = s == base
            rows.append(r)
        if P is not None:
            r, again = run("parent_again", P, None)
            r["slots_equal_parent"] = again == base
            rows.append(r)
        for r in rows:
            print(json.dumps(r), flush=True)

    if a.bam:
        rec = bam_records(a.bam, a.max_bytes)
        shape("bam_untiled", rec, 64 * BLOCK, 0, BLOCK, 0, 26)
        shape("bam_tiles", rec, 64 * BLOCK, BLOCK, a.tile, a.hist, 26)
    if a.gz:
        with gzip.open(a.gz) as f:
            text = f.read(a.max_bytes)
        shape("gzip_tile32768", text, 4 << 20, 0, 32768, 0, 18)
        shape("gzip_hist32768", text, 4 << 20, 0, 32768, 32768, 18)


if __name__ == "__main__":
    main()
