"""GPU BGZF inflate (csrc/fc2_inflate.hip) against the CPU on the CLI's BAM input: the blocks of
scripts/gen_reads' BAM (fc2_sam_to_bam, zlib level 1) inflated by fc2_bgzf_inflate_launch in launches
of --batch blocks (the ingest's batch) and in one launch of all, timed with HIP events on the launch
stream, each block's CRC-32 checked on the device (and again here); the CPU leg is zlib on one core over the same blocks.
The walk leg times fc2_bam_walk_launch (the blocks' BAM record starts) over the same blocks, in the same
launches, from the slots the inflate left, its lists checked against fc2_bam_walk_host.  The digest leg
times fc2_bam_digest_launch (the listed records' derived fields) over the blocks' contiguous bytes and the
walk's lists, in launches of --batch blocks and of 1024 (its most), every 97th block's rows checked against
fc2_bam_digest_host.  One JSON line.
Measurement infrastructure (not part of the product).

usage: python scripts/inflate_bench.py [--reads N] [--batch B] [--reps R]
"""
import argparse
import ctypes
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


def blocks(raw: bytes):
    """(payload offsets, payload lengths, isizes, crcs) of a BGZF file's blocks."""
    off, ln, isz, crc, pos = [], [], [], [], 0
    mv = memoryview(raw)
    while pos < len(raw):
        xlen = raw[pos + 10] | (raw[pos + 11] << 8)
        bsize = (raw[pos + 16] | (raw[pos + 17] << 8)) + 1
        off.append(pos + 12 + xlen)
        ln.append(bsize - 12 - xlen - 8)
        crc.append(int.from_bytes(mv[pos + bsize - 8:pos + bsize - 4], "little"))
        isz.append(int.from_bytes(mv[pos + bsize - 4:pos + bsize], "little"))
        pos += bsize
    return [np.array(x, np.uint32) for x in (off, ln, isz, crc)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from cli_steady import prepare
    from find_circ2_amd import _native as N
    d = tempfile.mkdtemp(prefix="fc2_inflate_")
    _, bams, _, _ = prepare(d, [a.reads])
    raw = open(bams[a.reads], "rb").read()
    off, ln, isz, crc = blocks(raw)
    n = len(off)
    dev = torch.device("cuda:0")
    src = torch.tensor(np.frombuffer(raw + bytes(64), np.uint8), device=dev)
    t_off, t_ln, t_isz, t_crc = (torch.tensor(x.view(np.int32), device=dev) for x in (off, ln, isz, crc))
    dst = torch.empty(n * 65536, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    L = N.lib()

    def launch(i0, i1):
        N.check(L.fc2_bgzf_inflate_launch(src.data_ptr(), t_off[i0:].data_ptr(), t_ln[i0:].data_ptr(),
                                          t_isz[i0:].data_ptr(), t_crc[i0:].data_ptr(), dst[i0 * 65536:].data_ptr(),
                                          st[i0:].data_ptr(), i1 - i0, ctypes.c_void_p(stream.cuda_stream)))

    cap = N.BAM_WALK_CAP
    w_starts = torch.empty(n * cap, dtype=torch.int16, device=dev)
    w_count = torch.empty(n, dtype=torch.int32, device=dev)
    w_exit = torch.empty(n, dtype=torch.int32, device=dev)

    def walk(i0, i1):
        N.check(L.fc2_bam_walk_launch(dst[i0 * 65536:].data_ptr(), t_isz[i0:].data_ptr(), st[i0:].data_ptr(),
                                      w_starts[i0 * cap:].data_ptr(), w_count[i0:].data_ptr(), w_exit[i0:].data_ptr(),
                                      i1 - i0, ctypes.c_void_p(stream.cuda_stream)))

    def timed(step, launch=launch):
        best = None
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i0 in range(0, n, step):
                launch(i0, min(n, i0 + step))
            e1.record(stream)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return best

    launch(0, n)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    out = dst.cpu().numpy()
    bad = sum(1 for i in range(n) if s[i] != 0 or zlib.crc32(out[i * 65536:i * 65536 + isz[i]].tobytes()) != crc[i])
    ms_all, ms_batch = timed(n), timed(a.batch)
    # the walk over the inflated slots; every 97th block's lists against the CPU's walk
    walk(0, n)
    torch.cuda.synchronize()
    wc, we = w_count.cpu().numpy().view(np.uint32), w_exit.cpu().numpy().view(np.uint32)
    ws = w_starts.cpu().numpy().view(np.uint16).reshape(n, cap)
    row, hc, he = np.zeros(cap, np.uint16), ctypes.c_uint32(), ctypes.c_uint32()
    walk_bad = 0
    for i in range(0, n, 97):
        blk = np.ascontiguousarray(out[i * 65536:i * 65536 + isz[i]])
        N.check(L.fc2_bam_walk_host(blk.ctypes.data, int(isz[i]), row.ctypes.data, ctypes.byref(hc), ctypes.byref(he)))
        walk_bad += not (hc.value == wc[i] and he.value == we[i] and (row[:hc.value] == ws[i, :hc.value]).all())
    wms_all, wms_batch = timed(n, walk), timed(a.batch, walk)
    # the digest over the contiguous bytes (as the ingest's compaction leaves them) and the walk's lists:
    # a launch sees its own blocks' bytes only, its rows dense behind those of the launches before it
    ooff = np.concatenate([[0], np.cumsum(isz, dtype=np.int64)])
    cont = np.concatenate([out[i * 65536:i * 65536 + isz[i]] for i in range(n)])
    d_cont = torch.tensor(cont, device=dev)
    rbase = np.concatenate([[0], np.cumsum(np.minimum(wc, cap), dtype=np.int64)])
    d_rows = torch.empty(int(rbase[n]) * 32 + 32, dtype=torch.uint8, device=dev)
    d_first = torch.empty(2 * n + 2, dtype=torch.int32, device=dev)
    rel = {}

    def digest_step(step):
        if step not in rel:                    # block offsets relative to their launch's first block
            r = np.concatenate([ooff[i0:min(n, i0 + step)] - ooff[i0] for i0 in range(0, n, step)])
            rel[step] = torch.tensor(r.astype(np.uint32).view(np.int32), device=dev)

        def digest(i0, i1):
            N.check(L.fc2_bam_digest_launch(d_cont.data_ptr() + int(ooff[i0]), int(ooff[i1] - ooff[i0]),
                                            rel[step][i0:].data_ptr(), t_isz[i0:].data_ptr(), st[i0:].data_ptr(),
                                            w_starts[i0 * cap:].data_ptr(), w_count[i0:].data_ptr(),
                                            d_rows.data_ptr() + int(rbase[i0]) * 32,
                                            d_first.data_ptr() + 4 * (i0 + i0 // step), i1 - i0,
                                            ctypes.c_void_p(stream.cuda_stream)))
        return digest

    step = min(a.batch, N.BAM_DIGEST_MAX_BLOCKS)
    dms_batch = timed(step, digest_step(step))
    rows = d_rows.cpu().numpy()[:int(rbase[n]) * 32].view(
        np.dtype([("state", "u1"), ("as_type", "u1"), ("xs_type", "u1"), ("has_qual", "u1"), ("block_size", "<u4"),
                  ("astart", "<i4"), ("qlen", "<i4"), ("as_bits", "<u4"), ("xs_bits", "<u4"), ("aend", "<i8")]))
    first = d_first.cpu().numpy().view(np.uint32)
    hrow, digest_bad, digest_checked = N.BamDigest(), 0, 0
    for i in range(0, n, 97):
        i0 = i // step * step
        i1 = min(n, i0 + step)
        chunk = cont[ooff[i0]:ooff[i1]]
        f = int(first[i0 + i0 // step + (i - i0)])
        for k in range(min(int(wc[i]), cap)):
            N.check(L.fc2_bam_digest_host(chunk.ctypes.data, len(chunk), int(ooff[i] - ooff[i0]) + int(ws[i, k]), ctypes.byref(hrow)))
            got = tuple(int(x) for x in rows[int(rbase[i0]) + f + k].item())
            digest_bad += got != tuple(getattr(hrow, fld) for fld, _ in N.BamDigest._fields_)
            digest_checked += 1
    digest_state1 = int(rows["state"].sum())
    dms_1024 = timed(N.BAM_DIGEST_MAX_BLOCKS, digest_step(N.BAM_DIGEST_MAX_BLOCKS))
    total = int(isz.sum())
    # CPU: zlib on one core, about 2 s of it
    t0, done, k = time.time(), 0, 0
    while time.time() - t0 < 2.0 and k < n:
        done += len(zlib.decompress(raw[off[k]:off[k] + ln[k]], -15))
        k += 1
    cpu_s = time.time() - t0
    print(json.dumps({
        "reads": a.reads, "blocks": n, "compressed_bytes": len(raw), "inflated_bytes": total,
        "bad_blocks": bad, "status_nonzero": int((s != 0).sum()),
        "gpu_one_launch_ms": round(ms_all, 3), "gpu_one_launch_GBps": round(total / ms_all / 1e6, 2),
        "gpu_batch": a.batch, "gpu_batched_ms": round(ms_batch, 3),
        "gpu_batched_GBps": round(total / ms_batch / 1e6, 2),
        "cpu_zlib_1core_GBps": round(done / cpu_s / 1e9, 3),
        "walk_records": int(wc.sum()), "walk_bad_blocks": int(walk_bad),
        "walk_one_launch_ms": round(wms_all, 3), "walk_batched_ms": round(wms_batch, 3),
        "walk_share_of_inflate_one_launch": round(wms_all / ms_all, 4),
        "walk_share_of_inflate_batched": round(wms_batch / ms_batch, 4),
        "walk_list_bytes_per_block": cap * 2 + 8,
        "digest_rows": int(rbase[n]), "digest_rows_state1": digest_state1, "digest_rows_checked": digest_checked,
        "digest_bad_rows": int(digest_bad), "digest_batch": step, "digest_batched_ms": round(dms_batch, 3),
        "digest_1024_ms": round(dms_1024, 3), "digest_share_of_inflate_batched": round(dms_batch / ms_batch, 4),
        "digest_row_bytes": int(rbase[n]) * 32, "digest_row_bytes_share_of_inflated": round(int(rbase[n]) * 32 / total, 4)}))


if __name__ == "__main__":
    main()
