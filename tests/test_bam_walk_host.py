"""fc2_bam_walk_host (include/fc2_ingest.h) -- the ingest's walk_block on one inflated BGZF block, in the
form of the device's rows -- against a restatement in Python of bam_plausible and walk_block
(csrc/fc2_ingest.cpp), on hand-built blocks: every way a block can begin and end among BAM records.
The blocks (shapes()) are also what the kernel's test launches (test_gpu_bam_walk.py)."""
import ctypes
import functools
import struct

import numpy as np

from find_circ2_amd import _native as N

CAP = N.BAM_WALK_CAP
NO_EXIT = N.BAM_WALK_NO_EXIT


# ---- the restatement ------------------------------------------------------------------------------
def py_plausible(d: bytes, o: int, n: int) -> bool:
    """bam_plausible(d + o, n - o): a plausible BAM record at byte o of a block of n bytes."""
    avail = n - o
    if avail < 36:
        return False
    bs, ref, pos, lname = struct.unpack_from("<iiiB", d, o)
    ncig, = struct.unpack_from("<H", d, o + 16)
    lseq, nref, npos = struct.unpack_from("<iii", d, o + 20)
    if bs < 32 or bs >= (1 << 28) or ref < -1 or pos < -1 or lname < 1 or lseq < 0 or nref < -1 or npos < -1:
        return False
    if 32 + lname + 4 * ncig + (lseq + 1) // 2 + lseq > bs:
        return False
    if 36 + lname > avail:
        return True
    if d[o + 36 + lname - 1] != 0:
        return False
    return all(0x21 <= c <= 0x7e for c in d[o + 36:o + 36 + lname - 1])


def py_walk(d: bytes):
    """walk_block(d, 0, len(d)): (count, exit or NO_EXIT, starts)."""
    n = len(d)
    o = 0
    while o + 36 <= n:
        if py_plausible(d, o, n):
            nx = o + 4 + struct.unpack_from("<i", d, o)[0]
            if nx + 36 > n or py_plausible(d, nx, n):
                break
        o += 1
    if o + 36 > n:
        return 0, NO_EXIT, []
    starts = []
    while o + 4 <= n:
        bs, = struct.unpack_from("<i", d, o)
        if bs < 32:
            return len(starts), NO_EXIT, starts
        starts.append(o)
        o += 4 + bs
    return len(starts), o, starts


def host_walk(block: bytes):
    """fc2_bam_walk_host on block: (count, exit, starts[:count]); the rest of the row must be untouched."""
    buf = np.frombuffer(block, np.uint8) if block else np.zeros(1, np.uint8)
    starts = np.full(CAP + 2, 0xA5A5, np.uint16)
    cnt, ex = ctypes.c_uint32(77), ctypes.c_uint32(77)
    N.check(N.lib().fc2_bam_walk_host(buf.ctypes.data, len(block), starts[1:].ctypes.data, ctypes.byref(cnt),
                                      ctypes.byref(ex)))
    assert cnt.value <= CAP
    assert (starts[1 + cnt.value:] == 0xA5A5).all() and starts[0] == 0xA5A5
    return cnt.value, ex.value, [int(x) for x in starts[1:1 + cnt.value]]


# ---- hand-built records ---------------------------------------------------------------------------
def rec(name=b"read/1", n_cigar=2, l_seq=50, tags=b"NMC\x01ASC\x30", ref=1, pos=1000, qual=None, seq=None,
        nul=True, block_size=None):
    """One BAM record and the offsets of its parts: (bytes, {"name", "cigar", "seq", "qual", "tags"})."""
    qn = name + (b"\0" if nul else b"x")
    cig = b"".join(struct.pack("<I", (25 << 4) | (0 if k % 2 == 0 else 3)) for k in range(n_cigar))
    seq = bytes([0x12, 0x48, 0x84, 0x21][k % 4] for k in range((l_seq + 1) // 2)) if seq is None else seq
    qual = bytes([30 + k % 10 for k in range(l_seq)]) if qual is None else qual
    assert len(seq) == (l_seq + 1) // 2 and len(qual) == l_seq
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(qn), 60, 4681, n_cigar, 0, l_seq, -1, -1, 0)
    parts, off = {}, 4 + len(body)
    for key, b in (("name", qn), ("cigar", cig), ("seq", seq), ("qual", qual), ("tags", tags)):
        parts[key] = off
        off += len(b)
        body += b
    bs = len(body) if block_size is None else block_size
    return struct.pack("<i", bs) + body, parts


# The smallest records.  A record the search accepts as a first start (and as its follower) must be
# plausible, and with l_read_name >= 1 that takes block_size >= 33: 37 bytes, the name only a NUL.  The
# chain from there on asks only block_size >= 32: 36 bytes, the fixed fields alone.
MINIMAL = rec(name=b"", n_cigar=0, l_seq=0, tags=b"")[0]
HEADER36 = rec(name=b"", n_cigar=0, l_seq=0, tags=b"", block_size=32)[0][:36]
assert len(MINIMAL) == 37 and len(HEADER36) == 36
# 64 KiB of them: two plausible records, then 36-byte steps -- as many starts as a block can have
MAX_BLOCK = (MINIMAL * 2 + HEADER36 * 1819)[:65536]
MAX_STARTS = [0, 37] + list(range(74, 65536 - 3, 36))


def stream(n_rec, seed=0):
    """n_rec records of varied name, CIGAR, SEQ and tag lengths (their starts fall on every residue
    mod 4): (bytes, [start of each], [parts of each])."""
    rng = np.random.default_rng(seed)
    out, starts, parts = bytearray(), [], []
    for k in range(n_rec):
        r, p = rec(name=b"q%d:%s" % (k, b"ab" * int(rng.integers(0, 9)) + b"c" * int(rng.integers(0, 2))),
                   n_cigar=int(rng.integers(1, 5)), l_seq=int(rng.integers(30, 160)),
                   tags=b"NMC\x02" + b"XZZ" + b"t" * int(rng.integers(0, 7)) + b"\0", ref=k % 3, pos=100 * k)
        starts.append(len(out))
        parts.append(p)
        out += r
    return bytes(out), starts, parts


def _decoy(block_size):
    """A 37-byte plausible record header + empty name, to be planted inside a QUAL."""
    return struct.pack("<iiiBBHHHiiii", block_size, 0, 5, 1, 0, 0, 0, 0, 0, -1, -1, 0) + b"\0"


@functools.lru_cache(maxsize=None)
def shapes():
    """[(label, block bytes, the expected (count, exit, starts))]."""
    S, st, parts = stream(400, seed=3)
    assert len(S) > 70000 and {s % 4 for s in st} == {0, 1, 2, 3}
    out = []

    def following(cut, end):
        """what a walk finds in S[cut:end] when its first start is the first record at or after cut"""
        own = [s - cut for s in st if s >= cut and s + 4 <= end]
        nxt = [s for s in st + [len(S)] if s > cut + own[-1]][0] - cut
        return len(own), nxt, own

    # too short to hold a record, and the shortest that can
    for n in (0, 1, 35):
        out.append(("len%d" % n, S[:n], (0, NO_EXIT, [])))
    out.append(("len36_minimal", MINIMAL[:36], (1, 37, [0])))
    out.append(("len36_cut", S[:36], (1, st[1], [0])))            # its name lies past the end: still plausible
    # a block that begins exactly at a record (each residue), and inside each part of one
    for k in (0, 1, 2, 3, 5):
        a = st[10 + k]
        out.append(("at_record_%d" % (a % 4), S[a:a + 30000], following(a, a + 30000)))
    for j, part in enumerate(("name", "cigar", "seq", "qual", "tags")):
        a = st[40 + j] + parts[40 + j][part] + 2
        out.append(("inside_" + part, S[a:a + 20000 + j], following(a, a + 20000 + j)))
    out.append(("full_64k", S[st[7]:st[7] + 65536], following(st[7], st[7] + 65536)))
    # wholly inside one 80-kb record: nothing
    big, bp = rec(name=b"long", n_cigar=1, l_seq=53400)
    assert len(big) > 80000
    out.append(("inside_80kb", big[bp["seq"] + 100:bp["seq"] + 100 + 65536], (0, NO_EXIT, [])))
    # the last record runs past the end: the exit lies beyond n
    a, b = st[20], st[23] + 50
    out.append(("exit_past_end", S[a:b], (4, st[24] - a, [s - a for s in st[20:24]])))
    assert out[-1][2][1] > b - a
    # ... far beyond (a block_size of 2^31 - 1 where the chain reads it but no plausibility is asked)
    two = bytearray(S[st[30]:st[32] + 4])
    two[-4:] = struct.pack("<i", 0x7FFFFFFF)
    out.append(("exit_2g", bytes(two), (3, st[32] - st[30] + 4 + 0x7FFFFFFF, [0, st[31] - st[30], st[32] - st[30]])))
    # a block_size of 31 in the middle of the chain: the starts so far, no exit
    a = st[50]
    cut = bytearray(S[a:st[60]])
    cut[st[53] - a:st[53] - a + 4] = struct.pack("<i", 31)
    out.append(("block_size_31", bytes(cut), (3, NO_EXIT, [s - a for s in st[50:53]])))
    # decoy headers inside a QUAL: one whose follower (inside the block) is implausible is skipped;
    # one whose follower lies past the block's end is accepted and ends up as the first start
    for label, dbs in (("decoy_skipped", 40), ("decoy_accepted", 100000)):
        q = bytearray(30 + k % 10 for k in range(300))
        q[100:137] = _decoy(dbs)
        r, p = rec(name=b"host", l_seq=300, qual=bytes(q))
        blk = r[p["qual"] + 7:] + S[st[70]:st[80]]
        d0 = 100 - 7
        real = len(r) - p["qual"] - 7
        if dbs == 40:
            n_own = [real + s - st[70] for s in st[70:80]]
            out.append((label, blk, (10, real + st[80] - st[70], n_own)))
        else:
            out.append((label, blk, (1, d0 + 4 + dbs, [d0])))
    # a name byte outside 0x21..0x7e, and a name without its NUL: not a start; the next record is
    for label, r in (("name_space", rec(name=b"bad name")[0]), ("name_no_nul", rec(name=b"goodname", nul=False)[0])):
        blk = r + S[st[90]:st[95]]
        out.append((label, blk, (5, len(r) + st[95] - st[90], [len(r) + s - st[90] for s in st[90:95]])))
    # 64 KiB of minimal records: the most starts a block can have
    out.append(("max_count", MAX_BLOCK, (len(MAX_STARTS), MAX_STARTS[-1] + 36, MAX_STARTS)))
    return out


# ---- the tests ------------------------------------------------------------------------------------
def test_shapes_cover_every_residue():
    res = set()
    for _, blk, _ in shapes():
        res |= {s % 4 for s in py_walk(blk)[2]}
    assert res == {0, 1, 2, 3}


def test_restatement_gives_the_expected_lists():
    for label, blk, want in shapes():
        assert len(blk) <= 65536
        got = py_walk(blk)
        assert got == (want[0], want[1], list(want[2])), (label, got[:2], want[:2])


def test_host_walk_equals_the_restatement():
    for label, blk, _ in shapes():
        assert host_walk(blk) == py_walk(blk), label


def test_max_count_fits_the_cap():
    """A step advances at least 36 bytes and the last start lies at or below 65536 - 4."""
    cnt, ex, starts = host_walk(MAX_BLOCK)
    assert cnt == 1821 == (65536 - 4) // 36 + 1 and cnt <= CAP
    assert starts == MAX_STARTS and starts[-1] == 65522 and ex == 65558
    # 36-byte records alone are never a first start (l_read_name 1 does not fit a block_size of 32)
    assert host_walk((HEADER36 * 1821)[:65536]) == (0, NO_EXIT, [])


def test_host_walk_on_cut_and_damaged_stream():
    """Random cuts of a record stream, a third with a few bytes overwritten: the restatement's lists."""
    S, _, _ = stream(300, seed=9)
    rng = np.random.default_rng(21)
    for k in range(120):
        a = int(rng.integers(0, len(S) - 40))
        blk = bytearray(S[a:a + int(rng.integers(1, 3000))])
        if k % 3 == 0:
            for _ in range(int(rng.integers(1, 5))):
                blk[int(rng.integers(0, len(blk)))] = int(rng.integers(0, 256))
        assert host_walk(bytes(blk)) == py_walk(bytes(blk)), k


def test_host_walk_arguments():
    L = N.lib()
    c, e = ctypes.c_uint32(), ctypes.c_uint32()
    row = np.zeros(CAP, np.uint16)
    buf = np.zeros(65537, np.uint8)
    assert L.fc2_bam_walk_host(buf.ctypes.data, 65537, row.ctypes.data, ctypes.byref(c), ctypes.byref(e)) == N.FC2_E_RANGE
    assert L.fc2_bam_walk_host(None, 5, row.ctypes.data, ctypes.byref(c), ctypes.byref(e)) == N.FC2_E_PARAM
    assert L.fc2_bam_walk_host(buf.ctypes.data, 5, None, ctypes.byref(c), ctypes.byref(e)) == N.FC2_E_PARAM
    assert L.fc2_ingest_set_gpu_walk(None, 1) == N.FC2_E_PARAM
    assert L.fc2_ingest_walk_counts(None, None, None) == N.FC2_E_PARAM
