"""Hand-built BAM record streams, their block tables and an independent restatement of the fragment-row
rule (include/fc2_ingest.h fc2_bam_frag), shared by test_bam_frag_host.py and test_gpu_bam_frag.py.

A stream is a list of scenarios, each a run of records with a label on its head, with single-record filler
fragments between them so that every scenario has a mapped record of another name before and after it.
The stream is cut into blocks of 1-4 KB whose record starts are listed by fc2_bam_walk_host, block by
block, as the device lists them."""
import ctypes
import functools
import struct

import numpy as np

from find_circ2_amd import _native as N
from test_bam_digest_host import py_digest

CAP = N.BAM_WALK_CAP
FRAG = np.dtype([("state", "u1"), ("n_records", "u1"), ("n_mates", "u1"), ("n_unmapped", "u1"), ("bytes", "<u4")])
assert FRAG.itemsize == 8 == ctypes.sizeof(N.BamFrag)


def rec(name, flag=0, ref=0, pos=100, bad_tag=False, l_seq=20):
    """One BAM record (block_size and body): 20M, AS:i; bad_tag: the tag's type is one BAM does not know."""
    qn = name.encode() + b"\0"
    cig = struct.pack("<I", (l_seq << 4) | 0)
    seq = bytes(0x12 for _ in range((l_seq + 1) // 2))
    qual = bytes(30 for _ in range(l_seq))
    tags = b"AS" + (b"?" if bad_tag else b"i") + struct.pack("<i", l_seq)
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(qn), 60, 4681, 1, flag, l_seq, -1, -1, 0) + qn + cig + seq + qual + tags
    return struct.pack("<I", len(body)) + body


R1, R2, REV, UNMAPPED, SUPP = 0x41, 0x81, 0x10, 0x4, 0x800

# (label, records, expected row of the head as (state, n_records, n_mates, n_unmapped) or None for state 0);
# a record is (name, flag, ref) or (name, flag, ref, bad_tag)
SCENARIOS = [
    ("single", [("a1", 0, 0)], (1, 1, 1, 0)),
    ("pair", [("b1", R1, 0), ("b1", R2, 0)], (1, 2, 2, 0)),
    ("proper supplementary", [("c1", 0, 0), ("c1", SUPP, 0)], None),
    ("supplementary on another refID", [("d1", 0, 0), ("d1", SUPP, 1)], (1, 2, 1, 0)),
    ("supplementary on the other strand", [("e1", 0, 0), ("e1", SUPP | REV, 0)], (1, 2, 1, 0)),
    ("reverse head, reverse supplementary", [("e2", REV, 0), ("e2", SUPP | REV, 0)], None),
    ("unmapped inside", [("g1", R1, 0), ("g1", R2 | UNMAPPED, 0), ("zz", UNMAPPED, -1), ("g1", R1 | SUPP, 2)], (1, 4, 1, 2)),
    ("pair, mate 2 proper", [("p1", R1, 0), ("p1", R2, 1), ("p1", R2 | SUPP, 1)], None),
    ("pair, mate 2's segment like mate 1's primary", [("p2", R1, 0), ("p2", R2, 1), ("p2", R2 | SUPP, 0)], (1, 3, 2, 0)),
    ("third mate", [("t1", R1, 0), ("t1", R2, 0), ("t1", R1, 1)], None),
    ("4 unmapped behind it", [("h0", 0, 0)] + [("u%d" % k, UNMAPPED, -1) for k in range(4)], (1, 5, 1, 4)),
    ("right after 4 unmapped, 5 behind it", [("h1", 0, 0)] + [("v%d" % k, UNMAPPED, -1) for k in range(5)], (1, 6, 1, 5)),
    ("right after 5 unmapped", [("h2", 0, 0)], None),
    ("16 records", [("s16", 0, 0)] + [("s16", SUPP, 1)] * 15, (1, 16, 1, 0)),
    ("17 records", [("s17", 0, 0)] + [("s17", SUPP, 1)] * 16, None),
    ("r1", [("r1", 0, 0)], (1, 1, 1, 0)),
    ("r10", [("r10", 0, 0)], (1, 1, 1, 0)),
    ("a name that continues r10, with a proper supplementary", [("r100", 0, 0), ("r100", SUPP, 0)], None),
    ("xa", [("xa", 0, 0)], (1, 1, 1, 0)),
    ("xb", [("xb", 0, 0)], (1, 1, 1, 0)),
    ("invalid record inside", [("k1", 0, 0), ("k1", SUPP, 1, True)], None),
    ("after an invalid record", [("k2", 0, 0)], None),
    ("invalid record closes it", [("m1", 0, 0)], None),
    ("the invalid closer", [("m2", 0, 0, True)], None),
    ("after the invalid closer", [("m3", 0, 0)], None),
]
# scenarios that must follow the one before them without a filler between
GLUED = {"right after 4 unmapped, 5 behind it", "right after 5 unmapped", "r10", "xb", "after an invalid record", "the invalid closer", "after the invalid closer"}


@functools.lru_cache(maxsize=None)
def stream(shift=0):
    """(bytes, {label: offset of the scenario's head}): the scenarios with fillers; `shift` lengthens the
    first record's name, so every later start moves to another residue mod 4."""
    out, heads, n_fill = bytearray(), {}, 0
    def filler():
        nonlocal n_fill
        out.extend(rec("f%04d" % n_fill + "x" * (shift if n_fill == 0 else 0), 0, n_fill % 3))
        n_fill += 1
    for label, recs, _ in SCENARIOS:
        if label not in GLUED:
            filler()
        heads[label] = len(out)
        for r in recs:
            out.extend(rec(r[0], r[1], r[2], bad_tag=len(r) > 3))
    for _ in range(3):
        filler()
    return bytes(out), heads


class Tables:
    """The launch's tables for a stream cut into blocks (numpy arrays, host memory)."""
    def __init__(self, data, cuts):
        self.data = np.frombuffer(data, np.uint8).copy()
        self.n_bytes = len(data)
        edges = [0] + list(cuts) + [len(data)]
        self.n_blocks = nb = len(edges) - 1
        self.ooff = np.array(edges[:-1], np.uint32)
        self.isize = np.diff(np.array(edges, np.int64)).astype(np.uint32)
        self.status = np.zeros(nb, np.uint32)
        self.starts = np.zeros((nb, CAP), np.uint16)
        self.count = np.zeros(nb, np.uint32)
        L = N.lib()
        for j in range(nb):
            blk = self.data[edges[j]:edges[j + 1]].copy()
            c, ex = ctypes.c_uint32(), ctypes.c_uint32()
            N.check(L.fc2_bam_walk_host(blk.ctypes.data, len(blk), self.starts[j].ctypes.data, ctypes.byref(c), ctypes.byref(ex)))
            self.count[j] = c.value

    def first(self):
        return np.concatenate([[0], np.cumsum(np.minimum(self.count, CAP))]).astype(np.uint32)

    def listed(self):
        """[(block, k, stream offset)] in the order of the lists."""
        return [(j, k, int(self.ooff[j]) + int(self.starts[j, k])) for j in range(self.n_blocks)
                for k in range(min(int(self.count[j]), CAP))]


def random_cuts(n, rng, lo=1000, hi=4000):
    cuts, o = [], 0
    while True:
        o += int(rng.integers(lo, hi + 1))
        if o >= n:
            return cuts
        cuts.append(o)


def host_rows(T):
    """fc2_bam_frag_host over the tables: (rows as a FRAG array, first)."""
    first = np.zeros(T.n_blocks + 1, np.uint32)
    total = int(T.first()[-1])
    rows = np.full(total + 2, 0xA5A5A5A5A5A5A5A5, np.uint64).view(FRAG)       # a guard row either side
    N.check(N.lib().fc2_bam_frag_host(T.data.ctypes.data, T.n_bytes, T.ooff.ctypes.data, T.isize.ctypes.data,
                                      T.status.ctypes.data, T.starts.ctypes.data, T.count.ctypes.data,
                                      rows[1:].ctypes.data, first.ctypes.data, T.n_blocks))
    assert (rows[[0, -1]].view(np.uint64) == 0xA5A5A5A5A5A5A5A5).all(), "a row outside the counted ones was written"
    assert (first == T.first()).all()
    return rows[1:-1].copy(), first


# ---- the rule, restated ---------------------------------------------------------------------------
def py_rows(T):
    """Every listed start's fragment row as (state, n_records, n_mates, n_unmapped, bytes) tuples."""
    d = T.data.tobytes()
    L = T.listed()
    index = {at: i for i, (_, _, at) in enumerate(L)}
    ends = [int(x) for x in T.ooff[1:]] + [T.n_bytes]

    def fields(i):
        """None unless the i-th listed record is usable; else its (at, end, flag, refID, name)."""
        j, _, at = L[i]
        row = py_digest(d, T.n_bytes, at)
        if row[0] != 1:
            return None
        end = at + 4 + row[4]
        for b in range(j, T.n_blocks):
            if b > j and int(T.ooff[b]) >= end:
                break
            if T.status[b] != 0:
                return None
        ref, _pos, l_name, _mq, _bin, _nc, flag = struct.unpack_from("<iiBBHHH", d, at + 4)
        return at, end, flag, ref, (l_name, d[at + 36:at + 36 + l_name - 1])

    F = [fields(i) for i in range(len(L))]
    rows = []
    for i, H in enumerate(F):
        row = (0, 0, 0, 0, 0)
        rows.append(row)
        if H is None or H[2] & 4:
            continue
        # back: at most 4 unmapped records, then a mapped one of another name, each ending where the next starts
        k, at, ok = i, H[0], False
        for step in range(5):
            k -= 1
            if k < 0 or F[k] is None or F[k][1] != at:
                break
            at = F[k][0]
            if F[k][2] & 4:
                continue
            ok = F[k][4] != H[4]
            break
        if not ok:
            continue
        # forward
        n_rec, n_unm, mates, cur, closed = 1, 0, [(H[2], H[3])], H, None
        bad = False
        while True:
            k = index.get(cur[1])
            if k is None or F[k] is None:
                bad = True
                break
            cur = F[k]
            if not cur[2] & 4 and cur[4] != H[4]:
                closed = cur
                break
            n_rec += 1
            if n_rec > N.BAM_FRAG_CAP:
                bad = True
                break
            if cur[2] & 4:
                n_unm += 1
                continue
            pf, pr = mates[-1]
            if (cur[2] & 0x40) == (pf & 0x40):
                if cur[3] == pr and (cur[2] & 0x10) == (pf & 0x10):
                    bad = True
                    break
            elif len(mates) == 2:
                bad = True
                break
            else:
                mates.append((cur[2], cur[3]))
        if not bad:
            rows[-1] = (1, n_rec, len(mates), n_unm, closed[0] - H[0])
    return rows


def as_tuples(rows):
    return [tuple(int(x) for x in r.item()) for r in rows]
