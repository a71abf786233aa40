"""The inputs that the tests of level 2's search effort share (test_deflate_model_deep.py on the CPU,
test_gpu_deflate_deep.py on the GPU): one input per branch that `depth` and `nice` open (deflate_model_deep.py), and
a stream of BAM records in the shape of the steady-state generator's spliced reads (scripts/gen_reads.c).

Every planted input is built around a key of four bytes and made so that the key's positions are the only ones in
the key's bucket of the 12-bit table of heads -- the filler is drawn again until that holds -- so the bucket's chain
is the planted occurrences and nothing else, and "the k-th candidate" is the k-th occurrence back."""
import struct
from functools import lru_cache

import numpy as np

from deflate_model import HASH_BITS

KEY = b"ABCD"


def bucket(word: bytes) -> int:
    return ((int.from_bytes(word, "little") * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def key_positions(text: bytes, key: bytes = KEY):
    """The positions whose four bytes fall into the key's bucket, and whether they all are the key."""
    v = np.frombuffer(text + bytes(3), np.uint8).astype(np.uint32)
    w = v[:-3] | v[1:-2] << 8 | v[2:-1] << 16 | v[3:] << 24
    at = np.nonzero((w * np.uint32(2654435761)) >> np.uint32(32 - HASH_BITS) == bucket(key))[0]
    at = [int(p) for p in at if p + 4 <= len(text)]
    return at, all(text[p:p + 4] == key for p in at)


def _clean(build, want):
    """build(rng) for the first seed that leaves exactly `want` positions in the key's bucket, all of them the key."""
    for seed in range(200):
        text = build(np.random.default_rng(1000 + seed))
        at, pure = key_positions(text)
        if pure and len(at) == want:
            return text
    raise AssertionError("no seed keeps the key's bucket to the key")


def _filler(rng, n, lo=0, hi=64):
    return bytes(rng.integers(lo, hi, n, dtype=np.uint8))


def bucket33(k):
    """33 steps of 64 bytes that begin with ABCD, then one more at position 33 * 64 whose 24 bytes after ABCD repeat
    those of the occurrence k candidates back (k = 1: the nearest, position 32 * 64; k = 33: position 0) and of no
    other: every other occurrence goes on with a byte of its own.  A walk of k candidates finds a match of 28 at
    distance 64 * k; a shorter walk finds matches of 4.  Returns (text, the searching position, the distance)."""
    assert 1 <= k <= 33

    def build(rng):
        tail = _filler(rng, 24, 128, 192)
        steps = [KEY + (tail + b"\xf0" if i == 33 - k else bytes([200 + i])) for i in range(33)] + [KEY + tail + b"\xf1"]
        return b"".join(s + _filler(rng, 64 - len(s)) for s in steps)

    return _clean(build, 34), 33 * 64, 64 * k


def nice40_120():
    """ABCD + 116 bytes; four steps on ABCD + the first 36 of them; four steps on ABCD + the 116 again: for the last,
    the nearest candidate fits for 40 bytes and the one behind it for 120.  At nice 32 the 40 end the walk; at nice
    258 (or anything over 40) the 120 are found.  Returns (text, the searching position, the two distances)."""
    def build(rng):
        tail = _filler(rng, 116, 128, 192)
        parts = [KEY + tail + b"\xc9", KEY + tail[:36] + b"\xc8", KEY + tail + b"\xca"]
        return b"".join(p + _filler(rng, 256 - len(p)) for p in parts)

    return _clean(build, 3), 512, (256, 512)


def stale_chain():
    """65536 bytes of two letters (16 four-byte words in all: the table's other buckets keep to themselves) with ABCD
    every 1024 bytes from position 500 on, 64 occurrences.  The last one, at 65012, and the one exactly 32768 before
    it, at 32244, go on with the same 100 bytes; the others with filler.  As the second tile of a launch with tile
    32768 and hist 32768 (a region of 65536 bytes) position 65012 walks 31 candidates, each 1024 further back, and the
    32nd is 32768 back: its link slot is the one position 65012 itself has just rewritten, and the walk ends there
    -- only a walk of 32 or more gets that far.  Returns (text, tile, hist, the searching position)."""
    def build(rng):
        a = bytearray(np.frombuffer(b"xy", np.uint8)[rng.integers(0, 2, 65536)].tobytes())
        tail = _filler(rng, 100, 128, 192)
        for i in range(64):
            p = 500 + 1024 * i
            a[p:p + 4] = KEY
            if i in (31, 63):
                a[p + 4:p + 104] = tail
        return bytes(a)

    return _clean(build, 64), 32768, 32768, 500 + 1024 * 63


def bam_records(n, seed=7):
    """n bytes of BAM records shaped like the steady-state generator's spliced reads (scripts/gen_reads.c): names
    s%d numbered among the six in ten unspliced reads that are not written; a primary record kM(100-k)S with 100
    bases, QUAL all 40 and AS:C XS:C tags; behind it the hard-clipped supplementary kH(100-k)M with the read's last
    100 - k bases, no QUAL (0xff) and an AS:C tag.  Three chromosomes; bases drawn at random."""
    rng = np.random.default_rng(seed)
    lens = (6000000, 5000000, 4000000)
    out, size, i = [], 0, 0

    def record(ref, pos, name, flag, cigar, bases, qual, tags):
        l_seq = len(bases)
        packed = bytearray((l_seq + 1) // 2)
        for j, b in enumerate(bases):
            packed[j >> 1] |= (1, 2, 4, 8)[b] << (0 if j & 1 else 4)
        body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, 60, 4681 + (pos >> 14), len(cigar), flag, l_seq, -1, -1, 0)
        body += name + b"\0" + b"".join(struct.pack("<I", ln << 4 | op) for ln, op in cigar) + bytes(packed) + qual + tags
        return struct.pack("<i", len(body)) + body

    while size < n:
        i += 1
        if rng.random() < 0.6:
            continue
        ref = int(rng.integers(0, 3))
        k = int(rng.integers(20, 81))
        span = int(rng.integers(200, 20000))
        a_pos = int(rng.integers(1000, lens[ref] - 30000))
        bases = rng.integers(0, 4, 100)
        name = b"s%d" % i
        recs = record(ref, a_pos, name, 0, [(k, 0), (100 - k, 4)], bases, bytes([40]) * 100,
                      b"ASC" + bytes([k]) + b"XSC" + bytes([int(rng.integers(0, 12))]))
        recs += record(ref, a_pos + span, name, 2048, [(k, 5), (100 - k, 0)], bases[k:], b"\xff" * (100 - k),
                       b"ASC" + bytes([100 - k]))
        out.append(recs)
        size += len(recs)
    return b"".join(out)[:n]


@lru_cache(maxsize=None)
def named_deep(name):
    return {"bucket33_9": lambda: bucket33(9), "bucket33_33": lambda: bucket33(33), "nice40_120": nice40_120,
            "stale_chain": stale_chain}[name]()
