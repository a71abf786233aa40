"""The inputs that the tests of the compressor's level 2 share (test_deflate_model2.py on the CPU,
test_gpu_deflate_model2.py on the GPU): one named input per branch of the level-2 search
(deflate_model2.py's `without` names), and a FASTQ in the shape of spliced_reads.fastq -- many reads per
junction -- whose redundancy level 1's single probe does not find."""
from functools import lru_cache

import numpy as np

from deflate_model2 import model2


def _filler(rng, n, lo=0, hi=64):
    """n bytes of 64 values: four of them seldom repeat by chance, and a block of them is worth compressing."""
    return bytes(rng.integers(lo, hi, n, dtype=np.uint8))


def _steps(rng, heads):
    """One step of 64 bytes per head: the head, then filler (no two occurrences of a head share a step, so
    each is the candidate after the other)."""
    return b"".join(h + _filler(rng, 64 - len(h)) for h in heads)


def chain8(seed=3):
    """Nine steps that begin with ABCD: the last repeats the first's next 20 bytes, the seven between go on
    otherwise -- the 8th candidate is the one worth having."""
    rng = np.random.default_rng(seed)
    x = b"ABCD" + _filler(rng, 20, 128, 192)
    return _steps(rng, [x] + [b"ABCD" + bytes([200 + k]) for k in range(7)] + [x])


def nearer_shorter(seed=4):
    """ABCD + 20 bytes, ABCD + the first 3 of them, and ABCD + the 20 again: the nearer candidate fits for
    7 bytes, the farther for 24."""
    rng = np.random.default_rng(seed)
    x = b"ABCD" + _filler(rng, 20, 128, 192)
    return _steps(rng, [x, x[:7] + b"\xc8", x])


def nice_stop(seed=5):
    """As nearer_shorter with 60 and 40 bytes: the nearer candidate's 44 bytes end the walk, and the
    farther one's 64 are never seen."""
    rng = np.random.default_rng(seed)
    x = b"ABCD" + _filler(rng, 60, 128, 192)
    return _steps(rng, [x, x[:44] + b"\xc8", x])


def lazy_at(at, seed=6):
    """QABCD+ in one step, ABCDEFGHIJ in the next, and QABCDEFGHIJ at position `at` of the text (in a later
    step): a match of 5 at `at`, one of 10 at `at` + 1."""
    rng = np.random.default_rng(seed)
    assert at >= 128
    text = _steps(rng, [b"QABCD+", b"ABCDEFGHIJ"]) + _filler(rng, at - 128) + b"QABCDEFGHIJ"
    return text + _filler(rng, -len(text) % 64 + 64)


def window_edge(seed=8):
    """65536 bytes of 0..255 over and over (256 four-byte words in all, so that the table's other entries
    keep what is planted) with two pieces of 40 random bytes, each planted twice: the lane 0 of 40000's step
    repeats one from 32736 back, whose link slot the step itself rewrites (the walk ends there), and the lane
    63 of 50000's step the other from 32767 back, the farthest source that lane may use."""
    rng = np.random.default_rng(seed)
    a = bytearray(bytes(range(256)) * 256)
    p = 40000 // 64 * 64
    q = 50000 // 64 * 64 + 63
    for at, back in ((p, 32736), (q, 32767)):
        a[at:at + 40] = a[at - back:at - back + 40] = bytes(rng.integers(0, 256, 40, dtype=np.uint8))
    return bytes(a), p, q


def planted_fastq(n, k, seed=12):
    """n bytes of FASTQ: reads of 100 bases, each a window at a random offset of one of k junction sequences
    of 160 random bases, three in ten with one base substituted; names @sim_%07d/1; qualities
    33 + min(40, geometric(0.15))."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    junctions = acgt[rng.integers(0, 4, (k, 160))]
    out, size, i = [], 0, 0
    while size < n:
        off = int(rng.integers(0, 61))
        seq = junctions[int(rng.integers(0, k)), off:off + 100].copy()
        if rng.random() < 0.3:
            at = int(rng.integers(0, 100))
            seq[at] = acgt[(int(np.nonzero(acgt == seq[at])[0][0]) + int(rng.integers(1, 4))) % 4]
        qual = (33 + np.minimum(40, rng.geometric(0.15, 100))).astype(np.uint8)
        rec = b"@sim_%07d/1\n" % i + seq.tobytes() + b"\n+\n" + qual.tobytes() + b"\n"
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n]


NAMED2 = {
    "chain8": chain8,                                    # 576 bytes
    "nearer_shorter": nearer_shorter,                    # 192 bytes
    "nice_stop": nice_stop,
    "lazy": lambda: lazy_at(150),
    "lazy_not_across_steps": lambda: lazy_at(191),       # the match of 5 at lane 63, the one of 10 at the next step's lane 0
    "window_edge": lambda: window_edge()[0],
    "wrapped_links": lambda: planted_fastq(32768 + 65, 20),
}
# the branch each is there for (deflate_model2's `without`)
BRANCH2 = {"chain8": "depth", "nearer_shorter": "depth", "nice_stop": "nice", "lazy": "lazy", "window_edge": "window"}


@lru_cache(maxsize=None)
def named2(name):
    data = NAMED2[name]()
    return (data,) + model2(data)
