"""The host model of the GPU DEFLATE compressor (deflate_model.py) on its own, so that "the kernel's
bytes equal the model's" (test_gpu_deflate_model.py) means something: zlib inflates every stream of
the model; each of its three codes, read back from its own stream, is complete, within 15 / 15 / 7
bits, and, where no node was clipped, costs what an independent Huffman build costs; and the inputs
named here reach the branches that ordinary texts leave out, by the model's own counters, and give
other bytes when the model is run without the branch.

Not reached: the overflow repair of the distance code.  It takes some 12,000 matches spread
geometrically over 17 or more distance symbols in one tile, and the compressor's table of 4096 last
positions forgets far sources long before; it is the same build_code as the literal/length code's,
with the same limit of 15, which the inputs below do reach."""
import heapq
import math
import zlib
from functools import lru_cache

import numpy as np
import pytest

from deflate_helpers import _DBASE, _LBASE, CONTENTS, deflate_blocks, explain
from deflate_model import model

GRID_LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 67, 68, 257, 258, 259, 4096, 32767, 32768, 65536]


# ---- the named inputs: each from a seed, none over 65536 bytes ------------------------------------------
def geometric(ratio, nsym, seed, values=None):
    """nsym byte values, the j-th ceil(ratio ** j) times, shuffled: a literal/length tree that is a
    chain, deeper than 15."""
    rng = np.random.default_rng(seed)
    values = rng.permutation(256)[:nsym] if values is None else values[:nsym]
    a = np.repeat(np.asarray(values, np.uint8), [math.ceil(ratio ** j) for j in range(nsym)])
    rng.shuffle(a)
    return a.tobytes()


def dyadic511(seed):
    """511 bytes whose counts are powers of two: 1, 2, 4, 7, 13, 23 and 165 byte values with code lengths
    3 .. 9 (the end of the block is the 166th of the nines), so the code lengths' own code has seven
    symbols in use with counts near 1, 2, 4, 7, 13, 23, 166: a chain again, deeper than 7."""
    rng = np.random.default_rng(seed)
    values, out, k = rng.permutation(256), [], 0
    for bits, count in {3: 1, 4: 2, 5: 4, 6: 7, 7: 13, 8: 23, 9: 165}.items():
        for _ in range(count):
            out += [values[k]] * 2 ** (9 - bits)
            k += 1
    a = np.array(out, np.uint8)
    rng.shuffle(a)
    return a.tobytes()


def far_copies(seed, k=40):
    """k blocks of 131 .. 257 rare bytes, some 16700 bytes of a skewed text, and the blocks again: matches
    whose length takes 5 extra bits and whose distance takes 13, with rare symbols for both."""
    rng = np.random.default_rng(seed)
    values = rng.permutation(256)
    common, rare = values[:15], values[15:]
    blocks = [bytes(rare[rng.integers(0, len(rare), int(rng.integers(131, 258)))].astype(np.uint8)) for _ in range(k)]
    first = b"".join(b + bytes([common[0]]) for b in blocks)
    again = b"".join(b + bytes([common[1]]) for b in blocks)
    # at distance 24500: symbol 28, and the top bits of its 13 extra bits are ones
    return first + geometric(2.0, 15, seed, common)[:24500 - len(first)] + again


def sixteen(seed, n=1000):
    return bytes(np.random.default_rng(seed).integers(0, 16, n, dtype=np.uint8))


NAMED = {
    "ll_overflow_1.7": lambda: geometric(1.7, 19, 1),     # 34161 bytes
    "ll_overflow_2.0": lambda: geometric(2.0, 16, 0),     # 65535 bytes
    "cl_overflow": lambda: dyadic511(2),
    "no_match": lambda: CONTENTS["acgt"](64),             # one step: nothing to refer to
    "distance_one_only": lambda: bytes(164),              # one match, at distance 1
    "one_literal": lambda: bytes(4096),
    "length_runs": lambda: sixteen(2),
    "three_word": lambda: far_copies(9),                  # 32309 bytes
    "flushes": lambda: CONTENTS["acgt"](32768),
}
# the branch that each named input is there for (deflate_model's `without`)
BRANCH = {
    "ll_overflow_1.7": "repair", "ll_overflow_2.0": "repair", "cl_overflow": "repair", "no_match": "dummy",
    "distance_one_only": "dummy", "length_runs": ("cap138", "rep16"), "three_word": "w2", "flushes": "keep",
}


@lru_cache(maxsize=None)
def named(name):
    data = NAMED[name]()
    return (data,) + model(data)


@lru_cache(maxsize=None)
def grid(content, n):
    data = CONTENTS[content](n)
    assert len(data) == n
    return (data,) + model(data)


def test_model_crc_is_zlibs():
    for name in sorted(NAMED):
        data, stream, info = named(name)
        assert info["crc"] == zlib.crc32(data), name


def _inflates(stream, data):
    z = zlib.decompressobj(-15)
    got = z.decompress(stream)
    assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b""
    assert got == data


# ---- zlib accepts the stream ----------------------------------------------------------------------------
@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_model_streams_inflate(content):
    for n in GRID_LENGTHS:
        data, stream, info = grid(content, n)
        _inflates(stream, data)
        assert len(stream) <= n + (10 if n == 65536 else 5), (n, info["kind"])


@pytest.mark.parametrize("name", sorted(NAMED))
def test_model_named_streams_inflate(name):
    data, stream, info = named(name)
    assert len(data) <= 65536
    _inflates(stream, data)


# ---- the codes are optimal ------------------------------------------------------------------------------
def _huffman_cost(freqs):
    """sum(freq * depth) of a Huffman tree over the frequencies: the sum of the inner nodes' weights,
    the same however ties are broken."""
    h = list(freqs)
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        s = heapq.heappop(h) + heapq.heappop(h)
        cost += s
        heapq.heappush(h, s)
    return cost


def _length_symbol(n):
    return 257 + max(i for i, b in enumerate(_LBASE) if b <= n) if n < 258 else 285


def _distance_symbol(d):
    return max(i for i, b in enumerate(_DBASE) if b <= d)


def _check_codes(stream, clipped):
    """The three codes of a dynamic stream, by what the stream itself says."""
    tokens, _, blocks = deflate_blocks(stream)
    assert len(blocks) == 1 and blocks[0][0] == "dynamic"
    _, ll, dl, cl, hclen, sent = blocks[0]
    lf, df, cf = [0] * 286, [0] * 30, [0] * 19
    lf[256] = 1
    for t in tokens:
        if t[0] == "lit":
            lf[t[1]] += 1
        else:
            lf[_length_symbol(t[1])] += 1
            df[_distance_symbol(t[2])] += 1
    for s in sent:
        cf[s] += 1
    for what, lens, freq, limit, clip in (("literal/length", ll, lf, 15, clipped[0]), ("distance", dl, df, 15, clipped[1]),
                                          ("code length", cl, cf, 7, clipped[2])):
        used = [l for l in lens if l]
        assert sum(2 ** (limit - l) for l in used) == 2 ** limit, what + " code not complete"
        assert max(used) <= limit, what
        assert all(lens[s] for s in range(len(freq)) if freq[s]), what + ": a symbol in use has no codeword"
        # a symbol with a codeword and no use is a dummy one, counted once as the compressor counts it
        weights = [(freq[s] or 1, l) for s, l in enumerate(lens) if l]
        cost = sum(f * l for f, l in weights)
        best = _huffman_cost([f for f, _ in weights])
        assert cost >= best, what
        if clip == 0:
            assert cost == best, "%s code costs %d bits, a Huffman code %d" % (what, cost, best)
    return max(ll), max(dl), max(cl)


@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_model_codes_are_optimal(content):
    seen = 0
    for n in GRID_LENGTHS:
        data, stream, info = grid(content, n)
        if info["kind"] == "dynamic":
            assert _check_codes(stream, info["clipped"]) == info["maxlen"]
            seen += 1
    assert seen or content == "random"


@pytest.mark.parametrize("name", sorted(NAMED))
def test_model_named_codes_are_optimal(name):
    data, stream, info = named(name)
    assert info["kind"] == "dynamic"
    assert _check_codes(stream, info["clipped"]) == info["maxlen"]


def test_model_stored_forms():
    for n in (65535, 65536):
        data, (stream, info) = CONTENTS["random"](n), model(CONTENTS["random"](n))
        assert info["kind"] == "stored"
        _inflates(stream, data)
        tokens, size, blocks = deflate_blocks(stream)
        assert tokens == ([("stored", 65535)] if n == 65535 else [("stored", 65535), ("stored", 1)])


# ---- named inputs reach the named paths -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["ll_overflow_1.7", "ll_overflow_2.0"])
def test_path_literal_length_overflow(name):
    data, stream, info = named(name)
    assert info["kind"] == "dynamic" and info["clipped"][0] > 0 and info["maxlen"][0] == 15, info["clipped"]


def test_path_code_length_code_overflow():
    data, stream, info = named("cl_overflow")
    assert len(data) == 511
    assert info["kind"] == "dynamic" and info["clipped"][2] > 0 and info["maxlen"][2] == 7, info["clipped"]


def test_path_single_distance_code():
    """No match: both dummy distance symbols, each with one bit; the header's HDIST field (the number
    of distance lengths less 1) is 1."""
    data, stream, info = named("no_match")
    assert info["kind"] == "dynamic" and not [t for t in info["tokens"] if isinstance(t, tuple)]
    assert info["hdist"] - 1 == 1 and info["dfreq"][:2] == [1, 1] and sum(info["dfreq"]) == 2
    _, _, blocks = deflate_blocks(stream)
    assert blocks[0][2] == [1, 1]
    # and one distance symbol in use, symbol 0: only symbol 1 is a dummy
    data, stream, info = named("distance_one_only")
    assert info["kind"] == "dynamic" and [t for t in info["tokens"] if isinstance(t, tuple)] == [("m", 100, 1)]
    assert info["dfreq"][:2] == [1, 1] and sum(info["dfreq"]) == 2


def test_path_one_literal_and_matches():
    data, stream, info = named("one_literal")
    assert info["kind"] == "dynamic"
    assert {t for t in info["tokens"] if not isinstance(t, tuple)} == {0}
    assert len([t for t in info["tokens"] if isinstance(t, tuple)]) >= 2


def test_path_length_runs_split():
    data, stream, info = named("length_runs")
    rle = info["rle"]
    assert info["kind"] == "dynamic"
    # a run of zeros over 138: symbol 18 for 138 of them, and 18 again for the rest
    assert [k for k in range(len(rle) - 1) if rle[k] == (18, 127) and rle[k + 1][0] == 18]
    # a run of one length of 7 or more: the length, symbol 16 for six more, and the run goes on
    assert [k for k in range(1, len(rle) - 1) if rle[k - 1][0] < 16 and rle[k] == (16, 3) and
            rle[k + 1][0] in (16, rle[k - 1][0])]
    assert deflate_blocks(stream)[2][0][5] == [s for s, _ in rle]


def test_path_three_word_token():
    data, stream, info = named("three_word")
    assert info["kind"] == "dynamic" and info["widest"] >= 34
    assert info["three_word"] > 0                                  # a = 0
    assert [a for a in range(1, 16) if model(data, a=a)[1]["three_word"] > 0][:3] == [1, 2, 3]


def test_path_flushes():
    data, stream, info = named("flushes")
    assert info["kind"] == "dynamic" and info["flushes"] >= 3
    for a in (1, 7, 15):
        s, i = model(data, a=a)
        assert s == stream and i["flushes"] >= 3
    assert named("ll_overflow_2.0")[2]["flushes"] >= 3


@pytest.mark.parametrize("name", sorted(BRANCH))
def test_model_without_the_branch_gives_other_bytes(name):
    """What makes equality with the model bite: on the input that reaches a branch, a compressor
    without the branch writes other bytes."""
    data, stream, info = named(name)
    branches = BRANCH[name] if isinstance(BRANCH[name], tuple) else (BRANCH[name],)
    for b in branches:
        assert model(data, without=(b,))[0] != stream, b
    if name == "three_word":                                       # at the other alignments too
        for a in (1, 2, 3):
            assert model(data, a=a, without=("w2",))[0] != stream, a
    # ... and the same bytes where the input does not reach it
    plain = CONTENTS["fastq"](4096)
    for b in branches:
        if b not in ("rep16",):                                    # (any text has a run of equal lengths)
            assert model(plain, without=(b,))[0] == model(plain)[0], b


def test_explain_names_the_stage():
    """What the GPU tests say when the kernel's stream is not the model's."""
    data = CONTENTS["fastq"](3000)
    want = model(data)[0]
    assert explain(want, want) is None
    assert explain(model(CONTENTS["random"](3000))[0], want).startswith("kind")
    assert explain(model(data[:-1] + b"!")[0], want).startswith("tokens")
    assert explain(want[:-1] + bytes([want[-1] ^ 0x80]), want).startswith("bytes")
    # the same tokens and codes, the lengths sent without symbol 16: another code for the lengths
    assert explain(model(data, without=("rep16",))[0], want).startswith("code length code lengths")
    assert explain(b"\x07", want).startswith("the kernel's stream cannot be read")     # (block type 3)
