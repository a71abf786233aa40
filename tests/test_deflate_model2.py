"""The host model of the GPU compressor's level 2 (deflate_model2.py) on its own, as
test_deflate_model.py is for level 1: zlib inflates its streams, its codes cost what an independent
Huffman build costs, every branch of the level-2 search is reached by a named input that gives other
bytes without it, and -- kernel and model being equal (test_gpu_deflate_model2.py) -- what level 2 buys
in size is decided here: never more bytes than level 1 on the contents grid, and at most 0.90 of
level 1 on a FASTQ with many reads per junction."""
import zlib

import pytest

from deflate2_inputs import BRANCH2, NAMED2, named2, planted_fastq, window_edge
from deflate_helpers import CONTENTS
from deflate_model import model
from deflate_model2 import model2
from test_deflate_model import GRID_LENGTHS, _check_codes, _inflates, grid


def _matches(info):
    """{position: (length, distance)} of the tokens."""
    out, pos = {}, 0
    for t in info["tokens"]:
        if isinstance(t, tuple):
            out[pos] = (t[1], t[2])
            pos += t[1]
        else:
            pos += 1
    return out


# ---- zlib accepts the streams, and the codes are optimal ------------------------------------------------
@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_model2_grid_streams_inflate_codes_optimal_and_no_larger_than_level_1(content):
    seen = 0
    for n in GRID_LENGTHS:
        data, level1, _ = grid(content, n)
        stream, info = model2(data)
        _inflates(stream, data)
        assert info["crc"] == zlib.crc32(data)
        assert len(stream) <= len(level1), (n, len(stream), len(level1))
        if info["kind"] == "dynamic":
            assert _check_codes(stream, info["clipped"]) == info["maxlen"]
            seen += 1
    assert seen or content == "random"


@pytest.mark.parametrize("name", sorted(NAMED2))
def test_model2_named_streams_inflate_and_codes_are_optimal(name):
    data, stream, info = named2(name)
    assert len(data) <= 65536 and info["kind"] == "dynamic"
    _inflates(stream, data)
    assert _check_codes(stream, info["clipped"]) == info["maxlen"]


# ---- the named inputs reach the named branches ----------------------------------------------------------
def test_path_eighth_candidate():
    data, stream, info = named2("chain8")
    assert len(data) == 576 and info["l2"]["deep"] == 1
    assert _matches(info)[512] == (24, 512)
    assert _matches(model2(data, without=("depth",))[1]).get(512, (0, 0))[0] < 24


def test_path_farther_longer_candidate():
    data, stream, info = named2("nearer_shorter")
    assert info["l2"]["farther"] >= 1
    assert _matches(info)[128] == (24, 128)
    assert _matches(model2(data, without=("depth",))[1])[128] == (7, 64)


def test_path_walk_ends_at_32():
    data, stream, info = named2("nice_stop")
    assert info["l2"]["nice"] >= 1
    assert _matches(info)[128] == (44, 64)                          # the first candidate's, 64 back
    assert _matches(model2(data, without=("nice",))[1])[128] == (64, 128)


def test_path_lazy_literal_inside_a_step():
    data, stream, info = named2("lazy")
    m = _matches(info)
    assert info["l2"]["lazy"] == 1 and 150 not in m and m[151] == (10, 151 - 64)
    assert _matches(model2(data, without=("lazy",))[1])[150] == (5, 150)


def test_path_no_lazy_step_across_a_step_boundary():
    """The shorter match at a step's lane 63 and the longer one at the next step's lane 0: positions
    191 / 192, since in the text's first step (63 / 64) nothing has a candidate yet."""
    data, stream, info = named2("lazy_not_across_steps")
    assert info["l2"]["lazy"] == 0 and _matches(info)[191] == (5, 191)
    assert model2(data, without=("lazy",))[0] == stream
    # one position earlier both lie in one step, and the lazy step is taken
    assert named2("lazy")[2]["l2"]["lazy"] == 1


def test_path_window_stop():
    data, p, q = window_edge()
    data, stream, info = named2("window_edge")
    m = _matches(info)
    assert info["l2"]["window"] >= 1
    assert p not in m                                               # 32736 back, the slot rewritten: not looked at
    assert m[q][1] == 32767 and m[q][0] >= 40                       # lane 63 reaches as far as 32767
    assert _matches(model2(data, without=("window",))[1])[p][1] == 32736


def test_path_links_wrap():
    data, stream, info = named2("wrapped_links")
    assert len(data) == 32768 + 65
    assert [p for p in _matches(info) if p >= 32768]                # matches found from the wrapped slots' step on
    assert info["l2"]["deep"] and info["l2"]["lazy"] and info["l2"]["farther"]


@pytest.mark.parametrize("name", sorted(BRANCH2))
def test_model2_without_the_branch_gives_other_bytes(name):
    data, stream, info = named2(name)
    assert model2(data, without=(BRANCH2[name],))[0] != stream
    # ... and level 1's bytes where no input reaches any of them: a text with nothing to refer to
    plain = CONTENTS["acgt"](64)
    assert model2(plain, without=(BRANCH2[name],))[0] == model2(plain)[0] == model(plain)[0]


def test_model2_alignment_changes_no_byte():
    data, stream, info = named2("wrapped_links")
    for a in (1, 7, 15):
        assert model2(data, a=a)[0] == stream


# ---- size -----------------------------------------------------------------------------------------------
# (n, junctions): level 1's bytes, level 2's bytes, as the model gives them
PLANTED = {(32768, 20): (14935, 12066), (65280, 40): (30622, 26320)}


@pytest.mark.parametrize("n,k", sorted(PLANTED))
def test_level_2_is_a_tenth_smaller_on_reads_of_shared_junctions(n, k):
    data = planted_fastq(n, k)
    assert len(data) == n
    one, two = len(model(data)[0]), len(model2(data)[0])
    print("n = %d, %d junctions: level 1 %d bytes, level 2 %d (%.3f), zlib level 6 %d" % (
        n, k, one, two, two / one, len(zlib.compress(data, 6)) - 6))
    assert two <= 0.90 * one, (one, two)
    assert (one, two) == PLANTED[(n, k)]
