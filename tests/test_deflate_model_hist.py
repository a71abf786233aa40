"""The host model of the GPU compressor with a history in front of every tile (deflate_model_hist.py) on its
own: without a history it is deflate_model / deflate_model2 byte for byte; the tiles' streams of a launch, back
to back, are one raw DEFLATE stream that zlib inflates to the text; every stream but the last ends on a byte
boundary with BFINAL = 0; every branch of the rule is reached by a named launch that gives other bytes without
it; and -- kernel and model being equal (test_gpu_deflate_hist.py) -- what the history buys in size is decided
here: at level 2, tiles of 32 KiB and of 8 KiB with 32 KiB of history are smaller in total than tiles of 32 KiB
alone on all three texts."""
import zlib

import pytest

from deflate2_inputs import planted_fastq
from deflate_helpers import CONTENTS, deflate_blocks, fastq_text
from deflate_hist_inputs import NAMED_HIST, named_hist
from deflate_model import model
from deflate_model2 import model2
from deflate_model_hist import launch_streams, model_hist
from test_deflate_model import GRID_LENGTHS


def _whole(streams):
    return b"".join(s for s, _, _ in streams)


def _inflates_as_one(streams, text):
    z = zlib.decompressobj(-15)
    got = z.decompress(_whole(streams))
    assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b""
    assert got == text


def _ends_open_on_a_byte(stream):
    """A stream that is not the launch's last: BFINAL = 0 in every block, and it ends with its last block -- a
    stored one (an empty one behind a Huffman block) -- so on a byte boundary.  Checked by reading it with a
    final empty block put behind it."""
    tokens, size, blocks = deflate_blocks(stream + b"\x01\x00\x00\xff\xff")
    assert blocks[-1] == ("stored",) and tokens[-1] == ("stored", 0)
    finals, pos = [], 0
    bits = int.from_bytes(stream[:1], "little")
    assert bits & 1 == 0                            # the first block's BFINAL
    if blocks[0][0] == "dynamic":                   # ... then 000, padding and 00 00 FF FF, and nothing else
        assert [b[0] for b in blocks] == ["dynamic", "stored", "stored"] and stream.endswith(b"\x00\x00\xff\xff")
        assert tokens[-2] == ("stored", 0)
    else:
        assert all(b == ("stored",) for b in blocks)
    return blocks


@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_without_a_history_it_is_the_other_two_models(content):
    for n in GRID_LENGTHS:
        data = CONTENTS[content](n)
        assert model_hist(b"", data, 1, True)[0] == model(data)[0], n
        assert model_hist(b"", data, 2, True)[0] == model2(data)[0], n
        if n <= 4096:                               # hist = 0 in a launch: every tile a stream of its own
            tile = max(1, n // 3)
            for level, m in ((1, model), (2, model2)):
                assert [s for s, _, _ in launch_streams(data, tile, 0, level)] == \
                    [m(data[k:k + tile])[0] for k in range(0, n, tile)]


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("tile,hist", [(64, 3), (100, 65), (997, 4096), (4096, 64), (8192, 32768), (32768, 32768)])
def test_a_launchs_streams_are_one_stream(tile, hist, level):
    for text in (planted_fastq(3 * tile + 17, 20), CONTENTS["random"](2 * tile + 1), CONTENTS["zeros"](2 * tile + 5))[:3 if tile < 8192 else 1]:
        streams = launch_streams(text, tile, hist, level)
        assert len(streams) == -(-len(text) // tile)
        _inflates_as_one(streams, text)
        for i, (s, crc, info) in enumerate(streams):
            data = text[i * tile:(i + 1) * tile]
            assert crc == zlib.crc32(data) and 0 < len(s) <= tile + 16
            if i + 1 < len(streams):
                _ends_open_on_a_byte(s)
            assert info["stored_bytes"] == len(data) + (10 if len(data) > 65535 else 5)
            assert (len(s) == info["stored_bytes"]) == (info["kind"] == "stored") and len(s) <= info["stored_bytes"]


@pytest.mark.parametrize("name", sorted(NAMED_HIST))
def test_named_launch_inflates_and_differs_without_its_branch(name):
    text, tile, hist, level, streams = named_hist(name)
    _inflates_as_one(streams, text)
    for s, _, _ in streams[:-1]:
        _ends_open_on_a_byte(s)
    branch, at = NAMED_HIST[name][1], NAMED_HIST[name][2]
    other = launch_streams(text, tile, hist, level, without=(branch,))
    assert other[at][0] != streams[at][0]
    # ... and the same bytes where nothing reaches the branch: one tile of a text with nothing to refer to
    plain = CONTENTS["acgt"](64)
    if branch not in ("nonfinal", "final"):
        assert launch_streams(plain, 64, 32, level, without=(branch,))[0][0] == (model2 if level == 2 else model)(plain)[0]


def _stats(name):
    text, tile, hist, level, streams = named_hist(name)
    return text, tile, streams, streams[NAMED_HIST[name][2]][2]


def _matches(info, h):
    """{position in the region: (length, distance)} of a tile's tokens behind h bytes of history."""
    out, pos = {}, h
    for t in info["tokens"]:
        if isinstance(t, tuple):
            out[pos] = (t[1], t[2])
            pos += t[1]
        else:
            pos += 1
    return out


def test_path_source_runs_from_the_history_into_the_tile():
    text, tile, streams, info = _stats("src_into_tile")
    assert info["hist"]["into_tile"] == 1 and info["kind"] == "dynamic"
    assert _matches(info, 64)[64] == (48, 16)       # the tile's first position: 16 back, through the boundary


def test_path_distance_32768_taken_and_32769_not():
    text, tile, streams, info = _stats("dist_32768")
    assert info["hist"]["d32768"] == 1 and _matches(info, 32768)[32768] == (258, 32768)
    text, tile, streams, info = _stats("dist_32769")
    assert info["hist"]["d32768"] == 0 and info["hist"]["too_far"] >= 1
    assert all(d <= 32768 for _, d in _matches(info, 32768).values()) and 32769 not in _matches(info, 32768)


def test_path_first_tiles_have_shorter_histories():
    text, tile, streams, info = _stats("short_first_histories")
    assert tile * (len(streams) - 1) < 4096         # every tile's history is what lies before it, below hist
    assert [s[2]["hist"]["entered_hist"] for s in streams] == [0, 100, 200, 300]
    assert all(s[2]["hist"]["hist_src"] >= 1 for s in streams[1:])


def test_path_a_step_straddles_the_boundary():
    text, tile, streams, info = _stats("straddle")
    assert info["hist"]["entered_hist"] == 65       # h = 65: position 64, the history's last, opens the tile's first step
    m = _matches(info, 65)
    assert m[128] == (20, 4) and 129 not in m


def test_path_histories_of_1_and_3_bytes():
    for name, h in (("hist_1", 1), ("hist_3", 3)):
        text, tile, streams, info = _stats(name)
        assert info["hist"]["entered_hist"] == h and info["hist"]["hist_src"] == 1 and info["kind"] == "dynamic"
        assert _matches(info, h)[92 - h] == (12, 92 - h)    # the key's second occurrence: back to position 0, the history's first


def test_path_literal_cost_is_the_tiles_own():
    text, tile, streams, info = _stats("literal_cost")
    assert b"A" not in text[3 * tile:] and set(text[:3 * tile]) == {65}
    other = launch_streams(text, tile, 12288, 1, without=("litcost",))[3][2]
    # a literal of the tile costs 2 bits; with the history's bytes counted 1.75, and the tile's few matches go
    assert sorted(l for l, d in _matches(info, 12288).values()) == [7, 8, 9] and not _matches(other, 12288)


def test_path_tiles_of_one_byte():
    text, tile, streams, info = _stats("tile_of_1")
    assert len(streams) == 20
    assert [s for s, _, _ in streams[:-1]] == [b"\x00\x01\x00\xfe\xff" + text[i:i + 1] for i in range(19)]
    assert streams[-1][0] == b"\x01\x01\x00\xfe\xff" + text[19:]


def test_path_stored_tiles_in_the_middle_and_at_the_end():
    text, tile, streams, info = _stats("stored_middle")
    assert [s[2]["kind"] for s in streams] == ["dynamic", "stored", "dynamic", "stored"]
    assert streams[1][0] == b"\x00\x00\x01\xff\xfe" + text[256:512]
    assert streams[3][0] == b"\x01\x64\x00\x9b\xff" + text[768:]


def test_path_huffman_form_refused_for_its_alignment_bytes():
    text, tile, streams, info = _stats("alignment_bytes")
    alone = launch_streams(text, tile, 64, 1, without=("align",))[0][2]
    assert info["kind"] == "stored" and alone["kind"] == "dynamic"
    assert alone["est"] < info["stored_bytes"] <= info["est"] <= alone["est"] + 5


def test_path_level_2_chain_walks_into_the_history():
    text, tile, streams, info = _stats("chain_into_history")
    assert info["hist"]["chain_into_hist"] >= 1 and info["l2"]["farther"] >= 1
    m = _matches(info, 512)
    at = 512 + 80 + 6 + 100                         # the 40 bytes' second occurrence in the tile
    assert m[at] == (40, at - 100) and m[512 + 80][0] == 6


def test_path_level_2_link_slots_reused_at_65536():
    text, tile, streams, info = _stats("links_reused")
    assert tile + 32768 == 65536 and info["l2"]["window"] >= 1
    assert 32768 not in _matches(info, 32768)       # position 0's slot is position 32768's own: not looked at
    assert _matches(launch_streams(text, tile, 32768, 2, without=("window",))[1][2], 32768)[32768] == (258, 32768)


# ---- size -----------------------------------------------------------------------------------------------
SIZE_N = 4 * 32768
TEXTS = {"planted20": lambda: planted_fastq(SIZE_N, 20), "planted40": lambda: planted_fastq(SIZE_N, 40),
         "fastq": lambda: fastq_text(SIZE_N)}


@pytest.mark.parametrize("text_name", sorted(TEXTS))
def test_level_2_with_history_is_smaller_than_tiles_of_32k_alone(text_name):
    text = TEXTS[text_name]()
    assert len(text) == SIZE_N
    size = {}
    for level in (1, 2):
        for tile, hist in ((32768, 0), (32768, 32768), (8192, 32768)):
            size[(level, tile, hist)] = sum(len(s) for s, _, _ in launch_streams(text, tile, hist, level))
    for level in (1, 2):
        base = size[(level, 32768, 0)]
        print("%s level %d: (32768, 0) %d bytes, (32768, 32768) %.4f, (8192, 32768) %.4f" % (
            text_name, level, base, size[(level, 32768, 32768)] / base, size[(level, 8192, 32768)] / base))
    assert size[(2, 32768, 32768)] < size[(2, 32768, 0)]
    assert size[(2, 8192, 32768)] < size[(2, 32768, 0)]
