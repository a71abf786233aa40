"""deflate_model_groups.group_streams, the rule of fc2_deflate_launch_groups in Python: every group's streams
back to back are one raw DEFLATE stream of the group's bytes (hist = 0 with several tiles too); one tile a group
is deflate_model.model / deflate_model2.model2; with a history a group is deflate_model_hist.launch_streams over
the group's bytes alone; a history never reaches across a group's start; BAM-like records in four tiles of
0x3fc0 bytes with 32 KiB of history stay within 1 % of the untiled blocks' size at both levels; and a block of
0xff00 random bytes in 16 tiles is 65280 + 16 * 5 stream bytes."""
import zlib
from functools import lru_cache

import numpy as np
import pytest

import deflate_model
from bgzf_helpers import bam_like
from deflate2_inputs import planted_fastq
from deflate_model2 import model2
from deflate_model_groups import boundary_input, group_streams, group_tiles
from deflate_model_hist import launch_streams


@lru_cache(maxsize=None)
def _text(n):
    return planted_fastq(n, 20)


def _inflates(text, group, tile, groups):
    assert len(groups) == -(-len(text) // group)
    for g, tiles in enumerate(groups):
        part = text[g * group:(g + 1) * group]
        z = zlib.decompressobj(-15)
        assert z.decompress(b"".join(s for s, _, _ in tiles)) == part and z.eof and z.unused_data == b"", g
        z = zlib.decompressobj(-15)                 # only the group's last tile ends the stream
        for k, (s, _, _) in enumerate(tiles):
            z.decompress(s)
            assert z.eof == (k + 1 == len(tiles)), (g, k)
        assert [c for _, c, _ in tiles] == [zlib.crc32(part[k:k + tile]) for k in range(0, len(part), tile)]


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("hist", (0, 1, 65, 4096))
@pytest.mark.parametrize("group,tile", [(100, 64), (100, 25), (100, 26), (100, 100), (4113, 64), (4113, 1028), (4113, 1029),
                                        (4113, 5000)])
def test_groups_inflate_to_their_bytes(group, tile, hist, level):
    text = _text(2 * group + 17)
    groups = group_streams(text, group, tile, hist, level)
    _inflates(text, group, tile, groups)
    assert sum(len(t) for t in groups) == group_tiles(len(text), group, tile)
    assert [len(t) for t in groups] == [-(-group // tile)] * 2 + [-(-17 // tile)]


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("hist", (0, 300))
def test_one_tile_a_group_is_the_untiled_model(hist, level):
    text, group = _text(2 * 4113 + 17), 4113
    model = model2 if level == 2 else deflate_model.model
    for tile in (group, group + 1, 65536 - hist):
        groups = group_streams(text, group, tile, hist, level)
        assert [len(t) for t in groups] == [1, 1, 1]
        for g, tiles in enumerate(groups):
            assert tiles[0][0] == model(text[g * group:(g + 1) * group], 0)[0], (tile, g)


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("tile,hist", [(64, 1), (1028, 63), (1029, 4096), (1500, 32768)])
def test_with_a_history_a_group_is_a_launch_of_its_own(tile, hist, level):
    text, group = _text(2 * 4113 + 17), 4113
    for g, tiles in enumerate(group_streams(text, group, tile, hist, level)):
        want = launch_streams(text[g * group:(g + 1) * group], tile, hist, level)
        assert [(s, c) for s, c, _ in tiles] == [(s, c) for s, c, _ in want], g


@pytest.mark.parametrize("level", (1, 2))
def test_no_history_across_a_group_boundary(level):
    group, tile, hist = 4113, 1029, 4096
    text = boundary_input(group)
    groups = group_streams(text, group, tile, hist, level)
    _inflates(text, group, tile, groups)
    first = groups[1][0][2]["tokens"]               # the second group's first tile: 300 bytes seen nowhere before
    assert not any(isinstance(t, tuple) and t[2] == 300 for t in first)
    assert groups[1][0][2]["hist"]["hist_src"] == 0
    # one launch over the same bytes (no groups) does reach back, and finds the copy at distance 300
    across = launch_streams(text[:2 * group], group, hist, level)[1][2]["tokens"]
    assert any(isinstance(t, tuple) and t[2] == 300 for t in across)
    assert groups[1][0][0] != launch_streams(text[:2 * group], group, hist, level)[1][0]


def test_bam_records_in_four_tiles_stay_within_a_percent():
    """The size condition: tile 0x3fc0 with 32 KiB of history against the untiled block (the model gives 1.0043
    at level 1 and 1.0011 at level 2)."""
    text = bam_like(3 * 0xff00 + 1000)
    for level in (1, 2):
        untiled = sum(len(s) for t in group_streams(text, 0xff00, 0xff00, 0, level) for s, _, _ in t)
        tiled = sum(len(s) for t in group_streams(text, 0xff00, 0x3fc0, 32768, level) for s, _, _ in t)
        ratio = tiled / untiled
        print("level %d: %d / %d = %.4f" % (level, tiled, untiled, ratio))
        assert ratio <= 1.01, (level, ratio)


def test_random_block_in_16_tiles_is_stored():
    data = bytes(np.random.default_rng(3).integers(0, 256, 0xff00, dtype=np.uint8))
    (tiles,) = group_streams(data, 0xff00, 0xff00 // 16, 0, 1)
    assert len(tiles) == 16 and all(info["kind"] == "stored" for _, _, info in tiles)
    assert sum(len(s) for s, _, _ in tiles) == 65280 + 80
    z = zlib.decompressobj(-15)
    assert z.decompress(b"".join(s for s, _, _ in tiles)) == data and z.eof
