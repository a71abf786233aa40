"""The GPU DEFLATE compressor over groups (deflate_kernel<level, true, true> through fc2_deflate_launch_groups)
against its host model (deflate_model_groups.py, itself checked in test_deflate_model_groups.py): the same
out_len, bytes and CRC at both levels on launches of two whole groups and a short one over the group x tile x
hist grid -- a group that is and is not a multiple of the tile, one tile a group, hist = 0 with several tiles --
and on an input whose second group begins with a copy of the first group's end, which a history that crossed the
boundary would find; at the 16 destination alignments and from an unaligned source, with the pattern around every
slot intact; one tile a group is fc2_deflate_launch_level, a single group fc2_deflate_launch_hist, byte for
byte."""
import ctypes
import zlib
from functools import lru_cache

import numpy as np
import pytest

from deflate2_inputs import planted_fastq
from deflate_helpers import explain, pattern, tile_bound
from deflate_model_groups import boundary_input, group_streams, group_tiles
from find_circ2_amd import _native as N
from test_gpu_deflate_hist import launch_hist
from test_gpu_deflate_model2 import deflate_launch_level

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GROUPS = (100, 4113, 0xff00)
HISTS = (0, 1, 63, 65, 4096, 32768)


def launch_groups(data: bytes, group: int, tile: int, hist: int, level: int, stride=None, dst_offset=0, src_offset=0):
    """fc2_deflate_launch_groups over data: (the tiles' streams, their CRCs), tiles numbered as the launch numbers
    them.  The output buffer is pre-filled with pattern() and has a guard slot before the first tile's slot and
    one after the last; nothing but [slot, slot + out_len) of every tile may differ from it afterwards."""
    stride = tile_bound(tile) if stride is None else stride
    n = len(data)
    tiles = group_tiles(n, group, tile)
    assert tiles == int(N.lib().fc2_deflate_group_tiles(n, group, tile))
    dev = torch.device("cuda:0")
    before = bytes(0xA5 ^ i for i in range(src_offset))
    src = torch.tensor(np.frombuffer(before + data, np.uint8).copy(), device=dev)
    skipped = np.full(dst_offset, 0x5A, np.uint8)
    dst = torch.tensor(np.concatenate([skipped, pattern((tiles + 2) * stride)]), device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ln = torch.full((tiles + 1,), -7, dtype=torch.int32, device=dev)
    cr = torch.full((tiles + 1,), -7, dtype=torch.int32, device=dev)
    scratch = torch.zeros(max(4, int(N.lib().fc2_deflate_scratch_bytes(n, tile))) + 64, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().fc2_deflate_launch_groups(src.data_ptr() + src_offset, n, group, tile, hist,
                                              dst.data_ptr() + dst_offset + stride, stride, ln.data_ptr(), cr.data_ptr(),
                                              scratch.data_ptr(), ctypes.c_void_p(stream), level))
    torch.cuda.synchronize(dev)
    d = dst.cpu().numpy()
    assert (d[:dst_offset] == skipped).all(), "bytes before the output buffer were written"
    d = d[dst_offset:]
    ln, cr = ln.cpu().numpy().view(np.uint32), cr.cpu().numpy().view(np.uint32)
    assert ln[tiles] == cr[tiles] == 0xFFFFFFF9, "an entry past the launch's tiles was written"
    assert not scratch[-64:].any().item(), "bytes past the scratch were written"
    clean = d == pattern(len(d))
    assert clean[:stride].all(), "the guard slot before the tiles was written"
    assert clean[(tiles + 1) * stride:].all(), "the guard slot after the tiles was written"
    streams = []
    for i in range(tiles):
        k = int(ln[i])
        assert 0 < k <= tile_bound(tile), (i, k)
        a = (i + 1) * stride
        bad = np.nonzero(~clean[a + k:a + stride])[0]
        assert len(bad) == 0, "tile %d wrote at byte %d of its slot, past its %d bytes" % (i, k + int(bad[0]), k)
        streams.append(d[a:a + k].tobytes())
    return streams, [int(c) for c in cr[:tiles]]


def _equal(data, group, tile, got, want):
    """got: launch_groups' result; want: group_streams' groups."""
    streams, crcs = got
    flat = [t for tiles in want for t in tiles]
    assert len(streams) == len(flat)
    for i, (s, (w, crc, info)) in enumerate(zip(streams, flat)):
        assert len(s) == len(w) and s == w, "tile %d of %d: %d bytes against the model's %d; %s" % (
            i, len(flat), len(s), len(w), explain(s, w) if info.get("kind") == "dynamic" and len(s) == len(w) else "")
        assert crcs[i] == crc, i
    i = 0
    for g, tiles in enumerate(want):                # each group inflates to its bytes, and ends there
        part = data[g * group:(g + 1) * group]
        z = zlib.decompressobj(-15)
        assert z.decompress(b"".join(streams[i:i + len(tiles)])) == part and z.eof and z.unused_data == b"", g
        assert crcs[i:i + len(tiles)] == [zlib.crc32(part[k:k + tile]) for k in range(0, len(part), tile)]
        i += len(tiles)


@lru_cache(maxsize=None)
def _grid_text(n):
    return planted_fastq(n, 20)


def _grid():
    for group in GROUPS:
        for tile in (64, group // 4, group // 4 + 1, group):
            for hist in HISTS:
                if tile + hist <= 65536:
                    yield group, tile, hist


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("group,tile,hist", list(_grid()))
def test_two_groups_and_17_bytes(group, tile, hist, level):
    text = _grid_text(2 * group + 17)
    _equal(text, group, tile, launch_groups(text, group, tile, hist, level), group_streams(text, group, tile, hist, level))


@pytest.mark.parametrize("level", (1, 2))
def test_no_history_across_a_group_boundary(level):
    group, tile, hist = 4113, 1029, 4096
    text = boundary_input(group)
    want = group_streams(text, group, tile, hist, level)
    assert not any(isinstance(t, tuple) and t[2] == 300 for t in want[1][0][2]["tokens"])   # the model's miss
    got = launch_groups(text, group, tile, hist, level)
    _equal(text, group, tile, got, want)


@pytest.mark.parametrize("level", (1, 2))
def test_destination_alignments_and_an_unaligned_source(level):
    group, tile, hist = 4113, 1029, 65
    text = _grid_text(2 * group + 17)
    want = group_streams(text, group, tile, hist, level)
    for a in range(16):
        _equal(text, group, tile, launch_groups(text, group, tile, hist, level, stride=tile_bound(tile) + 3, dst_offset=a), want)
    for off in (1, 7, 15):
        _equal(text, group, tile, launch_groups(text, group, tile, hist, level, src_offset=off), want)
    _equal(text, group, tile, launch_groups(text, group, tile, hist, level, stride=tile_bound(tile) + 5, dst_offset=3,
                                            src_offset=9), want)


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("hist", (0, 300))
def test_one_tile_a_group_is_fc2_deflate_launch_level(hist, level):
    group = 4113
    text = _grid_text(2 * group + 17)
    d, ln, cr, stride = deflate_launch_level(text, group, level)
    want = [d[(i + 1) * stride:(i + 1) * stride + int(ln[i])].tobytes() for i in range(len(ln))]
    for tile in (group, group + 1, 65536 - hist):
        streams, crcs = launch_groups(text, group, tile, hist, level)
        assert streams == want and crcs == [int(x) for x in cr], tile


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("tile,hist", [(1029, 4096), (64, 65)])
def test_a_single_group_is_fc2_deflate_launch_hist(tile, hist, level):
    text = _grid_text(2 * 4113 + 17)
    for group in (len(text), len(text) + 1, 1 << 31):
        assert launch_groups(text, group, tile, hist, level) == launch_hist(text, tile, hist, level), group
