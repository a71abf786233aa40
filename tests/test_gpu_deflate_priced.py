"""Level 2's priced passes on the GPU (deflate_kernel<2, .., .., true, true> through fc2_deflate_launch_priced) against
their host model (deflate_model_priced.py, itself checked in test_deflate_model_priced.py): the same out_len, bytes and
CRC with 2 and 3 passes at depth and nice (8, 32) and (32, 258) -- independent tiles of 1, 3, 4, 5, 63, 64, 65 and 4097
bytes and one of 0xff00 bytes of BAM records; the four inputs planted for the branches of the priced rule
(deflate_priced_inputs.py); tiles of 4096 with 4096 of history; the chain that runs over a region of 65536 bytes,
where link slots are reused in a pass that runs again; and groups of 0xff00 in tiles of 16320 with 32768 of history,
the BAM writer's setting (nine tiles at (8, 32), five at (32, 258)) -- into an unaligned destination, with the pattern
around every slot intact.  With one pass the slots are fc2_deflate_launch_deep's.  fc2_gpu_gzip_priced and
fc2_gpu_bgzf_priced give valid files that hold the input, and with one pass the _deep entries' bytes.

The model's answers are computed once a case and shared."""
import ctypes
import gzip
import zlib
from functools import lru_cache

import numpy as np
import pytest

from bgzf_helpers import check_blocks
from deflate2_inputs import planted_fastq
from deflate_deep_inputs import bam_records, named_deep
from deflate_helpers import explain, pattern, tile_bound
from deflate_model_groups import group_tiles
from deflate_model_priced import launch_priced
from deflate_priced_inputs import BRANCH, PLANTED, planted
from find_circ2_amd import _native as N
from test_gpu_deflate_deep import gpu_launch_deep
from test_gpu_deflate_model2 import _through

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SETTINGS = ((8, 32), (32, 258))
PASSES = (2, 3)


def gpu_launch_priced(data: bytes, group: int, tile: int, hist: int, depth: int, nice: int, passes: int, dst_offset=3,
                      extra_stride=5):
    """fc2_deflate_launch_priced over data: (the tiles' streams, their CRCs), as test_gpu_deflate_deep.gpu_launch_deep
    takes them: an unaligned destination pre-filled with pattern(), a guard slot before the first tile's slot and one
    after the last; nothing but [slot, slot + out_len) of every tile may differ from it afterwards, nor the entry past
    the launch's tiles in out_len and crc, nor the bytes past the scratch."""
    stride = tile_bound(tile) + extra_stride
    n = len(data)
    tiles = group_tiles(n, group, tile) if group else (n + tile - 1) // tile
    dev = torch.device("cuda:0")
    src = torch.tensor(np.frombuffer(data, np.uint8).copy(), device=dev)
    skipped = np.full(dst_offset, 0x5A, np.uint8)
    dst = torch.tensor(np.concatenate([skipped, pattern((tiles + 2) * stride)]), device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ln = torch.full((tiles + 1,), -7, dtype=torch.int32, device=dev)
    cr = torch.full((tiles + 1,), -7, dtype=torch.int32, device=dev)
    scratch = torch.zeros(max(4, int(N.lib().fc2_deflate_scratch_bytes(n, tile))) + 64, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().fc2_deflate_launch_priced(src.data_ptr(), n, group, tile, hist, dst.data_ptr() + dst_offset + stride,
                                              stride, ln.data_ptr(), cr.data_ptr(), scratch.data_ptr(),
                                              ctypes.c_void_p(stream), depth, nice, passes))
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


@lru_cache(maxsize=None)
def _input(key):
    kind, arg = key
    if kind == "bam":
        return bam_records(arg)
    if kind == "planted":
        return b"".join(planted(arg))
    if kind == "deep":
        return named_deep(arg)[0]
    return planted_fastq(arg, 20)


@lru_cache(maxsize=None)
def _want(key, group, tile, hist, depth, nice, passes):
    return launch_priced(_input(key), group, tile, hist, depth, nice, passes)


def _check(key, group, tile, hist, depth, nice, passes):
    data = _input(key)
    want = _want(key, group, tile, hist, depth, nice, passes)
    streams, crcs = gpu_launch_priced(data, group, tile, hist, depth, nice, passes)
    assert len(streams) == len(want), (key, group, tile, hist)
    for i, (s, (w, crc, info)) in enumerate(zip(streams, want)):
        assert len(s) == len(w) and s == w, "%r group %d tile %d hist %d at (%d, %d), %d passes, tile %d of %d: %d bytes against the model's %d; %s" % (
            key, group, tile, hist, depth, nice, passes, i, len(want), len(s), len(w),
            explain(s, w) if info.get("kind") == "dynamic" and len(s) == len(w) and i + 1 == len(want) else "")
        assert crcs[i] == crc, (key, i)
    # the streams of a stream's tiles, back to back, inflate to its bytes
    if group:
        parts = [data[g:g + group] for g in range(0, len(data), group)]
        per = [group_tiles(len(p), group, tile) for p in parts]
    elif hist:
        parts, per = [data], [len(streams)]
    else:
        parts, per = [data[k:k + tile] for k in range(0, len(data), tile)], [1] * len(streams)
    i = 0
    for part, cnt in zip(parts, per):
        z = zlib.decompressobj(-15)
        assert z.decompress(b"".join(streams[i:i + cnt])) == part and z.eof and z.unused_data == b"", (key, i)
        i += cnt
    return want


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("depth,nice", SETTINGS)
def test_independent_tiles_of_small_lengths(depth, nice, passes):
    for n in (1, 3, 4, 5, 63, 64, 65, 4097):
        _check(("text", n), 0, 65536, 0, depth, nice, passes)
    _check(("text", 4097 + 65), 0, 4097, 0, depth, nice, passes)       # (two tiles, the second of 65 bytes)


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("depth,nice", SETTINGS)
def test_one_tile_of_0xff00_bytes_of_bam_records(depth, nice, passes):
    want = _check(("bam", 0xff00), 0, 0xff00, 0, depth, nice, passes)
    assert want[0][2]["priced"]["passes"] == passes and want[0][2]["priced"]["gained"] > 0
    assert want[0][0] != _want(("bam", 0xff00), 0, 0xff00, 0, depth, nice, 1)[0][0]


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("name", sorted(PLANTED))
def test_the_planted_inputs(name, passes):
    history, data = planted(name)
    tile = len(data) if not history else len(history)
    assert not history or len(history) == len(data)
    want = _check(("planted", name), 0, tile, len(history), 8, 32, passes)
    assert want[-1][2]["priced"][BRANCH[name][0]] > 0


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("depth,nice", SETTINGS)
def test_tiles_of_4096_with_4096_of_history(depth, nice, passes):
    _check(("text", 3 * 4096 + 17), 0, 4096, 4096, depth, nice, passes)


def test_a_pass_that_runs_again_ends_its_walks_at_the_stale_slot_in_a_region_of_65536():
    text, tile, hist, _p = named_deep("stale_chain")
    want = _check(("deep", "stale_chain"), 0, tile, hist, 32, 258, 2)
    assert want[1][2]["priced"]["passes"] == 2


@pytest.mark.parametrize("passes", PASSES)
def test_groups_of_0xff00_in_tiles_of_16320_with_32768_of_history(passes):
    # (at level 2's own search: the model takes 9 s on these nine tiles at (32, 258); five tiles at it below)
    want = _check(("bam", 2 * 0xff00 + 1000), 0xff00, 16320, 32768, 8, 32, passes)
    assert len(want) == 9


def test_groups_at_32_258_on_five_tiles():
    # (the groups' instantiation at the deeper search, byte for byte, on an input its model takes under 5 s for)
    want = _check(("bam", 0xff00 + 1000), 0xff00, 16320, 32768, 32, 258, 2)
    assert len(want) == 5 and all(w[2]["priced"]["passes"] == 2 for w in want)


def test_with_one_pass_the_slots_are_launch_deeps():
    text = _input(("text", 3 * 4096 + 17))
    for group, tile, hist in ((0, 4096, 0), (0, 4096, 4096), (5000, 2048, 4096)):
        for depth, nice in SETTINGS:
            assert gpu_launch_priced(text, group, tile, hist, depth, nice, 1) == gpu_launch_deep(text, group, tile, hist, depth, nice)
    assert gpu_launch_priced(text, 0, 4096, 4096, 8, 32, 2) != gpu_launch_deep(text, 0, 4096, 4096, 8, 32)


# ---- the two host paths ------------------------------------------------------------------------------------

def test_gpu_gzip_priced_files_hold_the_input():
    tile, hist = 32768, 32768
    data = planted_fastq(2 * tile + 1234, 40)
    bound = N.lib().fc2_gpu_gzip_bound(len(data), tile)
    for depth, nice in SETTINGS:
        assert _through("fc2_gpu_gzip_priced", bound, data, tile, hist, depth, nice, 1) == \
            _through("fc2_gpu_gzip_deep", bound, data, tile, hist, depth, nice)
    one = _through("fc2_gpu_gzip_deep", bound, data, tile, hist, 8, 32)
    two = _through("fc2_gpu_gzip_priced", bound, data, tile, hist, 8, 32, 2)
    assert gzip.decompress(two) == data and two != one
    assert two[10:-8] == b"".join(s for s, _, _ in launch_priced(data, 0, tile, hist, 8, 32, 2))     # one member a piece
    each = _through("fc2_gpu_gzip_priced", bound, data, tile, 0, 8, 32, 3)                       # a member per tile
    assert gzip.decompress(each) == data and each.count(bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])) >= 3
    n = ctypes.c_uint64(7)
    out = (ctypes.c_uint8 * 64)()
    N.check(N.lib().fc2_gpu_gzip_priced(0, None, 0, tile, hist, 32, 258, 2, out, 64, ctypes.byref(n)))
    assert gzip.decompress(bytes(bytearray(out)[:n.value])) == b""


@pytest.mark.parametrize("tile,hist", [(0, 0), (16320, 32768)])
def test_gpu_bgzf_priced_blocks_hold_the_input(tile, hist):
    block = 0xff00
    data = bam_records(block + 4321)
    bound = N.lib().fc2_gpu_bgzf_tiles_bound(len(data), block, tile)
    for depth, nice in SETTINGS:
        assert _through("fc2_gpu_bgzf_priced", bound, data, block, 2, tile, hist, depth, nice, 1) == \
            _through("fc2_gpu_bgzf_deep", bound, data, block, 2, tile, hist, depth, nice)
    one = _through("fc2_gpu_bgzf_deep", bound, data, block, 2, tile, hist, 8, 32)
    two = _through("fc2_gpu_bgzf_priced", bound, data, block, 2, tile, hist, 8, 32, 2)
    blocks = check_blocks(two, data, block)         # valid blocks, ISIZE, CRC-32, gzip.decompress
    assert [b[3] for b in blocks] == [block, 4321] and two != one and len(two) < len(one)
    want = launch_priced(data, block if tile else 0, tile or block, hist, 8, 32, 2)
    assert b"".join(b[1] for b in blocks) == b"".join(s for s, _, _ in want)
