"""Level 2's search effort on the GPU (deflate_kernel<2, .., .., true> through fc2_deflate_launch_deep) against its
host model (deflate_model_deep.py, itself checked in test_deflate_model_deep.py): the same out_len, bytes and CRC
at depth and nice (8, 32), (9, 32), (32, 258) and (128, 258) in all three launch shapes -- independent tiles of
32768, tiles of 8192 with 32768 of history, groups of 0xff00 in tiles of 16320 with 32768 of history, tiles of 64
and 65 with 64 of history -- on the inputs the existing models are tested on, on the inputs planted for `depth` and
`nice` (deflate_deep_inputs.py) and on lengths 1, 4, 63, 64, 65 and 32768 + 65; into an unaligned destination,
with the pattern around every slot intact.  At (8, 32) the slots are those of fc2_deflate_launch_level, _hist and
_groups at level 2 from the same library.  fc2_gpu_gzip_deep and fc2_gpu_bgzf_deep give valid files that hold
the input, smaller at (32, 258) than level 2's.

Every case is a few tiles; the model's answers are computed once a setting and shared."""
import ctypes
import gzip
import zlib
from functools import lru_cache

import numpy as np
import pytest

from bgzf_helpers import check_blocks, parse_blocks
from deflate2_inputs import NAMED2, named2, planted_fastq
from deflate_deep_inputs import bam_records, named_deep
from deflate_helpers import explain, pattern, tile_bound
from deflate_hist_inputs import NAMED_HIST, named_hist
from deflate_model_deep import launch_deep
from deflate_model_groups import boundary_input, group_tiles
from find_circ2_amd import _native as N
from test_gpu_deflate_groups import launch_groups
from test_gpu_deflate_hist import launch_hist
from test_gpu_deflate_model2 import _through, deflate_launch_level

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SETTINGS = ((8, 32), (9, 32), (32, 258), (128, 258))


def gpu_launch_deep(data: bytes, group: int, tile: int, hist: int, depth: int, nice: int, dst_offset=3, extra_stride=5,
                    src_offset=0):
    """fc2_deflate_launch_deep over data: (the tiles' streams, their CRCs), tiles numbered as the launch numbers them.
    The destination is unaligned (dst_offset, and a stride that is no multiple of 16); the output buffer is
    pre-filled with pattern() and has a guard slot before the first tile's slot and one after the last; nothing but
    [slot, slot + out_len) of every tile may differ from it afterwards, nor the entry past the launch's tiles in
    out_len and crc, nor the bytes past the scratch."""
    stride = tile_bound(tile) + extra_stride
    n = len(data)
    tiles = group_tiles(n, group, tile) if group else (n + tile - 1) // tile
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
    N.check(N.lib().fc2_deflate_launch_deep(src.data_ptr() + src_offset, n, group, tile, hist,
                                            dst.data_ptr() + dst_offset + stride, stride, ln.data_ptr(), cr.data_ptr(),
                                            scratch.data_ptr(), ctypes.c_void_p(stream), depth, nice))
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
def _text(n, k=20):
    return planted_fastq(n, k)


@lru_cache(maxsize=None)
def _want(key, group, tile, hist, depth, nice):
    return launch_deep(_input(key), group, tile, hist, depth, nice)


@lru_cache(maxsize=None)
def _input(key):
    kind, arg = key
    if kind == "named2":
        return named2(arg)[0]
    if kind == "hist":
        return named_hist(arg)[0]
    if kind == "deep":
        return named_deep(arg)[0]
    if kind == "boundary":
        return boundary_input(arg)[:arg + 300 + 9]      # (the second group: the copy of the first one's end, and 9 bytes)
    if kind == "bam":
        return bam_records(arg)
    return _text(arg)


def _check(key, group, tile, hist, depth, nice):
    data = _input(key)
    want = _want(key, group, tile, hist, depth, nice)
    streams, crcs = gpu_launch_deep(data, group, tile, hist, depth, nice)
    assert len(streams) == len(want), (key, group, tile, hist)
    for i, (s, (w, crc, info)) in enumerate(zip(streams, want)):
        assert len(s) == len(w) and s == w, "%r group %d tile %d hist %d at (%d, %d), tile %d of %d: %d bytes against the model's %d; %s" % (
            key, group, tile, hist, depth, nice, i, len(want), len(s), len(w),
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


LENGTHS = (1, 4, 63, 64, 65, 32768 + 65)
# the long inputs of the existing models' tests, whose model takes seconds at depth 128: at (32, 258) only
LONG = {("named2", "window_edge"), ("hist", "dist_32768"), ("hist", "dist_32769"), ("hist", "links_reused")}


@pytest.mark.parametrize("depth,nice", SETTINGS)
def test_independent_tiles_of_32768(depth, nice):
    keys = [("named2", n) for n in sorted(NAMED2)] + [("deep", n) for n in ("bucket33_9", "bucket33_33", "nice40_120")] + \
        [("text", n) for n in LENGTHS]
    for key in keys:
        if key in LONG and (depth, nice) != (32, 258):
            continue
        _check(key, 0, 32768, 0, depth, nice)


@pytest.mark.parametrize("depth,nice", SETTINGS)
def test_tiles_of_8192_with_32768_of_history(depth, nice):
    for key in [("text", n) for n in LENGTHS] + [("deep", n) for n in ("bucket33_33", "nice40_120")] + [("bam", 3 * 8192 + 17)]:
        _check(key, 0, 8192, 32768, depth, nice)


@pytest.mark.parametrize("depth,nice", SETTINGS)
def test_the_history_models_named_launches(depth, nice):
    for name in sorted(NAMED_HIST):
        if ("hist", name) in LONG and (depth, nice) != (32, 258):
            continue
        _text_, tile, hist, _level, _ = named_hist(name)
        _check(("hist", name), 0, tile, hist, depth, nice)


@pytest.mark.parametrize("depth,nice", SETTINGS)
def test_groups_of_0xff00_in_tiles_of_16320_with_32768_of_history(depth, nice):
    for key in [("text", n) for n in LENGTHS] + [("bam", 0xff00 + 16320 + 9), ("boundary", 0xff00), ("deep", "bucket33_9")]:
        _check(key, 0xff00, 16320, 32768, depth, nice)


@pytest.mark.parametrize("depth,nice", SETTINGS)
@pytest.mark.parametrize("tile", (64, 65))
def test_tiles_of_64_and_65_with_64_of_history(tile, depth, nice):
    for key in [("text", n) for n in (1, 4, 63, 64, 65, 3 * tile + 17)] + [("deep", "nice40_120")]:
        _check(key, 0, tile, 64, depth, nice)
    _check(("text", 3 * tile + 17), 200, tile, 64, depth, nice)       # (groups of three tiles and a bit)


def test_the_deep_walk_ends_at_the_stale_slot_in_a_region_of_65536():
    text, tile, hist, _p = named_deep("stale_chain")
    _check(("deep", "stale_chain"), 0, tile, hist, 32, 258)
    assert _want(("deep", "stale_chain"), 0, tile, hist, 32, 258)[1][2]["l2"]["window"] > 0


def test_an_unaligned_source_and_every_destination_alignment():
    key, group, tile, hist, depth, nice = ("text", 0xff00 + 16320 + 9), 0xff00, 16320, 32768, 32, 258
    data, want = _input(key), _want(key, 0xff00, 16320, 32768, 32, 258)
    for a in range(16):
        streams, crcs = gpu_launch_deep(data, group, tile, hist, depth, nice, dst_offset=a, extra_stride=a % 3)
        assert streams == [s for s, _, _ in want] and crcs == [c for _, c, _ in want], a
    for off in (1, 7, 15):
        streams, crcs = gpu_launch_deep(data, group, tile, hist, depth, nice, src_offset=off)
        assert streams == [s for s, _, _ in want] and crcs == [c for _, c, _ in want], off


def test_at_8_32_the_slots_are_the_existing_entries_at_level_2():
    text = _text(0xff00 + 16320 + 9)
    d, ln, cr, stride = deflate_launch_level(text, 32768, 2)
    level = [d[(i + 1) * stride:(i + 1) * stride + int(ln[i])].tobytes() for i in range(len(ln))], [int(c) for c in cr]
    assert gpu_launch_deep(text, 0, 32768, 0, 8, 32) == level
    assert gpu_launch_deep(text, 0, 8192, 32768, 8, 32) == launch_hist(text, 8192, 32768, 2)
    assert gpu_launch_deep(text, 0xff00, 16320, 32768, 8, 32) == launch_groups(text, 0xff00, 16320, 32768, 2)
    assert gpu_launch_deep(text, 0xff00, 16320, 0, 8, 32) == launch_groups(text, 0xff00, 16320, 0, 2)
    assert gpu_launch_deep(text, 0, 64, 64, 8, 32) == launch_hist(text, 64, 64, 2)
    # ... and another setting is another search
    assert gpu_launch_deep(text, 0, 32768, 0, 32, 258) != level


# ---- the two host paths ------------------------------------------------------------------------------------

def test_gpu_gzip_deep_files_hold_the_input():
    tile, hist = 32768, 32768
    data = planted_fastq(3 * tile + 1234, 40)
    bound = N.lib().fc2_gpu_gzip_bound(len(data), tile)
    level2 = _through("fc2_gpu_gzip_hist", bound, data, tile, hist, 2)
    assert _through("fc2_gpu_gzip_deep", bound, data, tile, hist, 8, 32) == level2
    deep = _through("fc2_gpu_gzip_deep", bound, data, tile, hist, 32, 258)
    assert gzip.decompress(deep) == data and len(deep) < len(level2)
    assert deep[10:-8] == b"".join(s for s, _, _ in launch_deep(data, 0, tile, hist, 32, 258))     # one member a piece
    # a member per tile without a history
    each = _through("fc2_gpu_gzip_deep", bound, data, tile, 0, 32, 258)
    assert gzip.decompress(each) == data and len(each) < len(_through("fc2_gpu_gzip_level", bound, data, tile, 2))
    assert each.count(bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])) >= 4
    n = ctypes.c_uint64(7)
    out = (ctypes.c_uint8 * 64)()
    N.check(N.lib().fc2_gpu_gzip_deep(0, None, 0, tile, hist, 32, 258, out, 64, ctypes.byref(n)))
    assert gzip.decompress(bytes(bytearray(out)[:n.value])) == b""


@pytest.mark.parametrize("tile,hist", [(0, 0), (16320, 32768)])
def test_gpu_bgzf_deep_blocks_hold_the_input(tile, hist):
    block = 0xff00
    data = planted_fastq(2 * block + 4321, 40)
    bound = N.lib().fc2_gpu_bgzf_tiles_bound(len(data), block, tile)
    level2 = _through("fc2_gpu_bgzf_tiles", bound, data, block, 2, tile, hist, 2)           # pieces of two blocks
    assert _through("fc2_gpu_bgzf_deep", bound, data, block, 2, tile, hist, 8, 32) == level2
    deep = _through("fc2_gpu_bgzf_deep", bound, data, block, 2, tile, hist, 32, 258)
    blocks = check_blocks(deep, data, block)        # valid blocks, ISIZE, CRC-32, gzip.decompress
    untiled = _through("fc2_gpu_bgzf_level", N.lib().fc2_gpu_bgzf_bound(len(data), block), data, block, 2, 2)
    assert [b[3] for b in blocks] == [b[3] for b in parse_blocks(untiled)] == [block, block, 4321]
    assert len(deep) < len(level2)
    want = launch_deep(data, block if tile else 0, tile or block, hist, 32, 258)
    assert b"".join(b[1] for b in blocks) == b"".join(s for s, _, _ in want)
