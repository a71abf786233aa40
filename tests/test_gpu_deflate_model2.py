"""Level 2 of the GPU DEFLATE compressor (deflate_kernel<2> through fc2_deflate_launch_level) against
its host model (deflate_model2.py, itself checked in test_deflate_model2.py): the same out_len, bytes
and CRC on the contents x lengths grid, on the inputs named for the level-2 search's branches, on level
1's named inputs (the emission path is shared), at tile 0xff00, in a launch of several small tiles (the
links are placed by the tile size), at destination and source alignments; level 1 through the new entry
is fc2_deflate_launch byte for byte; and fc2_gpu_gzip_level / fc2_gpu_bgzf_level at level 2 write members
and blocks whose payloads are the model's."""
import ctypes
import gzip

import numpy as np
import pytest

from bgzf_helpers import check_blocks
from deflate2_inputs import NAMED2, named2, planted_fastq
from deflate_helpers import CONTENTS, check_streams, deflate_launch, explain, pattern, tile_bound
from deflate_model import crc32
from deflate_model2 import model2
from find_circ2_amd import _native as N
from test_deflate_model import GRID_LENGTHS, NAMED, named

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def deflate_launch_level(data: bytes, tile: int, level: int, stride=None, dst_offset=0, src_offset=0):
    """deflate_helpers.deflate_launch through fc2_deflate_launch_level."""
    stride = tile_bound(tile) if stride is None else stride
    n = len(data)
    tiles = (n + tile - 1) // tile
    dev = torch.device("cuda:0")
    before = bytes(0xA5 ^ i for i in range(src_offset))
    src = torch.tensor(np.frombuffer(before + data, np.uint8).copy(), device=dev)
    skipped = np.full(dst_offset, 0x5A, np.uint8)
    dst = torch.tensor(np.concatenate([skipped, pattern((tiles + 2) * stride)]), device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ln = torch.full((tiles,), -7, dtype=torch.int32, device=dev)
    cr = torch.full((tiles,), -7, dtype=torch.int32, device=dev)
    scratch = torch.zeros(max(4, int(N.lib().fc2_deflate_scratch_bytes(n, tile))), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().fc2_deflate_launch_level(src.data_ptr() + src_offset, n, tile, dst.data_ptr() + dst_offset + stride,
                                             stride, ln.data_ptr(), cr.data_ptr(), scratch.data_ptr(),
                                             ctypes.c_void_p(stream), level))
    torch.cuda.synchronize(dev)
    d = dst.cpu().numpy()
    assert (d[:dst_offset] == skipped).all(), "bytes before the output buffer were written"
    return d[dst_offset:], ln.cpu().numpy().view(np.uint32)[:tiles], cr.cpu().numpy().view(np.uint32)[:tiles], stride


def _launch2(data, tile, **kw):
    d, ln, cr, stride = deflate_launch_level(data, tile, 2, **kw)
    return check_streams(data, tile, d, ln, cr, stride), cr


def _equal(streams, cr, tiles, wants):
    for i, (s, t, w) in enumerate(zip(streams, tiles, wants)):
        assert len(s) == len(w) and s == w, "tile %d (%d bytes): %s" % (i, len(t), explain(s, w))
        assert int(cr[i]) == crc32(t), i


@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_kernel_equals_model2_on_the_grid(content):
    for n in GRID_LENGTHS:
        data = CONTENTS[content](n)
        streams, cr = _launch2(data, 65536 if n > 32768 else 32768)
        _equal(streams, cr, [data], [model2(data)[0]])


@pytest.mark.parametrize("name", sorted(NAMED2))
def test_kernel_equals_model2_on_the_level_2_inputs(name):
    data, want, info = named2(name)
    streams, cr = _launch2(data, 65536)
    _equal(streams, cr, [data], [want])


@pytest.mark.parametrize("name", sorted(NAMED))
def test_kernel_equals_model2_on_level_1s_named_inputs(name):
    data = named(name)[0]
    streams, cr = _launch2(data, 65536)
    _equal(streams, cr, [data], [model2(data)[0]])


def test_tile_0xff00_with_reads_of_shared_junctions():
    data = planted_fastq(0xff00 + 5000, 40)
    tiles = [data[:0xff00], data[0xff00:]]
    streams, cr = _launch2(data, 0xff00)
    _equal(streams, cr, tiles, [model2(t)[0] for t in tiles])


def test_five_small_tiles_and_a_short_one():
    data = planted_fastq(5 * 997 + 300, 3)
    tiles = [data[k:k + 997] for k in range(0, len(data), 997)]
    assert len(tiles) == 6 and len(tiles[-1]) == 300
    streams, cr = _launch2(data, 997)
    _equal(streams, cr, tiles, [model2(t)[0] for t in tiles])


def test_destination_alignments_with_a_flushing_stream():
    data, want, info = named2("wrapped_links")
    tile = 65536
    for a in (0, 1, 7, 15):
        assert model2(data, a=a)[1]["flushes"] >= 3
        d, ln, cr, stride = deflate_launch_level(data, tile, 2, dst_offset=a)     # (the bound is a multiple of 16)
        assert (stride + a) % 16 == a
        _equal(check_streams(data, tile, d, ln, cr, stride), cr, [data], [want])


def test_source_offsets():
    data, want, info = named2("wrapped_links")
    for off in (1, 15):
        streams, cr = _launch2(data, 65536, src_offset=off)
        _equal(streams, cr, [data], [want])


def test_level_1_through_the_new_entry_is_fc2_deflate_launch():
    data = planted_fastq(3 * 32768 + 100, 20)
    d0, ln0, cr0, stride = deflate_launch(data, 32768)
    d1, ln1, cr1, _ = deflate_launch_level(data, 32768, 1)
    assert (ln0 == ln1).all() and (cr0 == cr1).all() and (d0 == d1).all()
    d2, ln2, _, _ = deflate_launch_level(data, 32768, 2)
    assert int(ln2.sum()) < 0.9 * int(ln0.sum())


# ---- the two host paths at level 2 ----------------------------------------------------------------------
def _through(entry, bound, data, *args):
    L = N.lib()
    cap = int(bound)
    out = (ctypes.c_uint8 * (cap + 1))()
    out[cap] = 0xC3
    n = ctypes.c_uint64(0)
    src = ctypes.create_string_buffer(data, len(data))
    N.check(getattr(L, entry)(0, src, len(data), *args, out, cap, ctypes.byref(n)))
    assert out[cap] == 0xC3, "a byte past the buffer was written"
    return bytes(bytearray(out)[:int(n.value)])


def test_gpu_gzip_level_2_members_are_the_models():
    tile = 32768
    data = planted_fastq(3 * tile + 1234, 20)
    bound = N.lib().fc2_gpu_gzip_bound(len(data), tile)
    blob = _through("fc2_gpu_gzip_level", bound, data, tile, 2)
    assert gzip.decompress(blob) == data
    pos = 0
    for k in range(0, len(data), tile):
        want = model2(data[k:k + tile])[0]
        assert blob[pos + 10:pos + 10 + len(want)] == want, k
        pos += 10 + len(want) + 8
    assert pos == len(blob)
    one = _through("fc2_gpu_gzip_level", bound, data, tile, 1)
    assert one == _through("fc2_gpu_gzip", bound, data, tile) and len(blob) < 0.9 * len(one)


def test_gpu_bgzf_level_2_blocks_are_the_models():
    block = 0xff00
    data = planted_fastq(2 * block + 4321, 40)
    bound = N.lib().fc2_gpu_bgzf_bound(len(data), block)
    blob = _through("fc2_gpu_bgzf_level", bound, data, block, 2, 2)           # pieces of two blocks
    blocks = check_blocks(blob, data, block)
    for i, b in enumerate(blocks):
        assert b[1] == model2(data[i * block:(i + 1) * block])[0], i
    one = _through("fc2_gpu_bgzf_level", bound, data, block, 2, 1)
    assert one == _through("fc2_gpu_bgzf", bound, data, block, 2) and len(blob) < 0.9 * len(one)
