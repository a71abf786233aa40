"""The GPU DEFLATE compressor with a history in front of every tile (deflate_kernel<level, true> through
fc2_deflate_launch_hist) against its host model (deflate_model_hist.py, itself checked in
test_deflate_model_hist.py): the same out_len, bytes and CRC at both levels on the inputs named for the
rule's branches, on launches of 3 * tile + 17 bytes over the tile x hist grid, at the 16 destination
alignments and from an unaligned source, with the pattern around every slot intact; hist = 0 is
fc2_deflate_launch_level byte for byte; and fc2_gpu_gzip_hist writes one member per piece whose payload is the
model's streams back to back."""
# (a piece of fc2_gpu_gzip_hist is 4 MiB: its whole pieces are compared with fc2_deflate_launch_hist's own output)
import ctypes
import gzip
import zlib
from functools import lru_cache

import numpy as np
import pytest

from deflate2_inputs import planted_fastq
from deflate_helpers import explain, pattern, tile_bound
from deflate_hist_inputs import NAMED_HIST, named_hist
from deflate_model_hist import launch_streams
from find_circ2_amd import _native as N
from test_gpu_deflate_model2 import _through, deflate_launch_level

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILES = (64, 100, 4096, 8192, 32768)
HISTS = (1, 3, 4, 63, 64, 65, 4096, 32768)


def launch_hist(data: bytes, tile: int, hist: int, level: int, stride=None, dst_offset=0, src_offset=0):
    """fc2_deflate_launch_hist over data: (the tiles' streams, their CRCs).  The output buffer is pre-filled
    with pattern() and has a guard slot before the first tile's slot and one after the last; nothing but
    [slot, slot + out_len) of every tile may differ from it afterwards."""
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
    N.check(N.lib().fc2_deflate_launch_hist(src.data_ptr() + src_offset, n, tile, hist, dst.data_ptr() + dst_offset + stride,
                                            stride, ln.data_ptr(), cr.data_ptr(), scratch.data_ptr(),
                                            ctypes.c_void_p(stream), level))
    torch.cuda.synchronize(dev)
    d = dst.cpu().numpy()
    assert (d[:dst_offset] == skipped).all(), "bytes before the output buffer were written"
    d = d[dst_offset:]
    ln, cr = ln.cpu().numpy().view(np.uint32), cr.cpu().numpy().view(np.uint32)
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
    return streams, [int(c) for c in cr]


def _equal(data, tile, got, want):
    streams, crcs = got
    assert len(streams) == len(want)
    for i, (s, (w, crc, info)) in enumerate(zip(streams, want)):
        assert len(s) == len(w) and s == w, "tile %d of %d: %s" % (i, len(want), explain(s, w) if i + 1 == len(want) else
                                                                   "%d bytes against the model's %d" % (len(s), len(w)))
        assert crcs[i] == crc == zlib.crc32(data[i * tile:(i + 1) * tile]), i


@lru_cache(maxsize=None)
def _grid_text(n):
    return planted_fastq(n, 20)


@pytest.mark.parametrize("name", sorted(NAMED_HIST))
def test_kernel_equals_the_model_on_the_named_inputs(name):
    text, tile, hist, level, want = named_hist(name)
    _equal(text, tile, launch_hist(text, tile, hist, level), want)
    other = 3 - level                               # the other level on the same launch
    _equal(text, tile, launch_hist(text, tile, hist, other), launch_streams(text, tile, hist, other))


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("hist", HISTS)
@pytest.mark.parametrize("tile", TILES)
def test_launches_of_three_tiles_and_17_bytes(tile, hist, level):
    assert tile + hist <= 65536
    text = _grid_text(3 * tile + 17)
    want = launch_streams(text, tile, hist, level)
    got = launch_hist(text, tile, hist, level)
    _equal(text, tile, got, want)
    z = zlib.decompressobj(-15)
    assert z.decompress(b"".join(got[0])) == text and z.eof and z.unused_data == b""


@pytest.mark.parametrize("level", (1, 2))
def test_destination_alignments_and_an_unaligned_source(level):
    tile, hist = 4096, 65
    text = _grid_text(3 * tile + 17)
    want = launch_streams(text, tile, hist, level)
    for a in range(16):                             # (the bound, the default stride, is a multiple of 16)
        _equal(text, tile, launch_hist(text, tile, hist, level, dst_offset=a), want)
    for off in (1, 7, 15):
        _equal(text, tile, launch_hist(text, tile, hist, level, src_offset=off), want)
    _equal(text, tile, launch_hist(text, tile, hist, level, stride=tile_bound(tile) + 5, dst_offset=3, src_offset=9), want)


@pytest.mark.parametrize("level", (1, 2))
def test_no_history_is_fc2_deflate_launch_level(level):
    text = _grid_text(3 * 8192 + 17)
    d, ln, cr, stride = deflate_launch_level(text, 8192, level)
    streams, crcs = launch_hist(text, 8192, 0, level)
    assert [len(s) for s in streams] == [int(x) for x in ln] and crcs == [int(x) for x in cr]
    assert streams == [d[(i + 1) * stride:(i + 1) * stride + int(ln[i])].tobytes() for i in range(len(ln))]


@pytest.mark.parametrize("level", (1, 2))
def test_gpu_gzip_hist_writes_a_member_per_piece(level):
    tile, hist, piece = 32768, 32768, 4 << 20
    text = (_grid_text(1 << 20) * 8)[:2 * piece] + _grid_text(3 * tile + 17)
    bound = N.lib().fc2_gpu_gzip_bound(len(text), tile)
    blob = _through("fc2_gpu_gzip_hist", bound, text, tile, hist, level)
    assert gzip.decompress(blob) == text
    pos = 0
    for k in range(0, len(text), piece):
        part = text[k:k + piece]
        # the short piece against the model; a whole one against the launch itself, which the tests above hold
        # to the model (the model takes minutes over 4 MiB)
        want = b"".join(s for s, _, _ in launch_streams(part, tile, hist, level)) if len(part) < piece else \
            b"".join(launch_hist(part, tile, hist, level)[0])
        assert blob[pos:pos + 10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])
        z = zlib.decompressobj(31)
        assert z.decompress(blob[pos:]) == part and z.eof
        used = len(blob) - pos - len(z.unused_data)
        assert blob[pos + 10:pos + used - 8] == want, k
        assert blob[pos + used - 8:pos + used] == zlib.crc32(part).to_bytes(4, "little") + len(part).to_bytes(4, "little")
        pos += used
    assert pos == len(blob) and len(text) > 2 * piece
    assert _through("fc2_gpu_gzip_hist", bound, text[:3 * tile], tile, 0, level) == \
        _through("fc2_gpu_gzip_level", bound, text[:3 * tile], tile, level)
