"""fc2_gpu_bgzf_tiles: one buffer through the device writer of spliced_alignments.bam with every block cut into
tiles that share the block's history (upload, deflate_kernel over groups, the two framing kernels, the download of
exactly the piece's bytes; four pieces in flight).  On BAM-like records at lengths around a tile, a block and a
piece: any gzip reader sees the input again, each block's ISIZE and CRC-32 are right, and each block's payload is
the model's streams back to back; a tile that holds the block gives fc2_gpu_bgzf_level's bytes; random bytes in 16
tiles stay inside 64 KiB a block and come from the device; an output one byte short is an error."""
import ctypes

import numpy as np
import pytest

from bgzf_helpers import E_RANGE, bam_like, check_blocks
from deflate_model_groups import group_streams
from find_circ2_amd import _native as N

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 0xA5
BLOCK, TILE, HIST, PIECE_BLOCKS = 2000, 512, 1024, 2
PIECE = BLOCK * PIECE_BLOCKS


def gpu_bgzf_tiles(data: bytes, block, piece_blocks, tile, hist, level, cap=None, entry="fc2_gpu_bgzf_tiles"):
    L = N.lib()
    bound = int(L.fc2_gpu_bgzf_tiles_bound(len(data), block, tile))
    cap = bound if cap is None else cap
    out = (ctypes.c_uint8 * (cap + 1))()
    out[cap] = GUARD
    n = ctypes.c_uint64(0)
    src = ctypes.create_string_buffer(data, len(data)) if data else None
    if entry == "fc2_gpu_bgzf_tiles":
        rc = L.fc2_gpu_bgzf_tiles(0, src, len(data), block, piece_blocks, tile, hist, level, out, cap, ctypes.byref(n))
    else:
        rc = L.fc2_gpu_bgzf_level(0, src, len(data), block, piece_blocks, level, out, cap, ctypes.byref(n))
    assert out[cap] == GUARD, "a byte past the buffer was written"
    return rc, bytes(bytearray(out)[:int(n.value)]), bound


@pytest.fixture(scope="module")
def records():
    return bam_like(200 * 1024)


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, BLOCK - 1, BLOCK, BLOCK + 1, PIECE - 1, PIECE, PIECE + 1,
                               9 * PIECE + BLOCK + TILE + 7])
def test_lengths_around_tiles_blocks_and_pieces(records, n, level):
    data = records[:n]
    rc, out, bound = gpu_bgzf_tiles(data, BLOCK, PIECE_BLOCKS, TILE, HIST, level)
    assert rc == 0 and len(out) <= bound
    assert (len(out) == 0) == (n == 0)
    blocks = check_blocks(out, data, BLOCK)         # ISIZE, CRC-32, a whole stream a block, gzip.decompress
    want = group_streams(data, BLOCK, TILE, HIST, level) if n else []
    assert [b[1] for b in blocks] == [b"".join(s for s, _, _ in tiles) for tiles in want]


@pytest.mark.parametrize("level", (1, 2))
def test_bam_records_at_the_default_block_in_four_tiles(records, level):
    data = records[:2 * 0xff00 + 16320 + 9]
    rc, out, bound = gpu_bgzf_tiles(data, 0xff00, 2, 16320, 32768, level)
    assert rc == 0 and len(out) <= bound
    blocks = check_blocks(out, data, 0xff00)
    want = group_streams(data, 0xff00, 16320, 32768, level)
    assert [len(t) for t in want] == [4, 4, 2]
    assert [b[1] for b in blocks] == [b"".join(s for s, _, _ in tiles) for tiles in want]
    assert len(out) < len(data) * 0.9               # (the records were compressed, not stored)


@pytest.mark.parametrize("level", (1, 2))
def test_a_tile_that_holds_the_block_is_fc2_gpu_bgzf_level(records, level):
    data = records[:3 * PIECE + BLOCK + 7]
    rc0, want, _ = gpu_bgzf_tiles(data, BLOCK, PIECE_BLOCKS, 0, 0, level, entry="fc2_gpu_bgzf_level")
    assert rc0 == 0 and want
    for tile, hist in [(0, 0), (0, HIST), (BLOCK, HIST), (BLOCK + 1, 0), (65536, 32768)]:
        rc, out, _ = gpu_bgzf_tiles(data, BLOCK, PIECE_BLOCKS, tile, hist, level)
        assert rc == 0 and out == want, (tile, hist)


def test_random_bytes_in_16_tiles_stay_inside_64k():
    data = bytes(np.random.default_rng(3).integers(0, 256, 2 * 0xff00 + 4080 + 100, dtype=np.uint8))
    rc, out, bound = gpu_bgzf_tiles(data, 0xff00, 2, 0xff00 // 16, 0, 1)
    assert rc == 0 and len(out) <= bound
    blocks = check_blocks(out, data, 0xff00)
    assert all(b[0] <= 65536 for b in blocks)
    # from the device: 16 stored tiles of 4080 + 5 bytes (zlib's fallback would write one stream a block)
    assert [b[0] for b in blocks] == [0xff00 + 16 * 5 + 26] * 2 + [4080 + 100 + 2 * 5 + 26]
    for b in blocks[:2]:
        assert all(b[1][k * 4085:k * 4085 + 5] == bytes([1 if k == 15 else 0, 0xF0, 0x0F, 0x0F, 0xF0]) for k in range(16))


def test_output_one_byte_short(records):
    data = records[:3 * PIECE + 100]
    rc, out, _ = gpu_bgzf_tiles(data, BLOCK, PIECE_BLOCKS, TILE, HIST, 1)
    assert rc == 0
    rc2, _, _ = gpu_bgzf_tiles(data, BLOCK, PIECE_BLOCKS, TILE, HIST, 1, cap=len(out) - 1)
    assert rc2 == E_RANGE
    rc3, out3, _ = gpu_bgzf_tiles(data, BLOCK, PIECE_BLOCKS, TILE, HIST, 1, cap=len(out))
    assert rc3 == 0 and out3 == out
