"""fc2_gpu_bgzf: one buffer through the device writer of spliced_alignments.bam (csrc/fc2_bgzf_out.hip: upload,
deflate_kernel at tile = block, bgzf_frame_kernel, the download of exactly the piece's bytes; four pieces in
flight).  Every block is parsed and checked against zlib, any gzip reader sees the input again, the lengths
sit on both sides of a block and of a piece, random bytes take the stored form inside 64 KiB; an output
buffer one byte short is an error, not a write past its end."""
import ctypes

import numpy as np
import pytest

from bgzf_helpers import E_PARAM, E_RANGE, bam_like, check_blocks
from find_circ2_amd import _native as N

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 0xA5
BLOCK, PIECE_BLOCKS = 512, 4
PIECE = BLOCK * PIECE_BLOCKS


def gpu_bgzf(data: bytes, block: int, piece_blocks: int, cap=None):
    L = N.lib()
    bound = int(L.fc2_gpu_bgzf_bound(len(data), block))
    cap = bound if cap is None else cap
    out = (ctypes.c_uint8 * (cap + 1))()
    out[cap] = GUARD
    n = ctypes.c_uint64(0)
    src = ctypes.create_string_buffer(data, len(data)) if data else None
    rc = L.fc2_gpu_bgzf(0, src, len(data), block, piece_blocks, out, cap, ctypes.byref(n))
    assert out[cap] == GUARD, "a byte past the buffer was written"
    return rc, bytes(bytearray(out)[:int(n.value)]), bound


@pytest.fixture(scope="module")
def records():
    return bam_like(200 * 1024)


@pytest.mark.parametrize("n", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, PIECE - 1, PIECE, PIECE + 1, 9 * PIECE + 3 * BLOCK + 7])
def test_gpu_bgzf_lengths_around_blocks_and_pieces(records, n):
    data = records[:n]
    rc, out, bound = gpu_bgzf(data, BLOCK, PIECE_BLOCKS)
    assert rc == 0 and len(out) <= bound
    assert (len(out) == 0) == (n == 0)
    check_blocks(out, data, BLOCK)


def test_gpu_bgzf_bam_records_at_the_default_block(records):
    rc, out, bound = gpu_bgzf(records, 0xff00, 0)
    assert rc == 0 and len(out) <= bound
    check_blocks(out, records, 0xff00)
    assert len(out) < len(records) * 0.9         # (the records were compressed, not stored)


def test_gpu_bgzf_random_bytes_are_stored_inside_64k():
    data = bytes(np.random.default_rng(3).integers(0, 256, 200 * 1024, dtype=np.uint8))
    rc, out, bound = gpu_bgzf(data, 0xff00, 2)
    assert rc == 0 and len(out) <= bound
    blocks = check_blocks(out, data, 0xff00)
    assert all(b[0] <= 65536 for b in blocks)
    assert [b[0] for b in blocks[:-1]] == [0xff00 + 5 + 26] * (len(blocks) - 1)


def test_gpu_bgzf_output_one_byte_short(records):
    data = records[:3 * PIECE + 100]
    rc, out, _ = gpu_bgzf(data, BLOCK, PIECE_BLOCKS)
    assert rc == 0
    rc2, _, _ = gpu_bgzf(data, BLOCK, PIECE_BLOCKS, cap=len(out) - 1)        # (gpu_bgzf checks the guard byte)
    assert rc2 == E_RANGE
    rc3, out3, _ = gpu_bgzf(data, BLOCK, PIECE_BLOCKS, cap=len(out))         # exactly enough
    assert rc3 == 0 and out3 == out


def test_gpu_bgzf_bad_arguments():
    L = N.lib()
    n = ctypes.c_uint64(0)
    out = (ctypes.c_uint8 * 128)()
    src = ctypes.create_string_buffer(b"abc", 3)
    assert L.fc2_gpu_bgzf(0, src, 3, 0, 4, out, 128, ctypes.byref(n)) == E_PARAM
    assert L.fc2_gpu_bgzf(0, src, 3, 0xff01, 4, out, 128, ctypes.byref(n)) == E_PARAM
    assert L.fc2_gpu_bgzf(0, src, 3, 512, 1025, out, 128, ctypes.byref(n)) == E_PARAM
    assert L.fc2_gpu_bgzf(0, None, 3, 512, 4, out, 128, ctypes.byref(n)) == E_PARAM
    assert L.fc2_gpu_bgzf(0, src, 3, 512, 4, None, 128, ctypes.byref(n)) == E_PARAM
    assert L.fc2_gpu_bgzf(-1, src, 3, 512, 4, out, 128, ctypes.byref(n)) == E_PARAM
    assert L.fc2_gpu_bgzf_bound(3, 0) == 0 and L.fc2_gpu_bgzf_bound(3, 0xff01) == 0
