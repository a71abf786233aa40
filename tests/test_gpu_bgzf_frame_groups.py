"""bgzf_groups_scan_kernel and bgzf_groups_kernel (fc2_bgzf_frame_groups_launch, csrc/fc2_bgzf_out.hip) against
fc2_bgzf_frame_groups_host, the same rule compiled for the host: the bytes, the offsets and the total on the sweep
of tests/test_bgzf_frame_groups_host.py (1, 2, 3 and 65 groups of 1, 2, 4 and 16 tiles, a last tile of one byte),
the output at the 16 shifts, streams of one byte and up to the bound, the canary around the output intact; an
invalid out_len, and a block of valid tiles past 65536 bytes, leave the output unwritten; arguments that cannot be
a piece are refused before anything is launched."""
import ctypes

import numpy as np
import pytest

from bgzf_groups_helpers import SWEEP_GROUPS, SWEEP_TPG, sweep_case, tiles_of
from bgzf_helpers import CANARY, E_PARAM, GAVE_UP, stride_of, tile_bound
from find_circ2_amd import _native as N
from test_bgzf_frame_groups_host import frame_groups_host

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def frame_groups_gpu(slots, stride, out_len, crc, n_bytes, group, tile, room, out_shift=0, n_tiles=None):
    """As frame_groups_host, on the device; the output starts out_shift bytes into a 16-byte-aligned allocation."""
    dev = torch.device("cuda:0")
    n = len(out_len) if n_tiles is None else n_tiles
    n_groups = -(-n_bytes // group)
    d_slots = torch.tensor(np.ascontiguousarray(slots), device=dev)
    d_len = torch.tensor(np.ascontiguousarray(out_len, np.uint32).view(np.int32), device=dev)
    d_crc = torch.tensor(np.ascontiguousarray(crc, np.uint32).view(np.int32), device=dev)
    d_out = torch.full((out_shift + room + 64,), CANARY, dtype=torch.uint8, device=dev)
    d_off = torch.full((n_groups + 2,), -7, dtype=torch.int32, device=dev)
    d_total = torch.full((1,), -7, dtype=torch.int32, device=dev)
    assert d_slots.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = N.lib().fc2_bgzf_frame_groups_launch(d_slots.data_ptr(), stride, d_len.data_ptr(), d_crc.data_ptr(), n, n_bytes,
                                              group, tile, d_out.data_ptr() + out_shift, d_off.data_ptr(), d_total.data_ptr(),
                                              ctypes.c_void_p(stream))
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    assert (out[:out_shift] == CANARY).all(), "bytes before the output were written"
    off = d_off.cpu().numpy().view(np.uint32)
    assert off[n_groups + 1] == 0xFFFFFFF9, "an offset past the groups' was written"
    return rc, out[out_shift:], off[:n_groups + 1], int(d_total.cpu().numpy().view(np.uint32)[0])


@pytest.mark.parametrize("tpg", SWEEP_TPG)
@pytest.mark.parametrize("n_groups", SWEEP_GROUPS)
def test_groups_kernels_give_the_host_forms_bytes(n_groups, tpg):
    case = sweep_case(n_groups, tpg)
    room = 26 * n_groups + int(sum(int(x) for x in case[2]))
    rc0, want, want_off, want_total = frame_groups_host(*case, room)
    assert rc0 == 0 and want_total == room
    for shift in ((0, 5) if (n_groups, tpg) != (3, 4) else range(16)):
        rc, out, off, total = frame_groups_gpu(*case, room, out_shift=shift)
        assert rc == 0 and total == want_total
        assert np.array_equal(off, want_off)
        assert np.array_equal(out[:total], want[:total])
        assert (out[total:] == CANARY).all(), "bytes after total were written"


def test_groups_kernels_long_and_short_streams():
    """Streams of one byte, of thousands and at the bound: the whole 16-byte stores between the two ends, every
    tile's destination where the one before ended."""
    group, tile = 0xff00, 0xff00 // 4
    stride = stride_of(tile)
    rng = np.random.default_rng(77)
    lens = [tile + 16, 4097, 16, 15,   1, 1, 1, 1,   17, 16000, 1, 31,   32, 33, tile + 5, 9999,   4096, 47]
    n_bytes = 4 * group + tile + 1
    assert tiles_of(n_bytes, group, tile) == len(lens)
    slots = rng.integers(0, 256, (len(lens) + 1) * stride, dtype=np.uint8)
    crc = rng.integers(0, 1 << 32, len(lens), dtype=np.uint64).astype(np.uint32)
    room = 26 * 5 + sum(lens)
    rc0, want, want_off, want_total = frame_groups_host(slots, stride, lens, crc, n_bytes, group, tile, room)
    for shift in (0, 3, 13):
        rc, out, off, total = frame_groups_gpu(slots, stride, lens, crc, n_bytes, group, tile, room, out_shift=shift)
        assert rc0 == rc == 0 and total == want_total == room
        assert np.array_equal(off, want_off) and np.array_equal(out, want)
        assert (out[total:] == CANARY).all()


@pytest.mark.parametrize("n_groups,tpg", [(1, 1), (1, 16), (65, 4)])
def test_groups_kernels_invalid_tile_leaves_the_output_unwritten(n_groups, tpg):
    slots, stride, out_len, crc, n_bytes, group, tile = sweep_case(n_groups, tpg)
    n = len(out_len)
    for bad in (GAVE_UP, 0, tile_bound(tile) + 1):
        for at in sorted({0, n // 3, n - 1}):
            ln = out_len.copy()
            ln[at] = bad
            rc, out, off, total = frame_groups_gpu(slots, stride, ln, crc, n_bytes, group, tile, n_groups * 2048)
            assert rc == 0 and total == 0 and not off.any()
            assert (out == CANARY).all(), "an unwritten piece was written"


def test_groups_kernels_a_block_past_64k_leaves_the_piece_unwritten():
    group, tile = 0xff00, 0xff00 // 16
    stride = stride_of(tile)
    n_bytes = 2 * group + 5
    n = tiles_of(n_bytes, group, tile)
    slots = np.zeros((n + 1) * stride, np.uint8)
    crc = np.arange(n, dtype=np.uint32)
    ln = np.full(n, 100, np.uint32)
    ln[16:32] = [4096] * 15 + [65510 - 15 * 4096]   # the second block: exactly 65536 bytes
    rc0, want, want_off, want_total = frame_groups_host(slots, stride, ln, crc, n_bytes, group, tile, 3 * 65536)
    rc, out, off, total = frame_groups_gpu(slots, stride, ln, crc, n_bytes, group, tile, 3 * 65536)
    assert rc == rc0 == 0 and total == want_total == 1626 + 65536 + 126
    assert np.array_equal(off, want_off) and np.array_equal(out, want)
    ln[31] += 1                                     # every tile valid, the block one byte past 65536
    rc, out, off, total = frame_groups_gpu(slots, stride, ln, crc, n_bytes, group, tile, 3 * 65536)
    assert rc == 0 and total == 0 and not off.any()
    assert (out == CANARY).all(), "an unwritten piece was written"


def test_groups_launch_refuses_what_cannot_be_a_piece():
    slots, stride, out_len, crc, n_bytes, group, tile = sweep_case(2, 4)
    n = len(out_len)
    for args, kw in [((slots, stride, out_len, crc, n_bytes, group, tile), {"n_tiles": n - 1}),
                     ((slots, stride, out_len, crc, n_bytes, 17 * tile, tile), {"n_tiles": 17}),
                     ((slots, stride + 8, out_len, crc, n_bytes, group, tile), {})]:     # slots off the 16-byte boundaries
        rc, out, off, total = frame_groups_gpu(*args, room=4096, **kw)
        assert rc == E_PARAM
        assert (out == CANARY).all()
