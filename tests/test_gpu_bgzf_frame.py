"""bgzf_frame_kernel (fc2_bgzf_frame_launch, csrc/fc2_bgzf_out.hip) against fc2_bgzf_frame_host, the same rule
compiled for the host: the bytes, the offsets and the total on the sweep of tests/test_bgzf_frame_host.py
(every destination alignment, a tile of the stored form's length, a short last tile), the canary after the
output intact; each invalid out_len leaves the output unwritten; arguments that cannot be a piece are refused
before anything is launched."""
import ctypes

import numpy as np
import pytest

from bgzf_helpers import CANARY, E_PARAM, SWEEP_TILES, invalid_lengths, sweep_case, tile_bound
from find_circ2_amd import _native as N
from test_bgzf_frame_host import frame_host

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def frame_gpu(slots, stride, out_len, crc, n_bytes, tile, room, out_shift=0):
    """As frame_host, on the device; the output starts out_shift bytes into a 16-byte-aligned allocation."""
    dev = torch.device("cuda:0")
    n = len(out_len)
    d_slots = torch.tensor(np.ascontiguousarray(slots), device=dev)
    d_len = torch.tensor(np.ascontiguousarray(out_len, np.uint32).view(np.int32), device=dev)
    d_crc = torch.tensor(np.ascontiguousarray(crc, np.uint32).view(np.int32), device=dev)
    d_out = torch.full((out_shift + room + 64,), CANARY, dtype=torch.uint8, device=dev)
    d_off = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    d_total = torch.full((1,), -7, dtype=torch.int32, device=dev)
    assert d_slots.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = N.lib().fc2_bgzf_frame_launch(d_slots.data_ptr(), stride, d_len.data_ptr(), d_crc.data_ptr(), n, n_bytes, tile,
                                       d_out.data_ptr() + out_shift, d_off.data_ptr(), d_total.data_ptr(),
                                       ctypes.c_void_p(stream))
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    assert (out[:out_shift] == CANARY).all(), "bytes before the output were written"
    return rc, out[out_shift:], d_off.cpu().numpy().view(np.uint32), int(d_total.cpu().numpy().view(np.uint32)[0])


@pytest.mark.parametrize("n_tiles", SWEEP_TILES)
def test_frame_kernel_gives_the_host_forms_bytes(n_tiles):
    case = sweep_case(n_tiles)
    room = int(sum(26 + int(x) for x in case[2]))
    rc0, want, want_off, want_total = frame_host(*case, room)
    assert rc0 == 0 and want_total == room
    for shift in (0, 5):                         # the first block itself at two alignments
        rc, out, off, total = frame_gpu(*case, room, out_shift=shift)
        assert rc == 0 and total == want_total
        assert np.array_equal(off, want_off)
        assert np.array_equal(out[:total], want[:total])
        assert (out[total:] == CANARY).all(), "bytes after total were written"


def test_frame_kernel_long_streams():
    """Streams of thousands of bytes: the whole 16-byte stores between the two ends, at every alignment."""
    tile = 0xff00
    stride = (tile_bound(tile) + 15) & ~15
    rng = np.random.default_rng(77)
    lens = [tile + 5, 4097, 16, 15, 17, 33000, 1, 31, 32, 33, 65000, 20001, 9999, 4096, 47, 48, 49, 12345]
    slots = rng.integers(0, 256, len(lens) * stride, dtype=np.uint8)
    crc = rng.integers(0, 1 << 32, len(lens), dtype=np.uint64).astype(np.uint32)
    n_bytes = (len(lens) - 1) * tile + 1
    room = sum(26 + x for x in lens)
    rc0, want, want_off, want_total = frame_host(slots, stride, lens, crc, n_bytes, tile, room)
    rc, out, off, total = frame_gpu(slots, stride, lens, crc, n_bytes, tile, room, out_shift=3)
    assert rc0 == rc == 0 and total == want_total == room
    assert np.array_equal(off, want_off) and np.array_equal(out, want)
    assert (out[total:] == CANARY).all()


@pytest.mark.parametrize("n_tiles", [1, 65])
def test_frame_kernel_invalid_tile_leaves_the_output_unwritten(n_tiles):
    slots, stride, out_len, crc, n_bytes, tile = sweep_case(n_tiles)
    for bad in invalid_lengths(tile):
        ln = out_len.copy()
        ln[n_tiles // 3] = bad
        rc, out, off, total = frame_gpu(slots, stride, ln, crc, n_bytes, tile, n_tiles * (26 + tile_bound(tile)))
        assert rc == 0 and total == 0 and not off.any()
        assert (out == CANARY).all(), "an unwritten piece was written"


def test_frame_launch_refuses_what_cannot_be_a_piece():
    slots, stride, out_len, crc, n_bytes, tile = sweep_case(2)
    big = 0xff00 + 1
    big_stride = (tile_bound(big) + 15) & ~15
    for args in [(np.zeros(2 * big_stride, np.uint8), big_stride, out_len, crc, big + 1, big),
                 (slots, stride, out_len, crc, 2 * tile + 1, tile),
                 (slots, stride + 8, out_len, crc, n_bytes, tile)]:              # slots off the 16-byte boundaries
        rc, out, off, total = frame_gpu(*args, room=4096)
        assert rc == E_PARAM
        assert (out == CANARY).all()
