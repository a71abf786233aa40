"""sam_size_kernel, sam_scan_kernel and sam_write_kernel (fc2_sam_encode_launch, csrc/fc2_sam_encode.hip) against
fc2_sam_encode_host, the same rule compiled for the host: status, size, out_off, total and every output byte on
the planted lines, the refused ones and 2,000 of the mutations, in batches of 1, 2, 63, 64, 65 and 1000 lines, a
40,000-base line alone and between short ones, the canary after the total intact; and fc2_gpu_sam_encode: nine
batches through the four slots, the records in order and the host rule's."""
import ctypes

import numpy as np
import pytest

from find_circ2_amd import _native as N
from sam_encode_helpers import (CANARY, NAMES, bound, bwa_lines, c_names, encode_host, mutations, names_table, pack, planted_lines,
                                refused_lines, sam_line)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def encode_gpu(lines, table):
    """As encode_host, on the device."""
    dev = torch.device("cuda:0")
    text, off = pack(lines)
    n, nb = len(lines), int(off[-1])
    cap = bound(nb, n)
    d_text = torch.tensor(text, device=dev)
    d_off = torch.tensor(off.view(np.int32), device=dev)
    d_table = torch.tensor(table.view(np.int32), device=dev)
    d_out = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device=dev)
    d_out_off = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    d_size = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_total = torch.full((1,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = N.lib().fc2_sam_encode_launch(d_text.data_ptr(), nb, d_off.data_ptr(), n, d_table.data_ptr(), table.nbytes,
                                       d_out.data_ptr(), cap, d_out_off.data_ptr(), d_size.data_ptr(), d_status.data_ptr(),
                                       d_total.data_ptr(), ctypes.c_void_p(stream))
    assert rc == 0, N.lib().fc2_last_error()
    torch.cuda.synchronize(dev)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    return u32(d_status), u32(d_size), u32(d_out_off), int(u32(d_total)[0]), d_out.cpu().numpy()


def same_as_host(lines, table):
    want = encode_host(lines, NAMES, table)
    got = encode_gpu(lines, table)
    assert np.array_equal(got[0], want[0]), "status"
    assert np.array_equal(got[1], want[1]), "size"
    assert np.array_equal(got[2], want[2]), "out_off"
    assert got[3] == want[3], "total"
    assert np.array_equal(got[4], want[4]), "the output's bytes (the canary after the total among them)"
    assert (got[4][got[3]:] == CANARY).all()
    return want


@pytest.fixture(scope="module")
def table():
    return names_table()


def test_planted_and_refused_lines(table):
    status = same_as_host(planted_lines(), table)[0]
    assert not status.any()
    status = same_as_host([c[0] for c in refused_lines()], table)[0]
    assert status.all()
    same_as_host(planted_lines() + [c[0] for c in refused_lines()], table)


def test_mutations(table):
    status = same_as_host(mutations(2000), table)[0]
    assert 200 < int((status == 0).sum()) < 1900


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_batch_shapes(table, n):
    assert not same_as_host(bwa_lines(n, seed=n), table)[0].any()


def test_a_long_read_alone_and_between_short_ones(table):
    rng = np.random.default_rng(3)
    long = sam_line(seq=bytes(rng.choice(list(b"ACGTN"), 40000).astype(np.uint8)),
                    qual=bytes(rng.integers(33, 74, 40000).astype(np.uint8)), cigar=b"20000M5000N20000M",
                    tags=[b"MD:Z:" + b"7A" * 3000])
    base = bwa_lines(3)
    assert not same_as_host([long], table)[0].any()
    assert not same_as_host([base[0], long, base[1], base[2]], table)[0].any()


def test_gpu_sam_encode_nine_batches_through_four_slots(table):
    per = 150
    lines = bwa_lines(8 * per + 17, seed=9)
    refused = {100, 5 * per + 3}
    for i in refused:
        lines[i] += b"\tXF:f:0.5"
    text, off = pack(lines)
    n, nb = len(lines), int(off[-1])
    cap = N.lib().fc2_gpu_sam_encode_bound(nb, n)
    assert cap == bound(nb, n)
    out = np.full(cap + 64, CANARY, np.uint8)
    status = np.full(n, 0xDEADBEEF, np.uint32)
    out_n = ctypes.c_uint64()
    rc = N.lib().fc2_gpu_sam_encode(0, text.ctypes.data, off.ctypes.data, n, c_names(NAMES), len(NAMES), per, out.ctypes.data,
                                    cap, ctypes.byref(out_n), status.ctypes.data)
    assert rc == 0, N.lib().fc2_last_error()
    want = b""
    for b0 in range(0, n, per):                  # the host rule, batch by batch: the records in line order
        st, size, out_off, total, o = encode_host(lines[b0:b0 + per], NAMES, table)
        assert np.array_equal(status[b0:b0 + per], st)
        want += o[:total].tobytes()
    assert set(np.nonzero(status)[0]) == refused
    assert out_n.value == len(want) and out[:len(want)].tobytes() == want
    assert (out[len(want):] == CANARY).all()
