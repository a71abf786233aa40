"""sam_size_kernel, sam_scan_kernel and sam_write_kernel (fc2_sam_encode_launch, csrc/fc2_sam_encode.hip) against
fc2_sam_encode_host, the same rule compiled for the host: status, size, out_off, total and every output byte on
the planted lines, the refused ones and 2,000 of the mutations, in batches of 1, 2, 63, 64, 65 and 1000 lines, a
40,000-base line alone and between short ones, the canary after the total intact; at the batch's limits -- the scan's shares
of 1 to 16 sizes with ragged tails, exactly 4 MiB of text, offsets that are no lines among good ones, offsets that
repeat one long line until the sizes pass out_cap; and fc2_gpu_sam_encode: nine batches through the four slots, and
batches cut by the text cap, by a line no batch holds and made of refused lines only, the records in order and the
host rule's."""
import ctypes

import numpy as np
import pytest

from find_circ2_amd import _native as N
from sam_encode_helpers import (CANARY, E_PARAM, ENC_LONG, ENC_OFFSETS, MAX_LINES, MAX_TEXT, NAMES, bound, bwa_lines, c_names,
                                encode_host, encode_host_all, encode_host_packed, mutations, names_table, pack, planted_lines,
                                refused_lines, sam_line)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def launch(text, nb, off, table):
    """fc2_sam_encode_launch on `nb` bytes of text under any len(off) - 1 offsets: (rc, status, size, out_off, total,
    the output with 64 canary bytes after the bound); every table -7 (0xFFFFFFF9) where nothing was stored."""
    dev = torch.device("cuda:0")
    n = len(off) - 1
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
    torch.cuda.synchronize(dev)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    return rc, u32(d_status), u32(d_size), u32(d_out_off), int(u32(d_total)[0]), d_out.cpu().numpy()


def encode_gpu(lines, table):
    """As encode_host, on the device."""
    text, off = pack(lines)
    rc, *got = launch(text, int(off[-1]), off, table)
    assert rc == 0, N.lib().fc2_last_error()
    return tuple(got)


def same(got, want):
    assert np.array_equal(got[0], want[0]), "status"
    assert np.array_equal(got[1], want[1]), "size"
    assert np.array_equal(got[2], want[2]), "out_off"
    assert got[3] == want[3], "total"
    assert np.array_equal(got[4], want[4]), "the output's bytes (the canary after the total among them)"
    assert (got[4][got[3]:] == CANARY).all()
    return want


def same_as_host(lines, table):
    return same(encode_gpu(lines, table), encode_host(lines, NAMES, table))


def same_as_host_packed(text, nb, off, table):
    """same_as_host for offsets that pack() does not make."""
    rc, *got = launch(text, nb, off, table)
    assert rc == 0, N.lib().fc2_last_error()
    return same(tuple(got), encode_host_packed(text, nb, off, table))


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


@pytest.fixture(scope="module")
def short_lines():
    """16384 bwa-shaped lines of 50 bases (at most 250 bytes: under 4 MiB together), every 7th refused."""
    lines = [l + b"\tXF:f:0.5" if k % 7 == 3 else l for k, l in enumerate(bwa_lines(MAX_LINES, seed=21, read_len=50))]
    assert max(len(l) for l in lines) <= 250
    return lines


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2049, 16383, 16384])
def test_scan_shares_of_up_to_16_sizes(table, short_lines, n):
    """sam_scan_kernel's 1024 threads with 1, 2, 3 and 16 sizes each, the last shares short or empty, sizes of 0
    among the others."""
    status = same_as_host(short_lines[:n], table)[0]
    assert list(np.nonzero(status)[0]) == list(range(3, n, 7))


def test_exactly_4_mib_of_text_and_one_byte_more(table):
    lines = bwa_lines(12000, seed=23)
    room = MAX_TEXT - sum(len(l) for l in lines)
    assert room > 1000
    last = sam_line(tags=[b"XZ:Z:"])
    lines.append(last + bytes(65 + k % 26 for k in range(room - len(last))))
    text, off = pack(lines)
    assert int(off[-1]) == MAX_TEXT
    assert not same_as_host_packed(text, MAX_TEXT, off, table)[0].any()
    # a byte more is refused before anything is launched: no table is touched
    text = np.append(text, np.uint8(65))
    off[-1] += 1
    rc, status, size, out_off, total, out = launch(text, MAX_TEXT + 1, off, table)
    assert rc == E_PARAM
    untouched = np.uint32(-7 & 0xFFFFFFFF)
    assert (status == untouched).all() and (size == untouched).all() and (out_off == untouched).all() and total == untouched
    assert (out == CANARY).all()


def test_offsets_that_are_no_lines_among_good_ones(table):
    lines = bwa_lines(12, seed=25)
    text, off = pack(lines)
    nb = int(off[-1])
    good = encode_host(lines, NAMES, table)
    rec = lambda r, k: r[4][int(r[2][k]):int(r[2][k]) + int(r[1][k])].tobytes()
    # an offset past the text: the line that ends there is past it, the line that begins there descends
    past = off.copy()
    past[5] = nb + 100
    got = same_as_host_packed(text, nb, past, table)
    assert list(np.nonzero(got[0])[0]) == [4, 5] and list(got[0][4:6]) == [ENC_OFFSETS] * 2 and not got[1][4:6].any()
    assert all(rec(got, k) == rec(good, k) for k in range(12) if k not in (4, 5))
    # an offset below the one before it: line 4 descends, line 5 begins inside line 2 (whatever the rule makes of it)
    desc = off.copy()
    desc[5] = off[2] + 10
    got = same_as_host_packed(text, nb, desc, table)
    assert got[0][4] == ENC_OFFSETS and got[1][4] == 0
    assert all(got[0][k] == 0 and rec(got, k) == rec(good, k) for k in range(12) if k not in (4, 5))
    # a text that ends before the last line does
    got = same_as_host_packed(text, nb - 1, off, table)
    assert list(np.nonzero(got[0])[0]) == [11] and got[0][11] == ENC_OFFSETS and got[1][11] == 0
    assert all(rec(got, k) == rec(good, k) for k in range(11))


def test_zigzag_offsets_whose_sizes_pass_out_cap(table):
    """off = [0, T, 0, T, ...]: every even line the same accepted one, every odd line refused, the sizes' sum far
    past out_cap (FC2_SAM_ENC_BOUND of T bytes): the records that fit are written, the rest left out, nothing
    past out_cap."""
    rng = np.random.default_rng(27)
    line = sam_line(seq=bytes(rng.choice(list(b"ACGTN"), 30000).astype(np.uint8)),
                    qual=bytes(rng.integers(33, 74, 30000).astype(np.uint8)), cigar=b"30000M", tags=[b"NM:i:3"])
    text, _ = pack([line])
    T, n = len(line), 2000
    off = np.zeros(n + 1, np.uint32)
    off[1::2] = T
    status, size, out_off, total, out = same_as_host_packed(text, T, off, table)
    cap = bound(T, n)
    assert list(status) == [0, ENC_OFFSETS] * (n // 2) and size[0] > 45000 and list(size) == [size[0], 0] * (n // 2)
    assert total == int(size[0]) * (n // 2) > 100 * cap
    fit = cap // int(size[0])
    assert fit >= 2 and out[:fit * int(size[0])].tobytes() == out[:int(size[0])].tobytes() * fit
    assert (out[fit * int(size[0]):] == CANARY).all()       # what does not fit whole is not begun


def test_gpu_sam_encode_batches_cut_by_the_text_cap_a_long_line_and_refusals(table):
    """batch_lines = 0: 16,000 lines of 5 MB (the text cap cuts the first batch), a line of 4 MiB + 1 (status 8, no
    room), a batch of refused lines only between two such lines (total 0), and 16,000 lines again: five batches or
    more, so a slot is filled twice."""
    base = bwa_lines(4000, seed=29)
    too_long = sam_line(tags=[b"XZ:Z:"])
    too_long += b"z" * (MAX_TEXT + 1 - len(too_long))
    lines = base * 4 + [too_long] + [l + b"\tXF:f:0.5" for l in base[:300]] + [too_long] + base * 4
    assert sum(len(l) for l in base) * 4 > MAX_TEXT
    text, off = pack(lines)
    n, nb = len(lines), int(off[-1])
    cap = bound(nb, n)
    out = np.full(cap + 64, CANARY, np.uint8)
    status = np.full(n, 0xDEADBEEF, np.uint32)
    out_n = ctypes.c_uint64()
    rc = N.lib().fc2_gpu_sam_encode(0, text.ctypes.data, off.ctypes.data, n, c_names(NAMES), len(NAMES), 0, out.ctypes.data,
                                    cap, ctypes.byref(out_n), status.ctypes.data)
    assert rc == 0, N.lib().fc2_last_error()
    st, recs = encode_host_all(lines)
    assert list(status) == st
    assert [i for i, s in enumerate(st) if s == ENC_LONG] == [16000, 16301]
    assert all(st[16001:16301]) and not any(st[:16000]) and not any(st[16302:])
    want = b"".join(r for r in recs if r is not None)
    assert out_n.value == len(want) and out[:len(want)].tobytes() == want
    assert (out[len(want):] == CANARY).all()
