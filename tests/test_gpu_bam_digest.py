"""The record digests made on the GPU (fc2_bam_digest_launch, csrc/fc2_inflate.hip bam_digest_kernel)
against the CPU's (fc2_bam_digest_host), row for row: the hand-built records of test_bam_digest_host.py
as one stream cut into small blocks, a seeded fuzz of a real record stream in blocks of 1-4 kB (a third
of them damaged, the lists fc2_bam_walk_host's), blocks with a non-zero status, a stream that ends inside
its last record, and launches of 1, 2, 65 and 1024 blocks.  Every launch has guard bytes around the
stream and guard rows around `rows` and `first`: the input is unchanged and nothing but the counted rows
and first[0 .. n_blocks] is written."""
import ctypes
import struct

import numpy as np
import pytest

from find_circ2_amd import _native as N
from test_bam_digest_host import ROW, cases, host_digest, rec
from test_bam_walk_host import CAP, host_walk

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64                # guard bytes either side of the stream, guard rows either side of the rows
FILL = 0xA5


def digest_launch(data: bytes, sizes, starts, status=None, n_bytes=None, shift=0, counts=None):
    """fc2_bam_digest_launch over `data` cut into blocks of `sizes`, block i's listed starts (offsets into
    the block) starts[i]; the stream lies `shift` bytes past an aligned address.  Returns (first, rows):
    first[0 .. n] and the counted rows, after the checks of the module's docstring.  `counts`: the count
    words handed to the kernel when they are not len(starts[i])."""
    n = len(sizes)
    dev = torch.device("cuda:0")
    n_bytes = len(data) if n_bytes is None else n_bytes
    rng = np.random.default_rng(n)
    lead = GUARD + shift
    host = rng.integers(0, 256, lead + len(data) + GUARD, dtype=np.uint8)
    host[lead:lead + len(data)] = np.frombuffer(data, np.uint8)
    ooff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    table = np.full((n, CAP), 0xFFFF, np.uint16)                  # (unlisted entries: offsets never to be read)
    for i, st in enumerate(starts):
        table[i, :len(st)] = st
    counts = np.array([len(st) for st in starts] if counts is None else counts, np.uint32)
    total = int(np.minimum(counts, CAP).sum())
    d_bytes = torch.tensor(host, device=dev)
    as_i32 = lambda a: torch.tensor(np.ascontiguousarray(a).view(np.int32), device=dev)  # noqa: E731
    d_ooff, d_isize, d_count = as_i32(ooff[:n]), as_i32(np.array(sizes, np.uint32)), as_i32(counts)
    d_status = None if status is None else as_i32(np.array(status, np.uint32))
    d_starts = torch.tensor(table.view(np.int16), device=dev)
    d_rows = torch.full(((total + 2 * GUARD) * 32,), FILL, dtype=torch.uint8, device=dev)
    d_first = torch.tensor(np.full(n + 1 + 2 * GUARD, 0x5AA5C33C, np.uint32).view(np.int32), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().fc2_bam_digest_launch(d_bytes.data_ptr() + lead, n_bytes, d_ooff.data_ptr(), d_isize.data_ptr(),
                                          None if d_status is None else d_status.data_ptr(), d_starts.data_ptr(),
                                          d_count.data_ptr(), d_rows.data_ptr() + GUARD * 32,
                                          d_first.data_ptr() + GUARD * 4, n, ctypes.c_void_p(stream)))
    torch.cuda.synchronize(dev)
    assert (d_bytes.cpu().numpy() == host).all(), "the stream was written"
    rows = d_rows.cpu().numpy()
    first = d_first.cpu().numpy().view(np.uint32)
    assert (rows[:GUARD * 32] == FILL).all() and (rows[(GUARD + total) * 32:] == FILL).all(), "a guard row was written"
    assert (first[:GUARD] == 0x5AA5C33C).all() and (first[GUARD + n + 1:] == 0x5AA5C33C).all(), "a guard word was written"
    first = first[GUARD:GUARD + n + 1]
    assert [int(x) for x in first] == [int(x) for x in np.concatenate([[0], np.cumsum(np.minimum(counts, CAP))])]
    return first, rows[GUARD * 32:(GUARD + total) * 32].view(ROW)


def host_rows(data: bytes, n_bytes, sizes, starts):
    """fc2_bam_digest_host for every listed start, in row order."""
    buf = np.frombuffer(data, np.uint8).copy() if data else np.zeros(1, np.uint8)
    out, o = [], 0
    for sz, st in zip(sizes, starts):
        out += [host_digest(buf, n_bytes, o + s) for s in st]
        o += sz
    return out


def as_tuples(rows):
    return [tuple(int(x) for x in r) for r in rows.tolist()]


def cut(n_total, block):
    return [min(block, n_total - o) for o in range(0, n_total, block)]


def lists_of(offsets, sizes):
    """Stream offsets as per-block lists of offsets into the block."""
    edges = np.concatenate([[0], np.cumsum(sizes)])
    out = [[] for _ in sizes]
    for o in offsets:
        j = int(np.searchsorted(edges, o, side="right")) - 1
        out[j].append(int(o - edges[j]))
    return out


def hand_stream():
    """The hand-built records one behind the other (a byte between some, so every residue occurs):
    (stream, record starts, labels, states)."""
    data, at, labels, states = bytearray(), [], [], []
    for k, (label, r, state) in enumerate(cases()):
        data += b"\xEE" * (k % 3 == 0)
        at.append(len(data))
        data += r
        labels.append(label)
        states.append(state)
    return bytes(data) + b"\x11" * 7, at, labels, states


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("block", [97, 4000])
def test_hand_built_stream(shift, block):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    data, at, labels, states = hand_stream()
    sizes = cut(len(data), block)
    starts = lists_of(at, sizes)
    _, rows = digest_launch(data, sizes, starts, shift=shift)
    got, want = as_tuples(rows), host_rows(data, len(data), sizes, starts)
    for g, w, label, state in zip(got, want, labels, states):
        assert g == w, (label, g, w)
        assert g[0] == state, (label, g)
    assert {a % 4 for a in at} == {0, 1, 2, 3}
    edges = np.cumsum(sizes)
    if block == 97:                     # several records straddle a cut, and are digested all the same
        straddle = [k for k, a in enumerate(at) if states[k] and np.searchsorted(edges, a, side="right") !=
                    np.searchsorted(edges, a + len(cases()[k][1]) - 1, side="right")]
        assert len(straddle) > 20


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    """~200 consecutive blocks of 1-4 kB of the record stream of a bwa-mem-like BAM, a third of them with
    a few bytes overwritten; the lists are fc2_bam_walk_host's of each block, the rows the CPU's."""
    from samgen import sam_to_bam
    from test_native_caller import _rich_sam
    tmp = tmp_path_factory.mktemp("digest_fuzz")
    sam, raw = str(tmp / "rich.sam"), str(tmp / "raw.bam")
    _rich_sam(sam, 4000, seed=7)
    sam_to_bam(open(sam).read(), raw, compress="none")
    whole = open(raw, "rb").read()
    rng = np.random.default_rng(77)
    sizes = [int(rng.integers(1000, 4001)) for _ in range(200)]
    a = int(rng.integers(0, len(whole) - sum(sizes)))
    data = bytearray(whole[a:a + sum(sizes)])
    o = 0
    for k, sz in enumerate(sizes):
        if k % 3 == 0:
            for _ in range(int(rng.integers(1, 6))):
                data[o + int(rng.integers(0, sz))] = int(rng.integers(0, 256))
        o += sz
    data = bytes(data)
    starts, o = [], 0
    for sz in sizes:
        starts.append(host_walk(data[o:o + sz])[2])
        o += sz
    return data, sizes, starts, host_rows(data, len(data), sizes, starts)


def test_fuzz_equals_the_host_digest(fuzz):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    data, sizes, starts, want = fuzz
    _, rows = digest_launch(data, sizes, starts, shift=3)
    got = as_tuples(rows)
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:5], [(got[k], want[k]) for k in bad[:5]])
    assert sum(w[0] for w in want) > len(want) / 2 > 1000
    edges = np.concatenate([[0], np.cumsum(sizes)])
    at = [int(edges[i]) + s for i, st in enumerate(starts) for s in st]
    blk = [i for i, st in enumerate(starts) for _ in st]
    spans = sum(1 for a, i, w in zip(at, blk, want) if w[0] and a + 4 + w[4] > edges[i + 1])
    assert spans > 50
    assert {a % 4 for a, w in zip(at, want) if w[0]} == {0, 1, 2, 3}
    assert any(w[1] for w in want) and any(w[2] for w in want)


def test_records_touching_a_refused_block_are_left_to_the_host(fuzz):
    """Random blocks with status != 0: a record any of whose bytes lies in one gets state 0 (its block_size
    kept), every other row is as without a status array."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    data, sizes, starts, want = fuzz
    rng = np.random.default_rng(5)
    status = [int(rng.integers(1, 17)) if rng.random() < 0.25 else 0 for _ in sizes]
    status[0], status[1], status[-1] = 7, 0, 16
    _, rows = digest_launch(data, sizes, starts, status=status)
    got = as_tuples(rows)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    k = own = later = kept = 0
    for i, st in enumerate(starts):
        for s in st:
            w = want[k]
            if w[0]:
                end = int(edges[i]) + s + 4 + w[4]
                touched = [j for j in range(i, len(sizes)) if j == i or edges[j] < end]
                if any(status[j] for j in touched):
                    w = (0, 0, 0, 0, w[4], 0, 0, 0, 0, 0)
                    own += bool(status[i])
                    later += not status[i]                 # (refused only through a later block)
                else:
                    kept += 1
            assert got[k] == w, (i, s, got[k], w)
            k += 1
    assert own > 100 and later > 5 and kept > 500, (own, later, kept)


def test_stream_ends_inside_the_last_record():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    recs = [rec(tags=b"ASC\x30XSC\x10"), rec(((4, 6), (0, 44))), rec(tags=b"ASC\x31MDZ" + b"5" * 40 + b"\0")]
    data = b"".join(recs)
    at = [0, len(recs[0]), len(recs[0]) + len(recs[1])]
    sizes = cut(len(data), 80)
    starts = lists_of(at, sizes)
    for short in (0, 1, 2, len(recs[2]) - 5, len(recs[2]) - 3):
        n_bytes = len(data) - short
        _, rows = digest_launch(data, sizes, starts, n_bytes=n_bytes, shift=1)
        got = as_tuples(rows)
        assert got == host_rows(data, n_bytes, sizes, starts), short
        assert [g[0] for g in got] == [1, 1, int(short == 0)], (short, got)
        assert got[2][4] == (len(recs[2]) - 4 if len(recs[2]) - short >= 4 else 0)


@pytest.mark.parametrize("n_blocks", [1, 2, 65, 1024])
def test_launch_sizes(n_blocks):
    """Tiny blocks (one to three short records each, some none): first[] is the running sum of the counts
    at every launch size, the largest included."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(n_blocks)
    data, at = bytearray(), []
    while len(data) < 50 * n_blocks:
        at.append(len(data))
        data += rec(((0, 9),), l_seq=9, name=b"r%d" % len(at), tags=[b"", b"ASC\x07", b"XSs\x01\x80NMC\0"][len(at) % 3])
        data += bytes(int(rng.integers(0, 3)))
    data = bytes(data[:50 * n_blocks])                      # (the last record may be cut: state 0)
    sizes = [50] * n_blocks
    starts = lists_of(at, sizes)
    first, rows = digest_launch(data, sizes, starts)
    got = as_tuples(rows)
    assert got == host_rows(data, len(data), sizes, starts)
    assert int(first[-1]) == len(at) and sum(g[0] for g in got) >= len(at) - 1
    assert any(not st for st in starts) or n_blocks < 65


def test_counts_beyond_a_row_are_capped():
    """A count word above FC2_BAM_WALK_CAP (never the walk's, but the kernel may not trust it): CAP rows
    for that block, and the next block's rows behind them."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = rec(tags=b"ASC\x07")
    data = r + r
    sizes = [len(r), len(r)]
    starts = [[0] * CAP, [0]]
    first, rows = digest_launch(data, sizes, starts, counts=[CAP + 5, 1])
    got = as_tuples(rows)
    assert [int(x) for x in first] == [0, CAP, CAP + 1]
    assert set(got) == {host_digest(np.frombuffer(data, np.uint8).copy(), len(data), 0)} and got[0][0] == 1


def test_too_many_blocks():
    p = ctypes.c_void_p(64)
    L = N.lib()
    assert L.fc2_bam_digest_launch(p, 4, p, p, None, p, p, p, p, N.BAM_DIGEST_MAX_BLOCKS + 1, None) == N.FC2_E_PARAM
