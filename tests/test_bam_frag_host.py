"""fc2_bam_frag_host (include/fc2_ingest.h) -- the fragment rows of a chunk's listed record starts, the
oracle of the kernel's test -- against the rule restated in Python (frag_streams.py: py_rows, on
test_bam_digest_host.py's independent record decoder), on hand-built record streams cut into blocks of
1-4 KB: every shape the rule tells apart, with the expected row written beside each (frag_streams.SCENARIOS),
at all four start residues, with a refused block, with starts missing from the lists and with a start that
does not abut its predecessor."""
import struct

import numpy as np
import pytest

import frag_streams as FS
from find_circ2_amd import _native as N


def _true_starts(data):
    o, out = 0, []
    while o < len(data):
        out.append(o)
        o += 4 + struct.unpack_from("<I", data, o)[0]
    return out


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_scenarios_have_the_rows_written_beside_them(shift):
    data, heads = FS.stream(shift)
    for cuts in ([], FS.random_cuts(len(data), np.random.default_rng(10 + shift))):
        T = FS.Tables(data, cuts)
        # (a block's own walk misses a start in the last three bytes before the block's end, and may begin at
        # a false one: cut into blocks, a row may claim nothing where the uncut stream's row does)
        if not cuts:
            assert [at for _, _, at in T.listed()] == _true_starts(data), "the lists are the stream's own records"
        rows, _ = FS.host_rows(T)
        got = dict(zip((at for _, _, at in T.listed()), FS.as_tuples(rows)))
        assert FS.as_tuples(rows) == FS.py_rows(T)
        n_claimed = 0
        for label, recs, want in FS.SCENARIOS:
            row = got.get(heads[label], (0, 0, 0, 0, 0))
            if want is None or (cuts and row[0] == 0):
                assert row == (0, 0, 0, 0, 0), (label, row)
            else:
                n_claimed += 1
                assert row[:4] == want, (label, row)
                end = heads[label] + sum(len(FS.rec(r[0], r[1], r[2])) for r in recs[:want[1]])
                assert row[4] == end - heads[label], (label, row)
        assert n_claimed >= 8
        assert got[0] == (0, 0, 0, 0, 0), "the chunk's first record has nothing before it"


def test_start_residues_are_all_met():
    seen = set()
    for shift in range(4):
        _, heads = FS.stream(shift)
        seen |= {(label, at % 4) for label, at in heads.items()}
    assert all((label, r) in seen for label, _, _ in FS.SCENARIOS for r in range(4))


def test_the_last_fragment_has_no_closer_in_the_chunk():
    """The chunk ends after the last record: the fragment that record opens is not closed (state 0), the
    one before it is; cut one byte short, the last record is not usable and the one before it is open too."""
    data, _ = FS.stream(0)
    starts = _true_starts(data)
    T = FS.Tables(data, [])
    rows, _ = FS.host_rows(T)
    assert FS.as_tuples(rows[-2:]) == [(1, 1, 1, 0, starts[-1] - starts[-2]), (0, 0, 0, 0, 0)]
    T.n_bytes -= 1
    T.isize[-1] -= 1
    rows, _ = FS.host_rows(T)
    assert FS.as_tuples(rows) == FS.py_rows(T)
    assert FS.as_tuples(rows[-3:]) == [(1, 1, 1, 0, starts[-2] - starts[-3]), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)]


@pytest.mark.parametrize("seed", range(6))
def test_refused_block_in_the_middle(seed):
    """A block the device refused: no record that touches it is usable, whether or not its starts are
    listed, so no fragment is closed across it; the fragments wholly before and after it still are."""
    rng = np.random.default_rng(seed)
    data, _ = FS.stream(seed % 4)
    T = FS.Tables(data, FS.random_cuts(len(data), rng, 600, 1500))
    assert T.n_blocks >= 4
    j = int(rng.integers(1, T.n_blocks - 1))
    T.status[j] = 3
    if seed % 2:
        T.count[j] = 0                              # as the walk kernel leaves a refused block
    rows, first = FS.host_rows(T)
    want = FS.py_rows(T)
    assert FS.as_tuples(rows) == want
    lo, hi = int(T.ooff[j]), int(T.ooff[j]) + int(T.isize[j])
    for (b, k, at), row in zip(T.listed(), want):
        if row[0] and at < hi:
            assert at + row[4] <= lo, "a closed fragment and its closer's start lie before the refused block"
    assert any(r[0] for (b, _, _), r in zip(T.listed(), want) if b < j) or j == 1
    assert any(r[0] for (b, _, _), r in zip(T.listed(), want) if b > j)


@pytest.mark.parametrize("seed", range(8))
def test_lists_with_holes_and_false_starts(seed):
    """Starts dropped from the lists (a step reaches an offset that is not listed: nothing is claimed) and a
    start planted inside a record (it does not abut its predecessor, and its successor does not abut it)."""
    rng = np.random.default_rng(100 + seed)
    data, _ = FS.stream(seed % 4)
    T = FS.Tables(data, FS.random_cuts(len(data), rng))
    for _ in range(3):
        j = int(rng.integers(0, T.n_blocks))
        c = int(T.count[j])
        if c < 3:
            continue
        k = int(rng.integers(0, c))
        if seed % 2:                                # drop start k
            T.starts[j, k:c - 1] = T.starts[j, k + 1:c]
            T.count[j] = c - 1
        else:                                       # plant one 40 bytes into record k (ascending order kept)
            at = int(T.starts[j, k]) + 40
            if at + 4 > int(T.isize[j]) or (k + 1 < c and at >= int(T.starts[j, k + 1])):
                continue
            T.starts[j, k + 2:c + 1] = T.starts[j, k + 1:c]
            T.starts[j, k + 1] = at
            T.count[j] = c + 1
    rows, _ = FS.host_rows(T)
    assert FS.as_tuples(rows) == FS.py_rows(T)
    assert sum(r[0] for r in FS.as_tuples(rows)) > 5


def test_arguments():
    L = N.lib()
    data, _ = FS.stream(0)
    T = FS.Tables(data, [])
    assert L.fc2_bam_frag_host(T.data.ctypes.data, T.n_bytes, None, None, None, None, None, None, None, 0) == 0
    assert L.fc2_bam_frag_host(T.data.ctypes.data, T.n_bytes, None, T.isize.ctypes.data, None, T.starts.ctypes.data,
                               T.count.ctypes.data, None, None, 1) != 0
    big = np.zeros(N.BAM_DIGEST_MAX_BLOCKS + 2, np.uint32)
    rows = np.zeros(8, FS.FRAG)
    assert L.fc2_bam_frag_host(T.data.ctypes.data, T.n_bytes, big.ctypes.data, big.ctypes.data, None,
                               np.zeros(4, np.uint16).ctypes.data, big.ctypes.data, rows.ctypes.data, big.ctypes.data,
                               N.BAM_DIGEST_MAX_BLOCKS + 1) != 0
