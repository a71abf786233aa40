"""The fragment rows made on the GPU (fc2_bam_frag_launch, csrc/fc2_inflate.hip bam_frag_kernel, over the
digest rows fc2_bam_digest_launch made just before on the same stream) against the CPU's
(fc2_bam_frag_host), row for row: the hand-built streams of frag_streams.py at all four residues, uncut
and in blocks of 1-4 kB; a seeded fuzz of a real record stream in blocks of 1-4 kB, a third of its
records damaged; refused blocks; launches of 1, 2, 255 and 1024 blocks.  Every launch has guard bytes around the
stream and guard rows around frag_rows: the input is unchanged and nothing but the counted rows written."""
import ctypes
import struct

import numpy as np
import pytest

import frag_streams as FS
from find_circ2_amd import _native as N

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def frag_launch(T, shift=0):
    """fc2_bam_digest_launch then fc2_bam_frag_launch over the tables, the stream `shift` bytes past an
    aligned address: the counted fragment rows as (state, n_records, n_mates, n_unmapped, bytes) tuples."""
    dev = torch.device("cuda:0")
    n = T.n_blocks
    lead = GUARD + shift
    host = np.random.default_rng(n).integers(0, 256, lead + len(T.data) + GUARD, dtype=np.uint8)
    host[lead:lead + len(T.data)] = T.data
    total = int(T.first()[-1])
    d_bytes = torch.tensor(host, device=dev)
    as_i32 = lambda a: torch.tensor(np.ascontiguousarray(a).view(np.int32), device=dev)  # noqa: E731
    d_ooff, d_isize, d_count, d_status = as_i32(T.ooff), as_i32(T.isize), as_i32(T.count), as_i32(T.status)
    table = T.starts.copy()
    for j in range(n):
        table[j, min(int(T.count[j]), FS.CAP):] = 0xFFFF          # (unlisted entries: offsets never to be read)
    d_starts = torch.tensor(table.view(np.int16), device=dev)
    d_rows = torch.zeros((total + 1) * 32, dtype=torch.uint8, device=dev)
    d_first = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    d_frags = torch.full(((total + 2 * GUARD) * 8,), FILL, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = N.lib()
    N.check(L.fc2_bam_digest_launch(d_bytes.data_ptr() + lead, T.n_bytes, d_ooff.data_ptr(), d_isize.data_ptr(),
                                    d_status.data_ptr(), d_starts.data_ptr(), d_count.data_ptr(), d_rows.data_ptr(),
                                    d_first.data_ptr(), n, stream))
    N.check(L.fc2_bam_frag_launch(d_bytes.data_ptr() + lead, T.n_bytes, d_ooff.data_ptr(), d_isize.data_ptr(),
                                  d_status.data_ptr(), d_starts.data_ptr(), d_count.data_ptr(), d_rows.data_ptr(),
                                  d_first.data_ptr(), d_frags.data_ptr() + GUARD * 8, n, stream))
    torch.cuda.synchronize(dev)
    assert (d_bytes.cpu().numpy() == host).all(), "the stream was written"
    frags = d_frags.cpu().numpy()
    assert (frags[:GUARD * 8] == FILL).all() and (frags[(GUARD + total) * 8:] == FILL).all(), "a guard row was written"
    assert (d_first.cpu().numpy().view(np.uint32) == T.first()).all()
    return FS.as_tuples(frags[GUARD * 8:(GUARD + total) * 8].view(FS.FRAG))


def _same(T, shift=0):
    want = FS.as_tuples(FS.host_rows(T)[0])
    got = frag_launch(T, shift)
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:5], [(got[k], want[k]) for k in bad[:5]])
    return want


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_hand_built_streams(shift):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    data, heads = FS.stream(shift)
    for cuts in ([], FS.random_cuts(len(data), np.random.default_rng(10 + shift)), FS.random_cuts(len(data), np.random.default_rng(shift), 90, 400)):
        T = FS.Tables(data, cuts)
        want = _same(T, shift=(shift + 1) % 4)
        if not cuts:                                # the rows written beside the scenarios
            got = dict(zip((at for _, _, at in T.listed()), want))
            for label, _, exp in FS.SCENARIOS:
                assert got[heads[label]][:4] == (exp or (0, 0, 0, 0)), label
    # the chunk ends inside the last record
    T = FS.Tables(data, FS.random_cuts(len(data), np.random.default_rng(3)))
    T.n_bytes -= 1
    T.isize[-1] -= 1
    assert _same(T)[-2:] == [(0, 0, 0, 0, 0)] * 2


def _damage(data, starts, rng):
    """A third of the whole records at `starts` made invalid for the parser by one byte that matters -- a tag's
    type, l_read_name (the name is then not NUL-terminated), now and then block_size (the record's end
    moves, and the block's list with it) -- and a seventh of the others changed in what the rule reads and
    the parser accepts: flag & 0x40 / 0x10 / 4, refID, the name's last byte.  Returns (invalidated, altered)."""
    bad = alt = 0
    for o in starts:
        bs, ref, _, l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, o)
        if o + 4 + bs > len(data):
            continue
        r = rng.random()
        if r < 1 / 3:
            t = o + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
            kind = rng.random()
            if kind < 0.1:
                struct.pack_into("<i", data, o, bs - int(rng.integers(1, 4)))
            elif kind < 0.6 and t + 3 <= o + 4 + bs:
                data[t + 2] = ord("?")
            else:
                data[o + 12] = l_name - 1 if l_name > 2 else l_name + 1
            bad += 1
        elif r < 1 / 3 + 1 / 7:
            kind = int(rng.integers(0, 5))
            if kind < 3:
                struct.pack_into("<H", data, o + 18, flag ^ (0x40, 0x10, 0x4)[kind])
            elif kind == 3:
                struct.pack_into("<i", data, o + 4, (ref + 1) % 3)
            elif l_name > 1:
                data[o + 36 + l_name - 2] = ord("#")
            alt += 1
    return bad, alt


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    """~400 consecutive blocks of 1-4 kB of the record stream of a BAM shaped like the steady-state
    generator's (group_inputs.group_sam, paired), from a record start on, a third of its records damaged
    (_damage); the lists are fc2_bam_walk_host's of each block.  With the share of the listed starts whose
    digest says the host parser would not accept them."""
    import group_inputs as G
    from samgen import sam_to_bam
    from test_bam_digest_host import host_digest
    tmp = tmp_path_factory.mktemp("frag_fuzz")
    sam, raw = str(tmp / "g.sam"), str(tmp / "raw.bam")
    G.group_sam(sam, 3500, 5, True)
    sam_to_bam(open(sam).read(), raw, compress="none")
    whole = open(raw, "rb").read()
    o = 12 + struct.unpack_from("<i", whole, 4)[0]
    for _ in range(struct.unpack_from("<i", whole, o - 4)[0]):
        o += 8 + struct.unpack_from("<i", whole, o)[0]
    recs = []
    while o < len(whole):
        recs.append(o)
        o += 4 + struct.unpack_from("<i", whole, o)[0]
    rng = np.random.default_rng(77)
    sizes = [int(rng.integers(1000, 4001)) for _ in range(400)]
    a = recs[int(rng.integers(0, len(recs) // 4))]
    assert a + sum(sizes) < len(whole)
    data = bytearray(whole[a:a + sum(sizes)])
    n_bad, n_alt = _damage(data, [r - a for r in recs if a <= r < a + len(data) - 36], rng)
    T = FS.Tables(bytes(data), list(np.cumsum(sizes)[:-1]))
    listed = T.listed()
    invalid = sum(1 for _, _, at in listed if host_digest(T.data, T.n_bytes, at)[0] != 1)
    return T, invalid / len(listed), n_bad, n_alt


def test_fuzz_equals_the_host_rows(fuzz):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    T, invalid_share, n_bad, n_alt = fuzz
    want = _same(T, shift=3)
    closed = [w for w in want if w[0]]
    # a third of the records were made invalid, and more than a quarter of the starts the blocks' walks
    # still list are: the walks run into invalid records inside fragments, as closers and on the way back;
    # a few hundred fragments are closed all the same
    assert n_bad > 1500 and n_alt > 400 and invalid_share > 0.25, (n_bad, n_alt, invalid_share)
    assert len(closed) > 200 and len(want) > 3000, (len(closed), len(want))
    assert any(w[2] == 2 for w in closed) and any(w[3] for w in closed) and any(w[1] > 2 for w in closed)
    ends = np.concatenate([T.ooff[1:], [T.n_bytes]])
    across = sum(1 for (j, _, at), w in zip(T.listed(), want) if w[0] and at + w[4] >= ends[j])
    assert across > 20, "fragments whose closer lies in a later block"


def test_refused_blocks(fuzz):
    """Random blocks with status != 0 (their counts as the walk left them for some, 0 as the walk kernel
    leaves a refused block for others): no fragment is closed over a byte of one."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import copy
    T = copy.deepcopy(fuzz[0])
    rng = np.random.default_rng(5)
    for j in range(T.n_blocks):
        if rng.random() < 0.2:
            T.status[j] = int(rng.integers(1, 17))
            if rng.random() < 0.5:
                T.count[j] = 0
    T.status[0], T.status[1], T.status[-1] = 7, 0, 16
    want = _same(T)
    lo = T.ooff.astype(np.int64)
    hi = lo + T.isize
    refused = [(int(lo[j]), int(hi[j])) for j in range(T.n_blocks) if T.status[j]]
    n = 0
    for (_, _, at), w in zip(T.listed(), want):
        if w[0]:
            n += 1
            assert not any(a < at + w[4] + 36 and at < b for a, b in refused), (at, w)
    assert n > 200


@pytest.mark.parametrize("n_blocks", [1, 2, 255, 1024])
def test_launch_sizes(n_blocks):
    """Blocks of 250 bytes (two or three short records each) at every launch size, the largest
    included: fragments of one to three records, a pair here and there, each crossing blocks."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(n_blocks)
    data, k = bytearray(), 0
    while len(data) < 250 * n_blocks + 200:
        r = rng.random()
        name = "q%d" % k
        k += 1
        if r < 0.5:
            data += FS.rec(name, 0, int(rng.integers(3)))
        elif r < 0.8:
            data += FS.rec(name, FS.R1, 0) + FS.rec(name, FS.R2 | (FS.REV if r < 0.65 else 0), 1)
        else:
            data += FS.rec(name, 0, 1) + FS.rec(name, FS.SUPP, int(rng.integers(1, 3))) + FS.rec("x", FS.UNMAPPED, -1)
    data = bytes(data[:250 * n_blocks])                     # (the last record may be cut)
    T = FS.Tables(data, list(range(250, 250 * n_blocks, 250)))
    want = _same(T)
    assert n_blocks < 255 or sum(w[0] for w in want) > n_blocks / 4


def test_arguments():
    p = ctypes.c_void_p(64)
    L = N.lib()
    assert L.fc2_bam_frag_launch(p, 4, p, p, None, p, p, p, p, p, N.BAM_DIGEST_MAX_BLOCKS + 1, None) == N.FC2_E_PARAM
    assert L.fc2_bam_frag_launch(p, 4, p, p, None, p, p, p, p, None, 1, None) == N.FC2_E_PARAM
    assert L.fc2_bam_frag_launch(p, 4, p, p, None, p, p, p, p, ctypes.c_void_p(68), 1, None) == N.FC2_E_PARAM
    assert L.fc2_bam_frag_launch(None, 0, None, None, None, None, None, None, None, None, 0, None) == 0
