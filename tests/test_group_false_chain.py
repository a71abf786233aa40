"""A block's record list that begins at a false start leading onto the true chain, against the skip of
fc2_ingest_set_gpu_group (csrc/fc2_ingest.cpp sam_parse_loop): a record whose B array embeds a whole
well-formed record of another name, ending where the real record ends, with a BGZF block boundary inside
the real record.  The block's walk then lists the embedded record and the real record behind it; stepping
back from that record the device finds a mapped record of another name, and its row says the record opens
a fragment -- while on the true chain it is a further segment of the fragment before it.  The parse loop
compares the name with its own last mapped record before it steps over anything, so the counters stay
those of the feature off."""
import struct

import pytest

import frag_streams as FS
import group_inputs as G


def _rec_with_embedded(name, inner):
    """A mapped record whose last tag is XB:B:C holding `inner` (a whole record) as its bytes."""
    qn = name.encode() + b"\0"
    l_seq = 20
    tags = b"ASi" + struct.pack("<i", 20) + b"XBBC" + struct.pack("<i", len(inner)) + inner
    body = struct.pack("<iiBBHHHiiii", 0, 100, len(qn), 60, 4681, 1, 0, l_seq, -1, -1, 0) + qn + \
        struct.pack("<I", (l_seq << 4)) + bytes(0x12 for _ in range(10)) + bytes(30 for _ in range(l_seq)) + tags
    return struct.pack("<I", len(body)) + body


def _bam(records):
    text = b"@HD\tVN:1.5\n" + b"".join(b"@SQ\tSN:%s\tLN:90000\n" % n.encode() for n in G.NAMES)
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(G.NAMES))
    for n in G.NAMES:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", 90000)
    return head + b"".join(records), len(head)


@pytest.fixture(scope="module")
def trap(tmp_path_factory):
    """Fillers, then 40 times: a head P with an embedded record of another name, a supplementary H of P's
    name on another refID (a segment of P's fragment, never proper), two fillers; in BGZF blocks of the
    size that puts a block boundary inside the most P's, before the embedded record."""
    from samgen import bgzf_compress
    recs = [FS.rec("f%04d" % k, 0, k % 3) for k in range(150)]
    spans = []
    for k in range(40):
        inner = FS.rec("fake%02d" % k, 0, 2)
        p = _rec_with_embedded("trap%02d" % k + "x" * (k % 7), inner)
        at = sum(len(r) for r in recs)
        spans.append((at, at + len(p) - len(inner)))      # P's start, the embedded record's start
        recs += [p, FS.rec("trap%02d" % k + "x" * (k % 7), FS.SUPP, 1), FS.rec("g%04d" % k, 0, 0), FS.rec("h%04d" % k, 0, 1)]
    data, l_head = _bam(recs)
    def armed_at(block):
        return [k for k, (a, q) in enumerate(spans) if (a + l_head + 4) // block != (q + l_head) // block]
    block = max(range(400, 1200), key=lambda b: len(armed_at(b)))   # the block size that cuts the most P's
    d = tmp_path_factory.mktemp("false_chain")
    path = str(d / "trap.bam")
    open(path, "wb").write(bgzf_compress(data, block=block, level=1))
    return path, data[l_head:], l_head, spans, armed_at(block), block


def test_the_rows_do_claim_the_segment(trap):
    """The tables of the blocks around an armed trap: the embedded record is listed, and the real record
    behind it gets state 1 from fc2_bam_frag_host -- the rule as stated, on a false chain."""
    _, stream, l_head, spans, armed, block = trap
    assert len(armed) > 10
    claimed = 0
    for k in armed:
        a, q = spans[k]
        cut = ((q + l_head) // block) * block - l_head      # the block boundary inside P, as a stream offset
        assert a < cut <= q
        lo = a - 2 * len(FS.rec("f0000", 0, 0))           # two whole records before P
        hi = q + 600
        T = FS.Tables(stream[lo:hi], [cut - lo])
        rows = FS.as_tuples(FS.host_rows(T)[0])
        at = [x for _, _, x in T.listed()]
        h = q - lo + len(FS.rec("fake00", 0, 2))          # H: right behind the embedded record, P's end
        if (q - lo) in at and h in at:
            claimed += rows[at.index(h)][0]
    assert claimed > 5, "the trap is armed: rows say H opens a fragment"


@pytest.mark.parametrize("batch,block", [("4", "3000"), ("8", "1500")])
def test_the_parse_loop_does_not_follow_them(trap, monkeypatch, batch, block):
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    monkeypatch.setenv("FC2_PARSE_BLOCK", block)
    path = trap[0]
    ref, _, _ = G.caller_run(path)
    got, _, grp = G.caller_run(path, group=2)
    assert got == ref, (got[3], ref[3])
    assert ref[3][0] == 150 + 40 * 3 and grp[0] > 50, (ref[3], grp)
