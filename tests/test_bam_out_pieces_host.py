"""spliced_alignments.bam's device mode (fc2_ingest_set_bam_out_device) through the host model of the device,
mode 2: every piece's tiles raw-deflated by zlib level 1 and framed by fc2_bgzf_frame_host, the slots, their
rotation, the order of the writes and the close exactly the device mode's code.  The inflated record stream is
mode 0's, the blocks are cut where mode 0 cuts them, the header block is zlib's, the EOF block is last, the
project's reader takes the file; mode 0 still writes the bytes it wrote before the device mode existed
(SHA-256 pinned from that tree)."""
import ctypes
import hashlib

import pytest

from bgzf_helpers import E_PARAM, EOF_BLOCK, read_bam
from find_circ2_amd import _native as N
from find_circ2_amd.ingest import NativeIngest
from samgen import sam_to_bam
from test_native_caller import _rich_sam

# spliced_alignments.bam of the rich input (1500 fragments, seed 31) in mode 0, written by the tree before
# the device mode was added: from the SAM, and from its BAM
PARENT_SHA256 = {"sam": "25f1f49982956e416a3e8477078b5a464bda4e7dd5714056cbe7b818b71848d5",
                 "bam": "6138ec79441200665faa8056e6f2cb13a9feeaf2575050792e9de8bf5e76db9c"}


def write_bam(inp, is_bam, path, bam_device=None, noop=False):
    """The anchors of inp to path; (pieces from the device or its model, pieces zlib compressed)."""
    ing = NativeIngest(inp, is_bam)
    ing.set_bam_out(path, bam_device=bam_device)
    while not ing.eof:
        ing.next_chunk(15, False, noop, 500)
    ing.close_bam_out()
    counts = ing.bam_out_counts()
    ing.close()
    return counts


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("bampieces")
    sam = str(d / "rich.sam")
    _rich_sam(sam, 1500, seed=31)
    bam = str(d / "rich.bam")
    sam_to_bam(open(sam).read(), bam)
    inputs = {"sam": (sam, False), "bam": (bam, True)}
    mode0 = {}
    for kind, (inp, is_bam) in inputs.items():
        mode0[kind] = str(d / ("mode0_%s.bam" % kind))
        assert write_bam(inp, is_bam, mode0[kind]) == (0, 0)
    return inputs, mode0


@pytest.mark.parametrize("kind", ["sam", "bam"])
def test_mode_0_writes_the_parents_bytes(rich, kind):
    _, mode0 = rich
    assert hashlib.sha256(open(mode0[kind], "rb").read()).hexdigest() == PARENT_SHA256[kind]


@pytest.mark.parametrize("piece_blocks", [1, 4])
@pytest.mark.parametrize("block", [256, 0xff00])
@pytest.mark.parametrize("kind", ["sam", "bam"])
def test_host_model_pieces(rich, tmp_path, kind, block, piece_blocks):
    inputs, mode0 = rich
    inp, is_bam = inputs[kind]
    out = str(tmp_path / "o.bam")
    pieces = write_bam(inp, is_bam, out, dict(mode=2, block=block, piece_blocks=piece_blocks))
    blocks0, data0, rec0 = read_bam(mode0[kind])
    blocks, data, rec = read_bam(out)
    assert data == data0 and rec == rec0 and len(data) - rec > 400000
    # the header in block(s) of its own, zlib's as in mode 0; then the records cut every `block` bytes
    n_head = next(k for k in range(1, len(blocks0)) if sum(b[3] for b in blocks0[:k]) == rec0)
    assert blocks[:n_head] == blocks0[:n_head]
    n_rec = len(data) - rec
    want = [block] * (n_rec // block) + ([n_rec % block] if n_rec % block else [])
    assert [b[3] for b in blocks[n_head:]] == want + [0]
    if block == 0xff00:
        assert [b[3] for b in blocks] == [b[3] for b in blocks0]
    assert open(out, "rb").read().endswith(EOF_BLOCK) and blocks[-1][0] == 28
    n_pieces = -(-n_rec // (block * piece_blocks))
    assert pieces == (n_pieces, 0)
    if block == 256:
        assert n_pieces > 8                      # the four slots were used more than twice each
    elif piece_blocks == 1:
        assert n_pieces > 4                      # ... at least one of them twice
    # the project's own reader takes the file
    ing = NativeIngest(out, True)
    while not ing.eof:
        ing.next_chunk(15, False, False, 500)
    n_reads = ing.counts.n_reads
    ing.close()
    ing0 = NativeIngest(mode0[kind], True)
    while not ing0.eof:
        ing0.next_chunk(15, False, False, 500)
    assert n_reads == ing0.counts.n_reads > 500
    ing0.close()


def test_host_model_noop_writes_header_and_eof_only(rich, tmp_path):
    inputs, _ = rich
    out, out0 = str(tmp_path / "noop.bam"), str(tmp_path / "noop0.bam")
    assert write_bam(*inputs["sam"], out, dict(mode=2, block=256, piece_blocks=1), noop=True) == (0, 0)
    write_bam(*inputs["sam"], out0, noop=True)
    assert open(out, "rb").read() == open(out0, "rb").read()
    blocks, data, rec = read_bam(out)
    assert rec == len(data) and blocks[-1][3] == 0


def test_mode_0_through_the_setter_changes_nothing(rich, tmp_path):
    inputs, mode0 = rich
    out = str(tmp_path / "o.bam")
    assert write_bam(*inputs["sam"], out, dict(mode=0, block=256, piece_blocks=1)) == (0, 0)
    assert open(out, "rb").read() == open(mode0["sam"], "rb").read()


def test_setter_arguments(rich, tmp_path):
    inputs, _ = rich
    L = N.lib()
    ing = NativeIngest(*inputs["sam"])
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == E_PARAM       # before fc2_ingest_set_bam_out
    ing.set_bam_out(str(tmp_path / "a.bam"))
    for args in [(3, 0, 0, 0, 0.0), (-1, 0, 0, 0, 0.0), (2, 0, 0xff01, 0, 0.0), (2, 0, 0, 1025, 0.0), (2, 0, 0, 0, -1.0),
                 (1, -1, 0, 0, 0.0)]:
        assert L.fc2_ingest_set_bam_out_device(ing.h, *args) == E_PARAM, args
    assert L.fc2_ingest_set_bam_out_device(None, 2, 0, 0, 0, 0.0) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == E_PARAM       # once
    ing.next_chunk(15, False, False, 50)
    g, c = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.fc2_ingest_bam_out_counts(ing.h, ctypes.byref(g), ctypes.byref(c)) == 0 and (g.value, c.value) == (0, 0)
    assert L.fc2_ingest_bam_out_counts(None, ctypes.byref(g), ctypes.byref(c)) == E_PARAM
    ing.close_bam_out()
    assert ing.bam_out_counts() == (1, 0)
    ing.close()
    # after the first record the setter is refused
    ing = NativeIngest(*inputs["sam"])
    ing.set_bam_out(str(tmp_path / "b.bam"))
    ing.next_chunk(15, False, False, 50)
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == E_PARAM
    ing.close()
