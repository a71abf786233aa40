"""The -B writer's two GPU stages in their device mode, 1, on a device: what test_sam_encode_writer_host.py and
test_bam_out_pieces_host.py ask of the stand-in mode, 2, where a batch or a piece is computed inside the submit,
asked again where the uploads, the kernels and the downloads are in flight while the next slot fills.  At caps small
enough that every one of a stage's four slots is filled many times: the encode stage (fc2_ingest_set_bam_out_encode)
writes the default writer's file byte for byte, also with a refused line in the middle, and ends as the default
writer does on a line encode_sam fails on, batches still in flight; the BGZF stage (fc2_ingest_set_bam_out_device)
writes mode 0's header blocks, then the bytes fc2_gpu_bgzf_level / fc2_gpu_bgzf_tiles make of the same record
stream, then the EOF block; and both stages at once write the BGZF stage's file."""
import pytest

from bgzf_helpers import EOF_BLOCK, read_bam
from find_circ2_amd.ingest import NativeIngest
from sam_encode_helpers import E_IO
from samgen import sam_to_bam
from test_bam_out_pieces_host import write_bam as write_bam_pieces
from test_gpu_bgzf_tiles import gpu_bgzf_tiles
from test_sam_encode_writer_host import _tagged, records, rich, write_bam  # noqa: F401 (rich: the fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODE = 1                                         # the device itself
TIMEOUT_S = 20.0                                 # every wait for the device is bounded by it


def enc(**caps):
    return dict(mode=MODE, timeout_s=TIMEOUT_S, **caps)


def dev(block, piece_blocks, **tiles):
    return dict(mode=MODE, block=block, piece_blocks=piece_blocks, timeout_s=TIMEOUT_S, **tiles)


# ---- the encode stage ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 2, 63, 64, 65])
def test_encode_stage_writes_the_default_writers_file(rich, tmp_path, cap):
    _, sam, mode0 = rich
    out = str(tmp_path / "o.bam")
    (g, h), err = write_bam(sam, False, out, enc(max_lines=cap))
    assert err is None
    assert open(out, "rb").read() == open(mode0, "rb").read()
    n = len(records(mode0))
    assert n > 2000 and (g, h) == (-(-n // cap), 0) and g > 4          # every slot was filled again


def test_encode_stage_with_batches_cut_by_the_text_cap(rich, tmp_path):
    _, sam, mode0 = rich
    out = str(tmp_path / "o.bam")
    (g, h), err = write_bam(sam, False, out, enc(max_lines=64, max_text=1000))
    assert err is None and open(out, "rb").read() == open(mode0, "rb").read()
    assert g > len(records(mode0)) // 8 and h == 0                      # a few lines a batch


def test_an_f_tag_in_the_middle_goes_to_the_host_between_device_batches(rich, tmp_path):
    sam = _tagged(rich, tmp_path, b"XF:f:0.5")
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    assert write_bam(sam, False, a) == ((0, 0), None)
    assert any(b"XFf" in r for r in records(a))                         # (the line is one of those written)
    (g, h), err = write_bam(sam, False, b, enc(max_lines=64))
    assert err is None and h >= 1 and g > 4
    assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.parametrize("cap", [1, 64, 16384])
def test_a_rejected_line_ends_the_run_as_the_default_writer_does(rich, tmp_path, cap):
    """The stage dies in its collect with later batches submitted (caps 1 and 64); closing the ingest waits for
    them before their slots are freed."""
    sam = _tagged(rich, tmp_path, b"XQ:q:1")
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    _, err0 = write_bam(sam, False, a)
    assert err0 is not None and err0[0] == E_IO and err0[1] == "ValueError: bad SAM tag type"
    _, err = write_bam(sam, False, b, enc(max_lines=cap))              # (write_bam closes the ingest after the error)
    assert err == err0
    assert open(a, "rb").read() == open(b, "rb").read()                 # the records before the line, none after it
    assert 100 < len(records(a)) < len(records(rich[2]))


def test_bam_input_takes_the_encode_setter_and_does_nothing(rich, tmp_path):
    _, sam, _ = rich
    bam = str(tmp_path / "rich.bam")
    sam_to_bam(open(sam).read(), bam)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    assert write_bam(bam, True, a) == ((0, 0), None)
    assert write_bam(bam, True, b, enc(max_lines=64)) == ((0, 0), None)
    assert open(a, "rb").read() == open(b, "rb").read()


# ---- the BGZF stage --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def both_inputs(rich, tmp_path_factory):
    """The rich SAM and its BAM, and mode 0's spliced_alignments.bam of each."""
    d, sam, mode0 = rich
    bam = str(tmp_path_factory.mktemp("stages") / "rich.bam")
    sam_to_bam(open(sam).read(), bam)
    mode0_bam = bam[:-4] + "_mode0.bam"
    assert write_bam_pieces(bam, True, mode0_bam) == (0, 0)
    return {"sam": (sam, False, mode0), "bam": (bam, True, mode0_bam)}


@pytest.mark.parametrize("block,piece_blocks,tile,hist", [(256, 1, 0, 0), (256, 4, 0, 0), (0xff00, 1, 0, 0), (256, 1, 64, 256)])
@pytest.mark.parametrize("kind", ["sam", "bam"])
def test_bgzf_stage_writes_the_one_buffer_entrys_blocks(both_inputs, tmp_path, kind, block, piece_blocks, tile, hist):
    inp, is_bam, mode0 = both_inputs[kind]
    out = str(tmp_path / "o.bam")
    tiles = dict(tile=tile, hist=hist) if tile else {}
    pieces = write_bam_pieces(inp, is_bam, out, dev(block, piece_blocks, **tiles))
    blocks0, data0, rec0 = read_bam(mode0)
    blocks, data, rec = read_bam(out)
    assert data == data0 and rec == rec0 and len(data) - rec > 400000
    # the header in block(s) of its own, zlib's as in mode 0; then the records cut every `block` bytes; then EOF
    n_head = next(k for k in range(1, len(blocks0)) if sum(b[3] for b in blocks0[:k]) == rec0)
    assert blocks[:n_head] == blocks0[:n_head]
    n_rec = len(data) - rec
    assert [b[3] for b in blocks[n_head:]] == [block] * (n_rec // block) + ([n_rec % block] if n_rec % block else []) + [0]
    n_pieces = -(-n_rec // (block * piece_blocks))
    assert pieces == (n_pieces, 0)
    assert n_pieces > (8 if block == 256 else 4)                        # every slot was filled again
    # the record blocks: the bytes the one-buffer entry makes of the same stream (no EOF block of its own)
    if tile:
        rc, want, _ = gpu_bgzf_tiles(data[rec:], block, piece_blocks, tile, hist, 1)
    else:
        rc, want, _ = gpu_bgzf_tiles(data[rec:], block, piece_blocks, 0, 0, 1, entry="fc2_gpu_bgzf_level")
    assert rc == 0 and want and not want.endswith(EOF_BLOCK)
    blob = open(out, "rb").read()
    head_bytes = sum(b[0] for b in blocks[:n_head])
    assert blob[:head_bytes] == open(mode0, "rb").read()[:head_bytes]
    assert blob[head_bytes:len(blob) - len(EOF_BLOCK)] == want
    assert blob[len(blob) - len(EOF_BLOCK):] == EOF_BLOCK


# ---- both at once ----------------------------------------------------------------------------------------

def write_bam_both(sam, path, bam_encode, bam_device):
    """write_bam of a SAM input with both stages' counts: ((batches, host batches), (pieces, zlib pieces))."""
    ing = NativeIngest(sam, False)
    ing.set_bam_out(path, bam_device=bam_device, bam_encode=bam_encode)
    while not ing.eof:
        ing.next_chunk(15, False, False, 500)
    ing.close_bam_out()
    counts = ing.bam_encode_counts(), ing.bam_out_counts()
    ing.close()
    return counts


def test_both_stages_at_once_write_the_bgzf_stages_file(rich, tmp_path):
    _, sam, mode0 = rich
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    assert write_bam_both(sam, a, None, dev(256, 1))[0] == (0, 0)
    (g, h), (pieces, zlib_pieces) = write_bam_both(sam, b, enc(max_lines=64), dev(256, 1))
    assert open(a, "rb").read() == open(b, "rb").read()
    n = len(records(mode0))
    _, data, rec = read_bam(b)
    assert (g, h) == (-(-n // 64), 0) and g > 4
    assert (pieces, zlib_pieces) == (-(-(len(data) - rec) // 256), 0) and pieces > 8
    assert data == read_bam(mode0)[1]
