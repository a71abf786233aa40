"""spliced_alignments.bam's device mode with tiles inside a block (fc2_ingest_set_bam_out_device_tiles) through the
host model of the device, mode 2: every block one raw stream from zlib, flushed at the tiles' ends, its tiles in
slots of their own and framed by fc2_bgzf_frame_groups_host, the slots' rotation and the close the device mode's
code.  With tiles of 16320 bytes and 32 KiB of history the inflated file and the ISIZE sequence are mode 0's at
blocks of 0xff00 bytes (and the same stream in blocks of 4096), the pieces are counted, every block's CRC-32 --
combined from its tiles' -- is right; the setter is refused after the device mode is set and after the first
record, and so is what cannot be tiles; on the command line FC2_GPU_BAM_TILE / FC2_GPU_BAM_HISTORY without
FC2_GPU_BAM=1 change no byte of any output."""
import gzip
import zlib

import pytest

from bgzf_helpers import E_PARAM, EOF_BLOCK, read_bam
from find_circ2_amd import _native as N
from find_circ2_amd.ingest import NativeIngest
from samgen import sam_to_bam
from test_bam_out_pieces_host import write_bam
from test_deflate_level_abi import _cli
from test_native_caller import _rich_sam

TILE, HIST = 16320, 32768


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("bamtiles")
    sam = str(d / "rich.sam")
    fa = _rich_sam(sam, 1500, seed=31)
    bam = str(d / "rich.bam")
    sam_to_bam(open(sam).read(), bam)
    inputs = {"sam": (sam, False), "bam": (bam, True)}
    mode0 = {}
    for kind, (inp, is_bam) in inputs.items():
        mode0[kind] = str(d / ("mode0_%s.bam" % kind))
        assert write_bam(inp, is_bam, mode0[kind]) == (0, 0)
    return inputs, mode0, fa


@pytest.mark.parametrize("piece_blocks", [1, 3])
@pytest.mark.parametrize("block,tile", [(0xff00, TILE), (4096, 1024), (4096, 1000)])
@pytest.mark.parametrize("kind", ["sam", "bam"])
def test_host_model_with_tiles(rich, tmp_path, kind, block, tile, piece_blocks):
    inputs, mode0, _ = rich
    inp, is_bam = inputs[kind]
    out = str(tmp_path / "o.bam")
    pieces = write_bam(inp, is_bam, out, dict(mode=2, block=block, piece_blocks=piece_blocks, tile=tile, hist=HIST))
    blocks0, data0, rec0 = read_bam(mode0[kind])
    blocks, data, rec = read_bam(out)
    assert data == data0 and rec == rec0 and len(data) - rec > 400000
    n_head = next(k for k in range(1, len(blocks0)) if sum(b[3] for b in blocks0[:k]) == rec0)
    assert blocks[:n_head] == blocks0[:n_head]
    n_rec = len(data) - rec
    want = [block] * (n_rec // block) + ([n_rec % block] if n_rec % block else [])
    assert [b[3] for b in blocks[n_head:]] == want + [0]
    if block == 0xff00:
        assert [b[3] for b in blocks] == [b[3] for b in blocks0]     # the ISIZE sequence is mode 0's
    assert open(out, "rb").read().endswith(EOF_BLOCK)
    assert pieces == (-(-n_rec // (block * piece_blocks)), 0) and pieces[0] > (4 if piece_blocks == 1 else 1)
    # every block: one raw stream that ends with the block, its combined CRC-32 zlib's of the block's bytes
    at = rec
    for bsize, payload, crc, isize in blocks[n_head:-1]:
        z = zlib.decompressobj(-15)
        assert z.decompress(payload) == data[at:at + isize] and z.eof and z.unused_data == b"" and bsize <= 65536
        assert crc == zlib.crc32(data[at:at + isize])
        at += isize
    assert at == len(data)
    # the tiles are there: a sync flush's empty stored block ends every tile but the block's last
    tiles_per_block = -(-block // tile)
    assert blocks[n_head][1].count(b"\x00\x00\xff\xff") >= tiles_per_block - 1
    # and the file differs from the one without tiles only in the payloads
    plain = str(tmp_path / "plain.bam")
    assert write_bam(inp, is_bam, plain, dict(mode=2, block=block, piece_blocks=piece_blocks)) == pieces
    assert gzip.decompress(open(plain, "rb").read()) == data and open(plain, "rb").read() != open(out, "rb").read()


def test_a_tile_that_holds_the_block_is_the_writer_without_tiles(rich, tmp_path):
    inputs, _, _ = rich
    a, b, c = (str(tmp_path / n) for n in ("a.bam", "b.bam", "c.bam"))
    assert write_bam(*inputs["sam"], a, dict(mode=2, piece_blocks=2)) == \
        write_bam(*inputs["sam"], b, dict(mode=2, piece_blocks=2, tile=0xff00, hist=HIST)) == \
        write_bam(*inputs["sam"], c, dict(mode=2, piece_blocks=2, tile=0, hist=HIST))
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def test_tiles_setter_arguments(rich, tmp_path):
    inputs, _, _ = rich
    sam = inputs["sam"][0]
    L = N.lib()
    ing = NativeIngest(sam, False)
    assert L.fc2_ingest_set_bam_out_device_tiles(None, TILE, HIST) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device_tiles(ing.h, TILE, HIST) == E_PARAM      # before fc2_ingest_set_bam_out
    ing.set_bam_out(str(tmp_path / "a.bam"))
    assert L.fc2_ingest_set_bam_out_device_tiles(ing.h, TILE, 32769) == E_PARAM      # the history
    # what fc2_ingest_set_bam_out_device itself refuses: 17 tiles a block, tile + hist over 65536
    assert L.fc2_ingest_set_bam_out_device_tiles(ing.h, 0xff00 // 17, 0) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device_tiles(ing.h, 40000, 32768) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 4096, 0, 0.0) == 0          # (a tile that holds the block: no tiles)
    ing.close()
    ing = NativeIngest(sam, False)
    ing.set_bam_out(str(tmp_path / "b.bam"))
    for args in [(TILE, HIST), (0xff00 // 16, 0), (0, 0)]:
        assert L.fc2_ingest_set_bam_out_device_tiles(ing.h, *args) == 0
    assert L.fc2_ingest_set_bam_out_device_tiles(ing.h, TILE, HIST) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == 0
    assert L.fc2_ingest_set_bam_out_device_tiles(ing.h, TILE, HIST) == E_PARAM      # after the device mode is set
    ing.close()
    ing = NativeIngest(sam, False)
    ing.set_bam_out(str(tmp_path / "c.bam"))
    ing.next_chunk(15, False, False, 50)
    assert L.fc2_ingest_set_bam_out_device_tiles(ing.h, TILE, HIST) == E_PARAM      # after the first record
    ing.close()


def test_cli_tiles_alone_change_nothing(rich, tmp_path):
    inputs, _, fa = rich
    sam = inputs["sam"][0]
    files0, keys0 = _cli(fa, sam, str(tmp_path / "unset"), {"FC2_GPU_BAM_TILE": "", "FC2_GPU_BAM_HISTORY": ""})
    files1, keys1 = _cli(fa, sam, str(tmp_path / "tiles"), {"FC2_GPU_BAM_TILE": str(TILE), "FC2_GPU_BAM_HISTORY": str(HIST)})
    assert len(files0["spliced_alignments.bam"]) > 100000
    assert files1 == files0
    assert keys1 == keys0 and not [k for k in keys0 if k.startswith("bam_gpu")]


def test_run_log_note():
    from find_circ2_amd.cli import _bam_tiles_note
    assert _bam_tiles_note(None) == "" and _bam_tiles_note(dict(mode=1)) == ""
    assert _bam_tiles_note(dict(tile=0, hist=HIST)) == "" == _bam_tiles_note(dict(tile=0xff00, hist=HIST))
    assert _bam_tiles_note(dict(tile=TILE, hist=0)) == ", bam_gpu_tile=16320"
    assert _bam_tiles_note(dict(tile=TILE, hist=HIST)) == ", bam_gpu_tile=16320, bam_gpu_history=32768"
