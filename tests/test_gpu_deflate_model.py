"""The GPU DEFLATE compressor (deflate_kernel, csrc/fc2_deflate.hip) against its host model
(deflate_model.py, itself checked in test_deflate_model.py): the same out_len, the same bytes and the
same CRC, on the contents x lengths grid and on the inputs that reach the compressor's rare branches
(the Huffman length limit, dummy distance symbols, split runs of code lengths, tokens over three
staging words); at every destination alignment with a stream long enough to be flushed in pieces; at
unaligned sources; and in the stored forms.  A builder that fails into the stored form writes a valid
stream too: the overflow inputs must come out as a dynamic block with the longest codeword at the limit.
"""
import pytest

from deflate_helpers import CONTENTS, check_streams, deflate_blocks, deflate_launch, explain, tile_bound
from deflate_model import crc32, model
from test_deflate_model import GRID_LENGTHS, NAMED, grid, named

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _equal(streams, cr, tiles, wants):
    """out_len, the bytes and the CRC of each tile are the model's (wants: the model's streams)."""
    for i, (s, t, w) in enumerate(zip(streams, tiles, wants)):
        assert len(s) == len(w) and s == w, "tile %d (%d bytes): %s" % (i, len(t), explain(s, w))
        assert int(cr[i]) == crc32(t), i


def _launch(data, tile, **kw):
    d, ln, cr, stride = deflate_launch(data, tile, **kw)
    return check_streams(data, tile, d, ln, cr, stride), cr


@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_kernel_equals_model_on_the_grid(content):
    for n in GRID_LENGTHS:
        data, want, info = grid(content, n)
        streams, cr = _launch(data, 65536 if n > 32768 else 32768)
        _equal(streams, cr, [data], [want])


@pytest.mark.parametrize("name", sorted(NAMED))
def test_kernel_equals_model_on_the_named_inputs(name):
    data, want, info = named(name)
    streams, cr = _launch(data, 65536)
    _equal(streams, cr, [data], [want])


@pytest.mark.parametrize("name,code,limit", [("ll_overflow_1.7", 1, 15), ("ll_overflow_2.0", 1, 15), ("cl_overflow", 3, 7),
                                             ("three_word", 3, 7)])
def test_overflow_inputs_give_a_dynamic_block(name, code, limit):
    """By the kernel's own stream alone: not stored, and the longest codeword is at the limit."""
    data, want, info = named(name)
    assert info["clipped"][0 if code == 1 else 2] > 0
    streams, cr = _launch(data, 65536)
    assert streams[0][0] & 7 == 1 | (2 << 1)     # BFINAL, BTYPE 2
    tokens, size, blocks = deflate_blocks(streams[0])
    assert size == len(data) and [b[0] for b in blocks] == ["dynamic"]
    assert max(blocks[0][code]) == limit


def test_every_destination_alignment_with_flushes():
    tile = 32768
    one, want, info = named("flushes")
    assert info["flushes"] >= 3
    data, stride = one * 17, tile_bound(tile) + 1
    off = 16 - stride % 16                       # (a guard slot lies before the first tile's)
    assert [(off + (k + 1) * stride) % 16 for k in range(17)] == list(range(16)) + [0]
    d, ln, cr, stride = deflate_launch(data, tile, stride, dst_offset=off)
    streams = check_streams(data, tile, d, ln, cr, stride)
    _equal(streams, cr, [one] * 17, [want] * 17)


@pytest.mark.parametrize("a", [0, 1, 7, 15])
def test_overflow_tile_at_destination_alignment(a):
    tile = 65536
    data, want, info = named("ll_overflow_2.0")
    assert info["clipped"][0] > 0 and model(data, a=a)[1]["flushes"] >= 3
    d, ln, cr, stride = deflate_launch(data, tile, dst_offset=a)     # (the bound, 65552, is a multiple of 16)
    assert (stride + a) % 16 == a
    streams = check_streams(data, tile, d, ln, cr, stride)
    _equal(streams, cr, [data], [want])


@pytest.mark.parametrize("a", [0, 1, 2, 3])
def test_three_word_tokens_at_destination_alignment(a):
    data, want, info = named("three_word")
    assert model(data, a=a)[1]["three_word"] > 0
    d, ln, cr, stride = deflate_launch(data, 32768, dst_offset=a)
    assert (stride + a) % 16 == a
    streams = check_streams(data, 32768, d, ln, cr, stride)
    _equal(streams, cr, [data], [want])


def test_source_alignment():
    tile = 32768
    data, want, info = named("flushes")
    for off in (0, 1, 3, 15):
        d, ln, cr, stride = deflate_launch(data, tile, src_offset=off)
        streams = check_streams(data, tile, d, ln, cr, stride)
        _equal(streams, cr, [data], [want])
    # two tiles of 32767: the second starts unaligned, and its last group of 16 bytes is partial
    data = CONTENTS["fastq"](2 * 32767)
    tiles = [data[:32767], data[32767:]]
    streams, cr = _launch(data, 32767)
    _equal(streams, cr, tiles, [model(t)[0] for t in tiles])


@pytest.mark.parametrize("n", [65535, 65536])
def test_stored_forms_at_alignment_5(n):
    data = CONTENTS["random"](n)
    want, info = model(data, a=5)
    assert info["kind"] == "stored" and len(want) == n + (5 if n == 65535 else 10)
    d, ln, cr, stride = deflate_launch(data, 65536, dst_offset=5)
    assert (stride + 5) % 16 == 5
    streams = check_streams(data, 65536, d, ln, cr, stride)
    _equal(streams, cr, [data], [want])
    assert [t for t in deflate_blocks(streams[0])[0]] == ([("stored", 65535)] + ([("stored", 1)] if n == 65536 else []))
