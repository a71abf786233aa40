"""The GPU DEFLATE compressor (fc2_deflate_launch, csrc/fc2_deflate.hip) against zlib: every tile's
stream, inflated alone, gives the tile's bytes and ends where out_len says; the CRC-32 is zlib's;
nothing outside a tile's own bytes of its slot is written; the project's GPU inflater reads the
streams back; two launches give the same bytes, and they are the host model's (deflate_model.py) for
inputs up to 70 KB.  Sizes show that both halves are real: repeats are
found (a periodic text shrinks far below what Huffman codes alone reach), Huffman codes are built
(random ACGT shrinks below what fixed codes reach), and what does not shrink is stored."""
import zlib

import numpy as np
import pytest

from deflate_helpers import CONTENTS, E_PARAM, check_streams, deflate_launch, fastq_text, tile_bound
from deflate_model import model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILE = 32768
LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]


def _rng():
    return np.random.default_rng(2024)


def _run(data, tile, stride=None):
    """One input through the kernel, checked; returns (streams, out_len, crc)."""
    d, ln, cr, stride = deflate_launch(data, tile, stride)
    streams = check_streams(data, tile, d, ln, cr, stride)
    d2, ln2, cr2, _ = deflate_launch(data, tile, stride)       # the same bytes on every run
    assert np.array_equal(d, d2) and np.array_equal(ln, ln2) and np.array_equal(cr, cr2)
    if len(data) <= 70 * 1024:                                 # the same bytes as the host model's
        for i, s in enumerate(streams):
            want, info = model(data[i * tile:(i + 1) * tile])
            assert s == want, "tile %d: not the model's %s stream (%d bytes against %d)" % (i, info["kind"], len(s), len(want))
    return streams, ln, cr


def _round_trip(data, tile, streams, cr):
    """The streams through the project's GPU inflater, with their CRCs."""
    from gpu_helpers import inflate_run
    tiles = [data[i * tile:(i + 1) * tile] for i in range(len(streams))]
    got, st = inflate_run(streams, [len(t) for t in tiles], [int(c) for c in cr])
    assert [int(x) for x in st] == [0] * len(tiles)
    assert got == tiles


@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_deflate_every_length(content):
    blobs = []
    for n in LENGTHS:
        data = CONTENTS[content](n)
        assert len(data) == n
        streams, ln, cr = _run(data, TILE)
        blobs.append((data, streams, cr))
    # one inflate launch for all the lengths' tiles
    from gpu_helpers import inflate_run
    tiles = [d[i * TILE:(i + 1) * TILE] for d, s, _ in blobs for i in range(len(s))]
    got, st = inflate_run([x for _, s, _ in blobs for x in s], [len(t) for t in tiles],
                          [int(c) for _, _, cr in blobs for c in cr])
    assert [int(x) for x in st] == [0] * len(tiles)
    assert got == tiles


@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_deflate_one_tile_of_65536(content):
    data = CONTENTS[content](65536)
    streams, ln, cr = _run(data, 65536)
    _round_trip(data, 65536, streams, cr)


@pytest.mark.parametrize("content", ["fastq", "zeros", "random"])
def test_deflate_many_tiny_tiles(content):
    data = CONTENTS[content](100 * 40 + 37)     # tiles of 100 bytes: slots at every alignment
    streams, ln, cr = _run(data, 100)
    assert len(streams) == 41
    _round_trip(data, 100, streams, cr)


def test_deflate_one_symbol_code():
    data = b"\x07" * 5                           # one distinct byte, too short for a match
    streams, ln, cr = _run(data, TILE)
    _round_trip(data, TILE, streams, cr)


def _block_twice(second_at, n=65536, length=300):
    """A random block of non-zero bytes at offset 0 and again at second_at, zeros everywhere else.
    The compressor keeps one last position per hash of 4 bytes: every all-zero position shares one
    entry, so the block's own entries are still there when its copy comes (a filler of random bytes
    would overwrite all of them on the way), and both halves are compressible on their own."""
    block = bytes(_rng().integers(1, 256, length, dtype=np.uint8))
    a = bytearray(n)
    a[0:length] = block
    a[second_at:second_at + length] = block
    return bytes(a)


def _matches(stream, n):
    from deflate_helpers import deflate_tokens
    tokens, size = deflate_tokens(stream)
    assert size == n
    m = [t for t in tokens if t[0] == "match"]
    assert all(3 <= t[1] <= 258 and 1 <= t[2] <= 32768 and t[2] <= t[3] for t in m), "a match out of DEFLATE's range"
    return m


def test_deflate_repeat_at_distance_32768():
    """The window's reach: the block's copy is a match at distance exactly 32768 (distance symbol 29
    with all 13 extra bits set), read from the stream's own tokens."""
    data = _block_twice(32768)
    streams, ln, cr = _run(data, 65536)
    m = _matches(streams[0], 65536)
    far = [t for t in m if t[2] == 32768]
    # (a block position whose hash entry a later one took goes out as a literal: a few bytes at most)
    assert far and 32768 <= far[0][3] < 32768 + 16 and sum(t[1] for t in far) >= 280, far[:3]
    _round_trip(data, 65536, streams, cr)


def test_deflate_repeat_just_past_the_window_is_not_used():
    data = _block_twice(32769)                   # one byte too far: the copy goes out as literals
    streams, ln, cr = _run(data, 65536)
    m = _matches(streams[0], 65536)              # (no distance over 32768: checked there)
    assert not [t for t in m if t[3] < 32769 + 300 and t[3] + t[1] > 32769 and t[2] > 300]
    _round_trip(data, 65536, streams, cr)


def test_deflate_repeat_across_a_tile_boundary_is_not_used():
    """The same text in two tiles of 32768: the copy's source is in the other tile.  Each tile is
    inflated alone (check_streams), its matches stay inside it, and the second tile, identical to the
    first, gives the identical stream."""
    data = _block_twice(32768)
    streams, ln, cr = _run(data, TILE)
    assert len(streams) == 2
    for s in streams:
        m = _matches(s, TILE)                    # every distance <= the match's position in its own tile
        assert m and max(t[2] for t in m) < 32768
    assert streams[0] == streams[1]
    _round_trip(data, TILE, streams, cr)


def test_deflate_token_reader_agrees_with_zlib():
    """The tests' own token reader on zlib's streams (fixed, dynamic, stored), so that what it says
    of the kernel's streams can be believed."""
    from deflate_helpers import deflate_tokens
    data = fastq_text(70000)
    for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY)):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        tokens, size = deflate_tokens(c.compress(data) + c.flush())
        assert size == len(data)
        assert all(t[2] <= t[3] for t in tokens if t[0] == "match")


def test_deflate_sizes():
    """zlib on these inputs, for scale: the periodic text takes 370 bytes at level 1 and 23593 with
    Huffman codes alone; random ACGT 0.334 of its size at level 1, 0.282 Huffman-only, 0.535 with fixed
    codes."""
    _, ln, _ = _run(CONTENTS["line100"](TILE), TILE)
    print("line100:", int(ln[0]))
    assert int(ln[0]) <= 4096
    _, ln, _ = _run(CONTENTS["acgt"](TILE), TILE)
    print("acgt:", int(ln[0]) / TILE)
    assert int(ln[0]) <= 0.40 * TILE
    _, ln, _ = _run(CONTENTS["random"](TILE), TILE)
    print("random:", int(ln[0]))
    assert int(ln[0]) <= tile_bound(TILE)        # stored


def test_deflate_stride_above_the_bound():
    data = CONTENTS["fastq"](3 * 997 + 1)
    _run(data, 997, stride=tile_bound(997) + 11)


def test_deflate_bad_arguments():
    from find_circ2_amd import _native as N
    L = N.lib()
    buf = torch.zeros(1 << 17, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    ok = dict(src=p, n=100, tile=TILE, dst=p + 4096, stride=tile_bound(TILE), ln=p + 70000, cr=p + 70016, sc=p + 80000)
    bad = [dict(tile=0), dict(tile=65537), dict(stride=tile_bound(TILE) - 1), dict(src=None), dict(dst=None),
           dict(ln=None), dict(cr=None), dict(sc=None)]
    for b in bad:
        a = dict(ok, **b)
        rc = L.fc2_deflate_launch(a["src"], a["n"], a["tile"], a["dst"], a["stride"], a["ln"], a["cr"], a["sc"], None)
        assert rc == E_PARAM, b
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0                   # nothing was launched
    assert L.fc2_deflate_launch(None, 0, TILE, None, tile_bound(TILE), None, None, None, None) == 0
