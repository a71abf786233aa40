"""BGZF output (csrc/fc2_bgzf_out.hip, csrc/fc2_bgzf_frame_impl.h): the framing rule restated in Python, the
cases its host and device forms are swept over, and readers of what the writers produce."""
import gzip
import struct
import zlib

import numpy as np

E_PARAM, E_RANGE = -1, -4                        # include/fc2_bp.h
GAVE_UP = 0xFFFFFFFF
CANARY = 0xC3
HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
EOF_BLOCK = HEAD + bytes([0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def tile_bound(tile):
    """FC2_DEFLATE_TILE_BOUND (include/fc2_caller.h)."""
    return tile + 16


def stride_of(tile):
    return (tile_bound(tile) + 15) & ~15


def frame_py(slots, stride, out_len, crc, n_bytes, tile):
    """The rule of fc2_bgzf_frame_impl.h: (the block stream, the n_tiles + 1 offsets, total)."""
    n = len(out_len)
    if any(l == GAVE_UP or l == 0 or l > tile_bound(tile) or 26 + l > 65536 for l in out_len):
        return b"", [0] * (n + 1), 0
    out, off = bytearray(), []
    for i, l in enumerate(out_len):
        off.append(len(out))
        isize = tile if i + 1 < n else n_bytes - (n - 1) * tile
        out += HEAD + struct.pack("<H", 26 + l - 1) + bytes(slots[i * stride:i * stride + l])
        out += struct.pack("<II", crc[i], isize)
    off.append(len(out))
    return bytes(out), off, len(out)


SWEEP_TILE = 64
SWEEP_TILES = [1, 2, 63, 64, 65, 130]


def sweep_case(n_tiles, tile=SWEEP_TILE):
    """Slots of arbitrary bytes, out_len cycling 1..40 (block sizes 27..66: the offsets take every residue
    of 16), one tile at tile + 5 (the stored form's length), a short last tile: (slots, stride, out_len, crc,
    n_bytes, tile)."""
    rng = np.random.default_rng(1000 + n_tiles)
    stride = stride_of(tile)
    slots = rng.integers(0, 256, n_tiles * stride, dtype=np.uint8)
    out_len = np.array([1 + i % 40 for i in range(n_tiles)], np.uint32)
    out_len[n_tiles // 2] = tile + 5
    crc = rng.integers(0, 1 << 32, n_tiles, dtype=np.uint64).astype(np.uint32)
    return slots, stride, out_len, crc, (n_tiles - 1) * tile + 7, tile


def invalid_lengths(tile=SWEEP_TILE):
    """Each invalid form of out_len."""
    return [GAVE_UP, 0, tile_bound(tile) + 1]


def parse_blocks(blob):
    """[(BSIZE, the raw DEFLATE payload, CRC-32, ISIZE)] of a BGZF stream, every header checked."""
    blocks, pos = [], 0
    while pos < len(blob):
        assert blob[pos:pos + 16] == HEAD, "no BGZF header at %d" % pos
        bsize = struct.unpack_from("<H", blob, pos + 16)[0] + 1
        assert bsize >= 26 and pos + bsize <= len(blob)
        crc, isize = struct.unpack_from("<II", blob, pos + bsize - 8)
        blocks.append((bsize, blob[pos + 18:pos + bsize - 8], crc, isize))
        pos += bsize
    return blocks


def check_blocks(blob, data, block):
    """Every block of blob holds the next `block` bytes of data (the last one the rest): BSIZE at most 65536,
    the payload a complete raw DEFLATE stream of those bytes, their CRC-32 and count; and any gzip reader
    sees data again."""
    blocks = parse_blocks(blob)
    assert len(blocks) == -(-len(data) // block)
    for i, (bsize, payload, crc, isize) in enumerate(blocks):
        want = data[i * block:(i + 1) * block]
        assert bsize <= 65536
        z = zlib.decompressobj(-15)
        got = z.decompress(payload)
        assert z.eof and z.unused_data == b"", i
        assert got == want, "block %d inflates to other bytes" % i
        assert crc == zlib.crc32(want) and isize == len(want), i
    assert (gzip.decompress(blob) if blob else b"") == data
    return blocks


def bam_like(n, seed=7):
    """n bytes shaped like BAM records: block_size, fixed fields, a name, CIGAR words, packed bases,
    qualities, a few tags."""
    rng = np.random.default_rng(seed)
    out, size, k = [], 0, 0
    while size < n:
        lseq = int(rng.integers(30, 101))
        name = b"read_%07d\0" % k
        body = struct.pack("<iiBBHHHiiii", int(rng.integers(0, 3)), int(rng.integers(0, 90000)), len(name), 60, 4681, 2,
                           int(rng.choice([0, 16, 2048])), lseq, -1, -1, 0)
        body += name + struct.pack("<II", (lseq // 2) << 4, ((lseq + 1) // 2) << 4 | 4)
        body += rng.integers(0, 256, (lseq + 1) // 2, dtype=np.uint8).tobytes()
        body += np.minimum(40, rng.geometric(0.15, lseq)).astype(np.uint8).tobytes()
        body += b"ASC" + bytes([lseq // 2]) + b"XSC" + bytes([int(rng.integers(0, 30))]) + b"NMC\0"
        rec = struct.pack("<i", len(body)) + body
        out.append(rec)
        size += len(rec)
        k += 1
    return b"".join(out)[:n]


def read_bam(path):
    """(the BGZF blocks of the file, the inflated stream, the offset of the first record in it)."""
    blob = open(path, "rb").read()
    data = gzip.decompress(blob)
    assert data[:4] == b"BAM\1"
    lt, = struct.unpack_from("<i", data, 4)
    o = 8 + lt
    nref, = struct.unpack_from("<i", data, o)
    o += 4
    for _ in range(nref):
        ln, = struct.unpack_from("<i", data, o)
        o += 8 + ln
    return parse_blocks(blob), data, o
