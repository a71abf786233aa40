"""BGZF blocks made of several tiles (csrc/fc2_bgzf_frame_impl.h "groups"): the rule restated in Python, the CRC
combine, the cases the host and device forms are swept over, and slots filled by zlib the way the compressor
over groups fills them."""
import struct
import zlib

import numpy as np

from bgzf_helpers import GAVE_UP, HEAD, stride_of, tile_bound

POLY = 0xEDB88320


def _mul(a, b):
    """a * b modulo the CRC-32 polynomial, bit 31 the coefficient of x^0."""
    p, m = 0, 1 << 31
    while m:
        if a & m:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
        m >>= 1
    return p


def crc_append(crc_a, crc_b, n_b):
    """The CRC-32 of A followed by the n_b bytes of B: crc_a times x^(8 n_b), then crc_b."""
    pw, n = 1 << 23, n_b                            # x^8
    while n:
        if n & 1:
            crc_a = _mul(pw, crc_a)
        pw = _mul(pw, pw)
        n >>= 1
    return crc_a ^ crc_b


def tiles_of(n_bytes, group, tile):
    tpg = (group - 1) // tile + 1
    return n_bytes // group * tpg + (n_bytes % group + tile - 1) // tile


def frame_groups_py(slots, stride, out_len, crc, n_bytes, group, tile):
    """(the block stream, the n_groups + 1 offsets, total)."""
    n_groups, tpg = -(-n_bytes // group), (group - 1) // tile + 1
    layout = []
    for g in range(n_groups):
        gbytes = min(group, n_bytes - g * group)
        layout.append((gbytes, [(g * tpg + k, min(tile, gbytes - k * tile)) for k in range(-(-gbytes // tile))]))
    bad = any(l == GAVE_UP or l == 0 or l > tile_bound(tile) or 26 + l > 65536 for l in out_len) or \
        any(26 + sum(out_len[i] for i, _ in tiles) > 65536 for _, tiles in layout)
    if bad:
        return b"", [0] * (n_groups + 1), 0
    out, off = bytearray(), []
    for gbytes, tiles in layout:
        off.append(len(out))
        payload, c = bytearray(), 0
        for k, (i, n) in enumerate(tiles):
            payload += bytes(slots[i * stride:i * stride + out_len[i]])
            c = crc_append(c, crc[i], n) if k else crc[i]
        out += HEAD + struct.pack("<H", 26 + len(payload) - 1) + payload + struct.pack("<II", c, gbytes)
    off.append(len(out))
    return bytes(out), off, len(out)


SWEEP_TILE = 64
SWEEP_GROUPS = [1, 2, 3, 65]
SWEEP_TPG = [1, 2, 4, 16]


def sweep_case(n_groups, tpg, last=None, tile=SWEEP_TILE):
    """Slots of arbitrary bytes for n_groups groups of tpg tiles (the group 7 bytes short of tpg tiles, so every
    group's last tile is short when tpg > 1), out_len cycling 1..40 with one tile at tile + 5, arbitrary CRCs, the
    last group `last` bytes long (default: its last tile 1 byte): (slots, stride, out_len, crc, n_bytes, group, tile)."""
    group = tpg * tile - (7 if tpg > 1 else 0)
    if last is None:
        last = (tpg - 1) * tile + 1 if n_groups > 1 or tpg > 1 else 7
    assert 1 <= last <= group
    n_bytes = (n_groups - 1) * group + last
    n = tiles_of(n_bytes, group, tile)
    rng = np.random.default_rng(1000 * n_groups + tpg)
    stride = stride_of(tile)
    slots = rng.integers(0, 256, (n + 1) * stride, dtype=np.uint8)       # (one slot more: reads of whole words)
    out_len = np.array([1 + i % 40 for i in range(n)], np.uint32)
    out_len[n // 2] = tile + 5
    crc = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return slots, stride, out_len, crc, n_bytes, group, tile


def zlib_slots(data, group, tile):
    """What fc2_deflate_launch_groups leaves, from zlib level 1: a raw stream a group, flushed to a byte boundary
    at every tile's end but the group's last: (slots, stride, out_len, crc)."""
    stride, tpg = stride_of(tile), (group - 1) // tile + 1
    n = tiles_of(len(data), group, tile)
    slots = np.full((n + 1) * stride, 0xEE, np.uint8)
    ln, cr = [0] * n, [0] * n
    for g, g0 in enumerate(range(0, len(data), group)):
        part = data[g0:g0 + group]
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        for k, t0 in enumerate(range(0, len(part), tile)):
            t = part[t0:t0 + tile]
            s = z.compress(t) + (z.flush() if t0 + tile >= len(part) else z.flush(zlib.Z_SYNC_FLUSH))
            i = g * tpg + k
            assert 0 < len(s) <= tile_bound(tile), (len(s), tile)
            slots[i * stride:i * stride + len(s)] = np.frombuffer(s, np.uint8)
            ln[i], cr[i] = len(s), zlib.crc32(t)
    return slots, stride, ln, cr
