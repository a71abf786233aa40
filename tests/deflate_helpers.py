"""The GPU DEFLATE compressor (csrc/fc2_deflate.hip) through its C entry points, and the inputs its
tests share."""
import ctypes
import zlib

import numpy as np

from find_circ2_amd import _native as N

E_PARAM = -1                                     # include/fc2_bp.h


def tile_bound(tile):
    """FC2_DEFLATE_TILE_BOUND (include/fc2_caller.h)."""
    return tile + 16


def pattern(n):
    """What the output buffer holds before a launch (byte i of the allocation)."""
    return ((np.arange(n, dtype=np.int64) * 193 + 57) & 255).astype(np.uint8)


def deflate_launch(data: bytes, tile: int, stride=None, dst_offset=0, src_offset=0):
    """fc2_deflate_launch over data: (the whole output buffer, out_len, crc, stride).  The buffer is
    pre-filled with pattern() and has one guard slot before the first tile's slot and one after the
    last; the default stride is the bound itself, so slots fall on every alignment.  The allocations
    are 16-byte aligned: the first tile's slot lies at (stride + dst_offset) % 16, the first input byte
    at src_offset % 16 (the bytes skipped are not part of what is returned, and stay as they were)."""
    import torch
    stride = tile_bound(tile) if stride is None else stride
    n = len(data)
    tiles = (n + tile - 1) // tile
    dev = torch.device("cuda:0")
    before = bytes(0xA5 ^ i for i in range(src_offset))
    src = torch.tensor(np.frombuffer(before + data, np.uint8).copy(), device=dev) if n + src_offset else \
        torch.zeros(1, dtype=torch.uint8, device=dev)
    skipped = np.full(dst_offset, 0x5A, np.uint8)
    dst = torch.tensor(np.concatenate([skipped, pattern((max(1, tiles) + 2) * stride)]), device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ln = torch.full((max(1, tiles),), -7, dtype=torch.int32, device=dev)
    cr = torch.full((max(1, tiles),), -7, dtype=torch.int32, device=dev)
    scratch = torch.zeros(max(4, int(N.lib().fc2_deflate_scratch_bytes(n, tile))), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().fc2_deflate_launch(src.data_ptr() + src_offset, n, tile, dst.data_ptr() + dst_offset + stride, stride,
                                       ln.data_ptr(), cr.data_ptr(), scratch.data_ptr(), ctypes.c_void_p(stream)))
    torch.cuda.synchronize(dev)
    d = dst.cpu().numpy()
    assert (d[:dst_offset] == skipped).all(), "bytes before the output buffer were written"
    return (d[dst_offset:], ln.cpu().numpy().view(np.uint32)[:tiles], cr.cpu().numpy().view(np.uint32)[:tiles],
            stride)


def check_streams(data: bytes, tile: int, d, ln, cr, stride):
    """What every launch must satisfy (zlib as the reference); returns the tiles' streams."""
    tiles = (len(data) + tile - 1) // tile
    assert len(ln) == len(cr) == tiles
    clean = d == pattern(len(d))
    assert clean[:stride].all(), "the guard slot before the tiles was written"
    assert clean[(tiles + 1) * stride:].all(), "the guard slot after the tiles was written"
    streams = []
    for i in range(tiles):
        want = data[i * tile:(i + 1) * tile]
        n = int(ln[i])
        assert 0 < n <= tile_bound(tile), (i, n)
        a = (i + 1) * stride
        bad = np.nonzero(~clean[a + n:a + stride])[0]
        assert len(bad) == 0, "tile %d wrote at byte %d of its slot, past its %d bytes" % (i, n + int(bad[0]), n)
        s = d[a:a + n].tobytes()
        z = zlib.decompressobj(-15)
        got = z.decompress(s)                   # alone: a reference before the tile's start fails here
        assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b"", i
        assert got == want, "tile %d inflates to other bytes" % i
        assert int(cr[i]) == zlib.crc32(want), i
        streams.append(s)
    return streams


def fastq_text(n, seed=11):
    """A FASTQ-shaped text of n bytes: @name / bases / + / qualities, some name bytes >= 0x80."""
    rng = np.random.default_rng(seed)
    out, size, k = [], 0, 0
    while size < n:
        ln = int(rng.integers(30, 101))
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)].tobytes()
        qual = (33 + np.minimum(40, rng.geometric(0.15, ln))).astype(np.uint8).tobytes()
        name = b"@read_%07d_" % k + ("éü" if k % 7 == 0 else "x").encode("utf-8") + b"/1"
        rec = name + b"\n" + seq + b"\n+\n" + qual + b"\n"
        out.append(rec)
        size += len(rec)
        k += 1
    return b"".join(out)[:n]


def _rng():
    return np.random.default_rng(2024)


def _line100():
    return bytes(_rng().integers(0, 256, 100, dtype=np.uint8))


CONTENTS = {
    "zeros": lambda n: b"\x00" * n,                      # an overlapping match at distance 1
    "ab": lambda n: (b"AB" * (n // 2 + 1))[:n],
    "line100": lambda n: (_line100() * (n // 100 + 1))[:n],
    "acgt": lambda n: np.frombuffer(b"ACGT", np.uint8)[_rng().integers(0, 4, n)].tobytes(),
    "random": lambda n: bytes(_rng().integers(0, 256, n, dtype=np.uint8)),
    "range256": lambda n: (bytes(range(256)) * (n // 256 + 1))[:n],
    "fastq": lambda n: fastq_text(n),
}


# ---- an independent reader of a raw DEFLATE stream's tokens (RFC 1951), for what zlib does not tell ----
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, data):
        self.data = bytes(data)
        self.pos = 0

    def take(self, n):                           # n <= 16; past the end the bits are zeros
        i = self.pos >> 3
        x = (int.from_bytes(self.data[i:i + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)
        self.pos += n
        return x


def _decoder(lengths):
    """{(length, code MSB-first): symbol} of the canonical code (RFC 1951 3.2.2)."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise ValueError("no such codeword")


def deflate_tokens(stream: bytes):
    """The tokens of a raw DEFLATE stream in order: ("lit", byte), ("match", length, distance, position
    of its first byte), ("stored", length); and the number of bytes they stand for."""
    out, pos, _ = _read(stream)
    return out, pos


def deflate_blocks(stream: bytes):
    """deflate_tokens, and the stream's blocks in order: ("stored",), ("fixed",), or ("dynamic", the
    literal/length code's lengths (HLIT of them), the distance code's (HDIST), the code-length code's
    (all 19, by symbol), HCLEN, the code-length symbols the lengths were sent with)."""
    return _read(stream)


def _read(stream):
    bits, out, pos, blocks = _Bits(stream), [], 0, []
    while True:
        final, kind = bits.take(1), bits.take(2)
        if kind == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            assert n == (~nn & 0xFFFF)
            bits.pos += 8 * n
            out.append(("stored", n))
            blocks.append(("stored",))
            pos += n
        else:
            assert kind in (1, 2)
            if kind == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dl = [5] * 30
                blocks.append(("fixed",))
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[_CLORDER[k]] = bits.take(3)
                ct, lens, sent = _decoder(cl), [], []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, ct)
                    sent.append(s)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.take(3))
                    else:
                        lens += [0] * (11 + bits.take(7))
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                blocks.append(("dynamic", ll, dl, cl, hclen, sent))
            lt, dt = _decoder(ll), _decoder(dl)
            while True:
                s = _symbol(bits, lt)
                if s < 256:
                    out.append(("lit", s))
                    pos += 1
                elif s == 256:
                    break
                else:
                    n = _LBASE[s - 257] + bits.take(_LEXT[s - 257])
                    d = _symbol(bits, dt)
                    dist = _DBASE[d] + bits.take(_DEXT[d])
                    out.append(("match", n, dist, pos))
                    pos += n
        if final:
            return out, pos, blocks


def _kind(blocks):
    return [b[0] for b in blocks]


def explain(got, want):
    """The first stage at which the kernel's stream leaves the model's: kind, tokens, code lengths, bytes."""
    if got == want:
        return None
    try:
        gt, gsize, gb = deflate_blocks(got)
    except Exception as e:                       # (not a DEFLATE stream at all)
        return "the kernel's stream cannot be read: %r" % (e,)
    wt, wsize, wb = deflate_blocks(want)
    if _kind(gb) != _kind(wb):
        return "kind: %s, the model's %s" % (_kind(gb), _kind(wb))
    if gt != wt:
        k = next((i for i, (x, y) in enumerate(zip(gt, wt)) if x != y), min(len(gt), len(wt)))
        return "tokens: %d against %d, the first other one at %d: %s, the model's %s" % (
            len(gt), len(wt), k, gt[k:k + 1], wt[k:k + 1])
    for name, col in (("literal/length", 1), ("distance", 2), ("code length", 3)):
        for x, y in zip(gb, wb):
            if x[0] == "dynamic" and x[col] != y[col]:
                return "%s code lengths: %s, the model's %s" % (name, x[col], y[col])
    k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    return "bytes: %d against %d, the first other one at %d" % (len(got), len(want), k)
