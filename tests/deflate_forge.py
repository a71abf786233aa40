"""A bit-level DEFLATE writer (RFC 1951) for tests: streams put together from explicit instructions,
so that a case can hold any form the format allows -- or forbids -- and not only what a compressor
happens to emit.

A ``Forge`` collects blocks: ``stored``, ``fixed`` (a token list under the fixed code) and
``dynamic`` (given literal/length lengths, given distance lengths, a token list; the code-length
section -- plain symbols or the 16/17/18 repeats, HCLEN, a repeat spanning the HLIT/HDIST boundary,
the code-length code itself -- under the caller's control).  A token is

- an int: that literal;
- ``(length, dist)``: a match;
- ``Sym(s)``: literal/length symbol s by its number (no extra bits);
- ``LenOnly(length)``: a length symbol with its extra bits and no distance after it;
- ``Code(code, nbits)``: a raw codeword, MSB first as Huffman codes are packed -- also one the
  block's code does not contain;
- ``Raw(value, nbits)``: raw bits, LSB first.

``make_code`` gives the lengths of a complete code, ``expand`` the bytes a token list stands for
(no inflater asked)."""
from collections import namedtuple

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
         227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
         4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32

Sym = namedtuple("Sym", "sym")
LenOnly = namedtuple("LenOnly", "length")
Code = namedtuple("Code", "code nbits")
Raw = namedtuple("Raw", "value nbits")

_LEN_SYM = [0] * 259
for _i, _b in enumerate(LBASE):
    for _l in range(_b, min(259, _b + (1 << LEXT[_i]))):
        _LEN_SYM[_l] = _i                       # (258: symbol 285, not 284 with all its extra bits set)
_DIST_SYM = [0] * 32769
for _i, _b in enumerate(DBASE):
    for _d in range(_b, _b + (1 << DEXT[_i])):
        _DIST_SYM[_d] = _i


def _rev(code, nbits):
    r = 0
    for _ in range(nbits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canon(lengths):
    """The canonical code of RFC 1951 3.2.2: {symbol: (codeword reversed for LSB-first packing, its
    length)}.  Incomplete and over-subscribed length sets get the numbers the algorithm gives them."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (_rev(nxt[l] & ((1 << l) - 1), l), l)
            nxt[l] += 1
    return out


def make_code(n, maxlen):
    """The lengths (ascending) of a complete code of n symbols whose longest codeword has maxlen bits:
    the chain 1, 2, ..., maxlen, maxlen with its shortest leaf split until there are n leaves."""
    assert maxlen + 1 <= n <= (1 << maxlen), (n, maxlen)
    count = [0] * (maxlen + 1)
    for l in range(1, maxlen + 1):
        count[l] = 1
    count[maxlen] = 2
    for _ in range(n - (maxlen + 1)):
        l = next(k for k in range(1, maxlen) if count[k])
        count[l] -= 1
        count[l + 1] += 2
    return [l for l in range(1, maxlen + 1) for _ in range(count[l])]


def kraft(lengths):
    """Code space used, in units of 2^-15: 32768 for a complete code."""
    return sum(1 << (15 - l) for l in lengths if l)


def cl_plain(lengths):
    """A code-length section of plain symbols only."""
    return list(lengths)


def cl_rle(lengths):
    """A code-length section with the 16/17/18 repeats taken greedily over the whole sequence given
    (over literal/length and distance lengths in one piece, a repeat may span the boundary)."""
    ops, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                ops.append((18, k))
                run -= k
            if run >= 3:
                ops.append((17, run))
                run = 0
            ops += [0] * run
        else:
            ops.append(v)
            run -= 1
            while run >= 3:
                k = min(run, 6)
                ops.append((16, k))
                run -= k
            ops += [v] * run
        i = j
    return ops


def expand(prefix, tokens):
    """The bytes `tokens` (literals and matches) stand for, after the output `prefix`; only those
    bytes (not the prefix) are returned."""
    out = bytearray(prefix)
    n0 = len(out)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            assert 1 <= dist <= len(out), (dist, len(out))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                piece = bytes(out[-dist:])
                out += (piece * (length // dist + 1))[:length]
    return bytes(out[n0:])


class Forge:
    """Raw DEFLATE, block by block; ``bytes(forge)`` is the stream (its last byte zero-padded)."""

    def __init__(self):
        self._out = bytearray()
        self._acc = 0                            # the bits not yet in _out, LSB first
        self._n = 0
        self.symbols = 0                         # tokens written so far

    # ---- bits ---------------------------------------------------------------------------------
    def bits(self, value, nbits):
        self._acc |= (value & ((1 << nbits) - 1)) << self._n
        self._n += nbits
        if self._n >= 64:
            k = self._n >> 3
            self._out += (self._acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self._acc >>= 8 * k
            self._n -= 8 * k
        return self

    def code(self, code, nbits):
        return self.bits(_rev(code, nbits), nbits)

    def align(self):
        if self._n & 7:
            self.bits(0, 8 - (self._n & 7))
        return self

    def raw_bytes(self, data):
        self.align()
        k = self._n >> 3
        self._out += self._acc.to_bytes(k, "little") + bytes(data)
        self._acc = self._n = 0
        return self

    def bit_length(self):
        return 8 * len(self._out) + self._n

    def __bytes__(self):
        k = (self._n + 7) >> 3
        return bytes(self._out) + self._acc.to_bytes(k, "little")

    # ---- blocks -------------------------------------------------------------------------------
    def header(self, final, btype):
        return self.bits(1 if final else 0, 1).bits(btype, 2)

    def stored(self, data, final=False, nlen=None):
        """A stored block; `nlen` overrides the complement of LEN."""
        assert len(data) <= 65535
        self.header(final, 0).align()
        self.bits(len(data), 16).bits((~len(data)) & 0xFFFF if nlen is None else nlen, 16)
        return self.raw_bytes(data)

    def tokens(self, toks, lcode, dcode):
        bits = self.bits
        for t in toks:
            if isinstance(t, int):
                c, n = lcode[t]
                bits(c, n)
            elif isinstance(t, Sym):
                c, n = lcode[t.sym]
                bits(c, n)
            elif isinstance(t, Code):
                self.code(t.code, t.nbits)
            elif isinstance(t, Raw):
                bits(t.value, t.nbits)
            else:
                length = t.length if isinstance(t, LenOnly) else t[0]
                s = _LEN_SYM[length]
                c, n = lcode[257 + s]
                bits(c, n)
                if LEXT[s]:
                    bits(length - LBASE[s], LEXT[s])
                if not isinstance(t, LenOnly):
                    s = _DIST_SYM[t[1]]
                    c, n = dcode[s]
                    bits(c, n)
                    if DEXT[s]:
                        bits(t[1] - DBASE[s], DEXT[s])
        self.symbols += len(toks)
        return self

    def fixed(self, toks, final=False, eob=True):
        self.header(final, 1)
        lcode = canon(FIXED_LL)
        self.tokens(toks, lcode, canon(FIXED_DL))
        if eob:
            self.bits(*lcode[256])
        return self

    def dynamic(self, ll, dl, toks, final=False, eob=True, cl_ops=None, cl_lens=None, hclen=None, hlit=None,
                hdist=None):
        """A dynamic block with literal/length lengths `ll` and distance lengths `dl`.  `cl_ops`: the
        code-length section, ints 0..15 and (16 | 17 | 18, repeat count) pairs (default: the repeats
        taken greedily within each of the two codes); `cl_lens`: the 19 lengths of the code-length
        code (default: a complete code over the symbols used); `hclen`: how many of them are written
        (default: up to the last non-zero one); `hlit`, `hdist`: the header's count fields (default:
        len(ll) - 257, len(dl) - 1)."""
        if cl_ops is None:
            cl_ops = cl_rle(ll) + cl_rle(dl)
        if cl_lens is None:
            used = sorted({op if isinstance(op, int) else op[0] for op in cl_ops})
            if len(used) < 2:                    # a second, unused symbol completes the code
                used = sorted(set(used) | {1 if used == [0] else 0})
            m = min(7, len(used) - 1)
            cl_lens = [0] * 19
            for s, l in zip(used, make_code(len(used), m)):
                cl_lens[s] = l
        last = max([k for k in range(19) if cl_lens[CL_ORDER[k]]] + [3]) + 1
        ncl = last if hclen is None else hclen
        assert 4 <= ncl <= 19
        self.header(final, 2)
        self.bits(len(ll) - 257 if hlit is None else hlit, 5)
        self.bits(len(dl) - 1 if hdist is None else hdist, 5)
        self.bits(ncl - 4, 4)
        for k in range(ncl):
            self.bits(cl_lens[CL_ORDER[k]], 3)
        clcode = canon(cl_lens)
        for op in cl_ops:
            if isinstance(op, int):
                self.bits(*clcode[op])
            elif isinstance(op, (Code, Raw)):
                self.tokens([op], None, None)
            else:
                s, rep = op
                self.bits(*clcode[s])
                if s == 16:
                    self.bits(rep - 3, 2)
                elif s == 17:
                    self.bits(rep - 3, 3)
                else:
                    self.bits(rep - 11, 7)
        lcode = canon(ll)
        self.tokens(toks, lcode, canon(dl))
        if eob:
            self.bits(*lcode[256])
        return self
