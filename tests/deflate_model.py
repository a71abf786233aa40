"""A bit-exact model of one tile of the GPU DEFLATE compressor (deflate_kernel,
find_circ2_amd/csrc/fc2_deflate.hip): plain Python over bytes, one statement of the algorithm that the
kernel's header comment documents, so that "the kernel's bytes equal the model's" can be asked of any
input.  The model's own validity does not rest on the kernel: tests/test_deflate_model.py has zlib
inflate its streams and compares its codes' cost with an independent Huffman build.

model(data, a=0) -> (stream, info).  `a` is the destination's low four address bits: it changes no
byte of the stream, only info's count of stage flushes and of tokens that reach a third staging word.

`without` names branches to leave out, for the tests alone: they show that an input which reaches a
branch gives other bytes when the branch is missing, so that equality with the model would notice a
kernel that lacks it.  "repair": no overflow repair in build_code; "dummy": no dummy symbols in a
code with fewer than two; "cap138": a run of zeros over 138 goes out as one symbol 18; "rep16": no
symbol 16; "w2": a token's bits past the second staging word are lost; "keep": a flush forgets the
unfinished 16-byte piece."""

HASH_BITS = 12
MIN_MATCH, MAX_MATCH, MAX_DIST = 4, 258, 32768
STAGE_FLUSH = 2048
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def log2x16(x):
    """16 log2(x), x >= 1: the mantissa's top four bits stand for the fraction."""
    m = x.bit_length() - 1
    return 16 * m + ((((x << (31 - m)) & 0xFFFFFFFF) >> 27) & 15)


def len_sym(l):
    """Length l = len - 3 (0..255): symbol, extra-bit count, extra bits (RFC 1951 3.2.5)."""
    if l < 8:
        return 257 + l, 0, 0
    if l == 255:
        return 285, 0, 0
    eb = l.bit_length() - 3
    return 261 + 4 * eb + ((l >> eb) & 3), eb, l & ((1 << eb) - 1)


def dist_sym(d):
    """Distance d = dist - 1 (0..32767)."""
    if d < 4:
        return d, 0, 0
    m = d.bit_length() - 1
    eb = m - 1
    return 2 * m + ((d >> eb) & 1), eb, d & ((1 << eb) - 1)


def literal_cost(data):
    """What a literal costs on average, in 1/16 bit: the bytes' entropy, at least a bit each."""
    n = len(data)
    hist = [0] * 256
    for b in data:
        hist[b] += 1
    ln = log2x16(n)
    cost = 0
    for f in hist:
        if f:
            cost += f * max(16, ln - log2x16(f))
    return cost // n


def find_matches(data, lit16):
    """Pass 1: the tokens in position order (a literal's byte, or ("m", length, distance)), the two
    symbol histograms (the end of the block counted) and the tokens' extra bits."""
    n = len(data)
    pad = data + bytes(20)
    htab = [0] * (1 << HASH_BITS)
    lfreq, dfreq = [0] * 288, [0] * 32
    tokens, extra, skip = [], 0, 0
    for base in range(0, n, 64):
        top = min(base + 64, n)
        word, cand = {}, {}
        for p in range(base, top):                  # read first ...
            v = int.from_bytes(pad[p:p + 4], "little")
            word[p] = v
            if p + MIN_MATCH <= n:
                cand[p] = htab[((v * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)]
        for p in cand:                              # ... then enter the step's own positions
            h = ((word[p] * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)
            htab[h] = max(htab[h], p + 1)
        if skip >= base + 64:
            continue
        found = {}
        for p, c1 in cand.items():
            if not c1 or p < skip:
                continue
            c = c1 - 1
            d = p - c
            if d > MAX_DIST or pad[c:c + 4] != pad[p:p + 4]:
                continue
            maxlen = min(n - p, MAX_MATCH)
            l = 4
            while l < maxlen and pad[c + l] == pad[p + l]:
                l += 1
            l = min(l, maxlen)
            deb = (d - 1).bit_length() - 2 if d > 4 else 0
            if l >= MIN_MATCH and l * lit16 >= 16 * (11 + deb):
                found[p] = (l, d)
        p = max(skip, base)
        while p < top:                              # greedily from the lowest position on
            if p in found:
                l, d = found[p]
                tokens.append(("m", l, d))
                s, eb, _ = len_sym(l - 3)
                lfreq[s] += 1
                extra += eb
                s, eb, _ = dist_sym(d - 1)
                dfreq[s] += 1
                extra += eb
                p += l
                skip = p
            else:
                tokens.append(pad[p])
                lfreq[pad[p]] += 1
                p += 1
    lfreq[256] = 1
    return tokens, lfreq, dfreq, extra


def build_code(freq, n, maxbits, without=()):
    """Code lengths <= maxbits for freq[:n] and the bit-reversed canonical codewords; freq gets the
    dummy symbols of a code with fewer than two in use.  Returns (ok, lens, codes, clipped nodes)."""
    used = sum(1 for s in range(n) if freq[s])
    if used < 2 and "dummy" not in without:
        if freq[0] == 0:
            freq[0] = 1
            used += 1
        if used < 2:
            freq[1] = 1
    lens, codes = [0] * n, [0] * n
    order = sorted((freq[s], s) for s in range(n) if freq[s])
    m = max(used, 2)
    if len(order) < m:                              # ("dummy" left out: no code to build)
        return True, lens, codes, 0
    w = [f for f, _ in order] + [0] * (m - 1)
    par = [0] * (2 * m - 1)
    i, j = 0, m
    for k in range(m, 2 * m - 1):                   # two queues: the leaves, and the inner nodes as made
        total = 0
        for _ in range(2):
            if i < m and (j >= k or w[i] <= w[j]):
                pick = i
                i += 1
            else:
                pick = j
                j += 1
            total += w[pick]
            par[pick] = k
        w[k] = total
    blc = [0] * 17
    dep = [0] * (2 * m - 1)
    overflow = 0
    for k in range(2 * m - 3, -1, -1):
        d = dep[par[k]] + 1
        if d > maxbits:
            d = maxbits
            overflow += 1
        dep[k] = d
        if k < m:
            blc[d] += 1
    clipped = overflow
    while overflow > 0 and "repair" not in without:
        bits = maxbits - 1
        while bits > 0 and blc[bits] == 0:
            bits -= 1
        if bits == 0:
            break
        blc[bits] -= 1
        blc[bits + 1] += 2
        blc[maxbits] -= 1
        overflow -= 2
    kraft = sum(blc[b] << (maxbits - b) for b in range(1, maxbits + 1))
    if kraft != 1 << maxbits or sum(blc[1:maxbits + 1]) != m:
        return False, lens, codes, clipped
    idx = 0
    for b in range(maxbits, 0, -1):                 # the rarest symbols get the longest codewords
        for _ in range(blc[b]):
            lens[order[idx][1]] = b
            idx += 1
    nxt, c = [0] * 17, 0
    for b in range(1, maxbits + 1):
        c = (c + (blc[b - 1] if b > 1 else 0)) << 1
        nxt[b] = c
    for s in range(n):
        l = lens[s]
        if l:
            codes[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return True, lens, codes, clipped


def run_lengths(lens, without=()):
    """The code lengths as (symbol, extra) of the code-length alphabet, runs split as the kernel does."""
    out, k = [], 0
    while k < len(lens):
        val, run = lens[k], 1
        while k + run < len(lens) and lens[k + run] == val:
            run += 1
        k += run
        if val == 0:
            while run >= 11:
                r = run if "cap138" in without else min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((val, 0))
            run -= 1
            while run >= 3 and "rep16" not in without:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
        out += [(val, 0)] * run
    return out


class _Writer:
    """The stream's bits, least significant first, and what the kernel's staging does with them at
    destination alignment a."""

    def __init__(self, a, without):
        self.a, self.without = a, without
        self.buf, self.acc, self.nacc = bytearray(), 0, 0   # whole bytes, and the bits of the next ones
        self.stage0 = 0
        self.flushes = self.three_word = 0

    @property
    def bits(self):
        return 8 * len(self.buf) + self.nacc

    def put(self, v, nb):
        if not nb:
            return
        sh = (8 * self.a + self.bits - 8 * self.stage0) & 31
        if sh + nb > 64:
            self.three_word += 1
            if "w2" in self.without:
                v &= (1 << (64 - sh)) - 1
        self.acc |= v << self.nacc
        self.nacc += nb
        whole = self.nacc >> 3
        self.buf += (self.acc & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
        self.acc >>= 8 * whole
        self.nacc &= 7

    def flush(self):
        done = (8 * self.a + self.bits) >> 3        # whole bytes so far, as a coordinate
        if done - self.stage0 < STAGE_FLUSH:
            return
        self.stage0 = done & ~15
        self.flushes += 1
        if "keep" in self.without:
            k = self.stage0 - self.a
            self.buf[k:] = bytes(len(self.buf) - k)
            self.acc = 0

    def bytes(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.nacc else b"")


_CRC_TABLE = []
for _b in range(256):
    for _ in range(8):
        _b = (_b >> 1) ^ (0xEDB88320 if _b & 1 else 0)
    _CRC_TABLE.append(_b)


def crc32(data):
    """The gzip CRC-32 that goes out beside the stream."""
    r = 0xFFFFFFFF
    for b in data:
        r = (r >> 8) ^ _CRC_TABLE[(r ^ b) & 255]
    return r ^ 0xFFFFFFFF


def stored(data):
    """One stored block, or 65535 bytes and the last one (LEN is 16 bits)."""
    n = len(data)
    first = min(n, 65535)
    out = bytes([0 if n > 65535 else 1]) + first.to_bytes(2, "little") + (first ^ 0xFFFF).to_bytes(2, "little")
    out += data[:first]
    if n > 65535:
        out += b"\x01\x01\x00\xfe\xff" + data[65535:]
    return out


def model(data, a=0, without=()):
    """The stream deflate_kernel writes for one tile of 1..65536 bytes, and how it got there: info has
    kind ("dynamic" or "stored"), ntok and tokens, dfreq (the distance histogram, dummy symbols in it),
    clipped and maxlen (build_code's clipped nodes and the longest codeword of the literal/length,
    distance and code-length codes), hlit, hdist and hclen (the numbers of lengths sent: the header's
    fields are these less 257, 1 and 4), rle (the code lengths' (symbol, extra) pairs), widest (the
    widest token in bits) and, at alignment a, flushes (of the stage) and three_word (tokens whose bits
    reach a third staging word); and crc, the tile's CRC-32."""
    data = bytes(data)
    n = len(data)
    assert 1 <= n <= 65536 and 0 <= a < 16
    tokens, lfreq, dfreq, extra = find_matches(data, literal_cost(data))
    ok_l, llen, lcode, clip_l = build_code(lfreq, 286, 15, without)
    ok_d, dlen, dcode, clip_d = build_code(dfreq, 30, 15, without)
    ok = ok_l and ok_d
    data_bits = extra + sum(lfreq[s] * llen[s] for s in range(286)) + sum(dfreq[s] * dlen[s] for s in range(30))
    hlit, hdist, rle = 286, 30, []
    if ok:
        while hlit > 257 and llen[hlit - 1] == 0:
            hlit -= 1
        while hdist > 1 and dlen[hdist - 1] == 0:
            hdist -= 1
        rle = run_lengths(llen[:hlit] + dlen[:hdist], without)
    cfreq = [0] * 20
    for s, _ in rle:
        cfreq[s] += 1
    ok_c, clen, ccode, clip_c = build_code(cfreq, 19, 7, without)
    ok = ok and ok_c
    info = dict(ntok=len(tokens), clipped=(clip_l, clip_d, clip_c), maxlen=(max(llen), max(dlen), max(clen)),
                hlit=hlit, hdist=hdist, hclen=0, rle=rle, widest=0, flushes=0, three_word=0,
                dfreq=dfreq[:30], tokens=tokens, crc=crc32(data))
    out = _Writer(a, without)
    if ok:
        out.put(1 | (2 << 1), 3)                    # BFINAL, dynamic codes
        hclen = 19
        while hclen > 4 and clen[CL_ORDER[hclen - 1]] == 0:
            hclen -= 1
        info["hclen"] = hclen
        out.put(hlit - 257, 5)
        out.put(hdist - 1, 5)
        out.put(hclen - 4, 4)
        for k in range(hclen):
            out.put(clen[CL_ORDER[k]], 3)
        for s, e in rle:
            out.put(ccode[s], clen[s])
            if s >= 16:
                out.put(e, 2 if s == 16 else 3 if s == 17 else 7)
        out.three_word = 0                          # (the header's pieces are 7 bits at most)
    dyn_bytes = (out.bits + data_bits + 7) >> 3
    stored_bytes = n + (10 if n > 65535 else 5)
    if not (ok and dyn_bytes < stored_bytes):
        info["kind"] = "stored"
        return stored(data), info
    info["kind"] = "dynamic"
    for b0 in range(0, len(tokens), 64):
        for t in tokens[b0:b0 + 64]:
            if isinstance(t, tuple):
                s, eb, ev = len_sym(t[1] - 3)
                bits, nb = lcode[s] | (ev << llen[s]), llen[s] + eb
                s, eb, ev = dist_sym(t[2] - 1)
                bits |= dcode[s] << nb
                nb += dlen[s]
                bits |= ev << nb
                nb += eb
            else:
                bits, nb = lcode[t], llen[t]
            info["widest"] = max(info["widest"], nb)
            out.put(bits, nb)
        out.flush()
    out.put(lcode[256], llen[256])
    info["flushes"], info["three_word"] = out.flushes, out.three_word
    return out.bytes(), info
