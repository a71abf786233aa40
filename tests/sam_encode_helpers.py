"""BAM records from SAM text (csrc/fc2_sam_encode_impl.h): the entries' callers, the planted and the refused
lines, bwa-shaped lines and their seeded mutations, shared by the host, writer and device tests."""
import ctypes

import numpy as np

from find_circ2_amd import _native as N

E_PARAM, E_FORMAT, E_RANGE, E_IO = -1, -3, -4, -5     # include/fc2_bp.h
CANARY = 0xC3
MAX_LINES, MAX_TEXT = 16384, 4 << 20
ENC_OFFSETS, ENC_LONG = 7, 8                          # FC2_SAM_ENC_OFFSETS, FC2_SAM_ENC_LONG (include/fc2_ingest.h)
# "dup" twice: the last one's index counts, as in the ingest's own map
NAMES = [b"chr1", b"chr2", b"chrX", b"dup", b"chr3", b"dup"]


def bound(text_bytes, n_lines):
    return 2 * text_bytes + 40 * n_lines


def c_names(names):
    return (ctypes.c_char_p * max(1, len(names)))(*names)


def names_table(names=NAMES):
    need = ctypes.c_uint64()
    arr = c_names(names)
    assert N.lib().fc2_sam_names_table(arr, None, len(names), None, 0, ctypes.byref(need)) == 0
    t = np.zeros(need.value // 4, np.uint32)
    assert N.lib().fc2_sam_names_table(arr, None, len(names), t.ctypes.data, need.value, ctypes.byref(need)) == 0
    return t


def pack(lines):
    """(the lines back to back as uint8, the len(lines) + 1 offsets)."""
    off = np.zeros(len(lines) + 1, np.uint32)
    off[1:] = np.cumsum([len(l) for l in lines])
    text = np.frombuffer(b"".join(lines) + b"\0", np.uint8).copy()      # (never empty)
    return text, off


def encode_host_packed(text, nb, off, table):
    """fc2_sam_encode_host on `nb` bytes of text under any len(off) - 1 offsets, ascending or not: (status, size,
    out_off, total, the output with 64 canary bytes after the bound)."""
    n = len(off) - 1
    cap = bound(nb, n)
    out = np.full(cap + 64, CANARY, np.uint8)
    status, size = np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xDEADBEEF, np.uint32)
    out_off, total = np.full(n + 1, 0xDEADBEEF, np.uint32), ctypes.c_uint32(0xDEADBEEF)
    rc = N.lib().fc2_sam_encode_host(text.ctypes.data, nb, off.ctypes.data, n, table.ctypes.data, table.nbytes, out.ctypes.data,
                                     cap, out_off.ctypes.data, size.ctypes.data, status.ctypes.data, ctypes.addressof(total))
    assert rc == 0, N.lib().fc2_last_error()
    return status, size, out_off, int(total.value), out


def encode_host(lines, names=NAMES, table=None):
    """encode_host_packed on one batch of lines."""
    text, off = pack(lines)
    return encode_host_packed(text, int(off[-1]), off, names_table(names) if table is None else table)


def encode_host_all(lines, names=NAMES):
    """encode_host over any number of lines, in batches the rule takes: (status list, record-or-None list).  A line
    no batch holds ends the batch before it and is FC2_SAM_ENC_LONG, as in fc2_gpu_sam_encode."""
    table = names_table(names)
    st, recs, i = [], [], 0
    while i < len(lines):
        if len(lines[i]) > MAX_TEXT:
            st.append(ENC_LONG)
            recs.append(None)
            i += 1
            continue
        j, nb = i, 0
        while j < len(lines) and j - i < MAX_LINES and nb + len(lines[j]) <= MAX_TEXT:
            nb += len(lines[j])
            j += 1
        status, size, out_off, total, out = encode_host(lines[i:j], names, table)
        assert (out[total:] == CANARY).all(), "bytes at or after total were written"
        assert int(out_off[-1]) == total == int(size.sum())
        for k in range(j - i):
            st.append(int(status[k]))
            recs.append(out[int(out_off[k]):int(out_off[k]) + int(size[k])].tobytes() if status[k] == 0 else None)
            assert (status[k] == 0) == (size[k] != 0)
        i = j
    return st, recs


_line_buf = ctypes.create_string_buffer(1 << 20)


def encode_line(line, names=NAMES, _cache={}):
    """fc2_sam_encode_line, the yardstick (encode_sam itself): (rc, the record's bytes or None, the message)."""
    key = tuple(names)
    if key not in _cache:
        _cache[key] = c_names(names)
    n = ctypes.c_uint64()
    rc = N.lib().fc2_sam_encode_line(line, len(line), _cache[key], len(names), _line_buf, len(_line_buf), ctypes.byref(n))
    if rc != 0:
        return rc, None, N.lib().fc2_last_error().decode("latin-1")
    return 0, _line_buf.raw[:n.value], ""


def check_contract(lines, names=NAMES):
    """Never a wrong byte: for every line status != 0 (and no bytes), or the bytes are the yardstick's and the
    yardstick succeeded.  Returns the statuses."""
    st, recs = encode_host_all(lines, names)
    for i, line in enumerate(lines):
        if st[i] == 0:
            rc, want, msg = encode_line(line, names)
            assert rc == 0, (i, line[:200], msg)
            assert recs[i] == want, (i, line[:200])
    return st


def sam_line(qname=b"r1", flag=b"0", rname=b"chr1", pos=b"100", mapq=b"60", cigar=b"10M", rnext=b"*", pnext=b"0", tlen=b"0",
             seq=b"ACGTACGTAC", qual=b"IIIIIIIIII", tags=()):
    return b"\t".join([qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual] + list(tags))


def _seq(n, rng):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def planted_lines():
    """Every form the device rule must accept (the issue's list)."""
    rng = np.random.default_rng(11)
    L = []
    for flag in (b"0", b"16", b"2064"):
        L.append(sam_line(flag=flag))
    L += [sam_line(pos=b"0"), sam_line(pos=b"1"), sam_line(mapq=b"255"), sam_line(flag=b"4", pos=b"0", rname=b"*", cigar=b"*")]
    L += [sam_line(cigar=b"*"), sam_line(cigar=b"10M")]
    L += [sam_line(cigar=b"3" + bytes([op])) for op in b"MIDNSHP=X"]
    L.append(sam_line(cigar=b"".join(b"%d%c" % (1 + k % 7, b"MIDNSHP=X"[k % 9]) for k in range(1000))))
    L += [sam_line(cigar=b"268435455M"), sam_line(cigar=b"5S268435455N5M"), sam_line(pos=b"999999999", cigar=b"268435455D")]
    for rnext in (b"=", b"*", b"chr2", b"nowhere", b"dup"):
        L.append(sam_line(rnext=rnext, pnext=b"500"))
    L += [sam_line(rname=b"dup"), sam_line(rname=b"nowhere", rnext=b"="), sam_line(rname=b"=", rnext=b"=")]
    L += [sam_line(tlen=b"-350"), sam_line(tlen=b"-999999999", pnext=b"-5", pos=b"-3", flag=b"-1", mapq=b"-1")]
    L += [sam_line(flag=b"65536", mapq=b"256"), sam_line(flag=b"999999999", mapq=b"999999999")]
    L.append(sam_line(seq=b"*", qual=b"*"))
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 300):
        s = _seq(n, rng)
        L.append(sam_line(seq=s, qual=bytes(33 + int(q) for q in rng.integers(0, 42, n)), cigar=b"%dM" % n))
    L.append(sam_line(seq=b"acgtnRYKM=.ryswkmbdhvNU", qual=b"*"))
    L.append(sam_line(seq=bytes(b for b in range(256) if b != 9), qual=b"*"))          # every byte nt16 can meet
    L.append(sam_line(seq=b"", qual=b""))
    L += [sam_line(qual=b"*"), sam_line(qual=b"III"), sam_line(qual=b"I" * 25), sam_line(seq=b"*", qual=b"IIII")]
    L.append(sam_line(qual=bytes([33, 32, 0, 255, 126, 34, 35, 36, 37, 38])))
    L.append(sam_line())                                                                # no tags at all
    L += [sam_line(tags=[b"XA:A:x"]), sam_line(tags=[b"XA:A:"]), sam_line(tags=[b"XA:A:xyz"])]
    for v in (-2147483649, -2147483648, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 4294967295, 4294967296,
              999999999999999999, -999999999999999999):
        L.append(sam_line(tags=[b"NM:i:%d" % v]))
    L += [sam_line(tags=[b"NM:i:-0"]), sam_line(tags=[b"NM:i:007"])]
    L += [sam_line(tags=[b"XZ:Z:"]), sam_line(tags=[b"XZ:Z:" + b"z" * 200]), sam_line(tags=[b"XH:H:1AE301"])]
    L.append(sam_line(tags=[b"NM:i:2", b"MD:Z:10A5^AC6", b"AS:i:94", b"XS:i:0", b"SA:Z:chr2,500,+,50M50S,60,1;", b"XA:A:q"]))
    L += [sam_line(qname=b"q"), sam_line(qname=b"n" * 254)]
    return L + lane_boundary_lines()


def _letters(n, first=0):
    """n bytes no two neighbours of which are equal, so a byte a lane off is a wrong byte."""
    return bytes(65 + (first + k) % 26 + 32 * ((first + k) // 26 % 2) for k in range(n))


def lane_boundary_lines():
    """Accepted lines whose runs of bytes end around the 64 lanes a wavefront loads and stores with: the name, Z and
    H values, CIGAR ops, a QUAL shorter than SEQ, tabs at bytes 63, 64 and 65 of the line, and a 64th tag."""
    rng = np.random.default_rng(12)
    L = []
    for n in (63, 64, 65, 127, 128):
        L.append(sam_line(qname=_letters(n, n), tags=[b"NM:i:%d" % n]))
    for n in (63, 64, 65, 127, 128, 129):
        L.append(sam_line(tags=[b"XZ:Z:" + _letters(n, n), b"NM:i:1"]))
        L.append(sam_line(tags=[b"XH:H:" + bytes(b"0123456789ABCDEF"[(k * 7 + n) % 16] for k in range(n)), b"XA:A:e"]))
        L.append(sam_line(tags=[b"NM:i:300", b"XZ:Z:" + _letters(n, 3), b"XH:H:" + b"1A" * (n // 2) + b"F" * (n % 2)]))
    for n in (63, 64, 65, 128, 129):
        L.append(sam_line(cigar=b"".join(b"%d%c" % (1 + (k * 5 + n) % 300, b"MIDNSHP=X"[(k + n) % 9]) for k in range(n))))
    for n in (64, 65, 129):
        for short in (1, 64):
            L.append(sam_line(seq=_seq(n, rng), qual=bytes(33 + int(q) for q in rng.integers(0, 42, n - short)),
                              cigar=b"%dM" % n))
    # tab 1, 5 or 10 of the line at its byte 63, 64 or 65 (from 0): a longer name moves them there
    for tab in (1, 5, 10):
        before = len(b"\t".join(sam_line(qname=b"").split(b"\t")[:tab]))       # the tab's place under an empty name
        for at in (63, 64, 65):
            line = sam_line(qname=_letters(at - before, tab))
            assert [i for i, c in enumerate(line) if c == 9][tab - 1] == at
            L.append(line)
    L.append(sam_line(tags=[b"X%c:A:%c" % (48 + k % 10, 65 + k % 26) if k % 3 else b"Y%c:i:%d" % (97 + k % 26, k * 1021 - 30000)
                            for k in range(63)] + [b"NM:i:64"]))
    return L


def refused_lines():
    """[(line, encode_sam fails on it too)]: what the rule must refuse (status != 0, size 0)."""
    R = [(b"\t".join(sam_line().split(b"\t")[:10]), True), (b"", True), (b"r1", True)]
    R += [(sam_line(tags=[t]), True) for t in (b"XA", b"XA:i", b"XAi:5:", b"XA:i5", b"XQ:q:1", b"XB:B:", b"XB:B:q,1")]
    R += [(sam_line(tags=[t]), False) for t in (b"XF:f:0.5", b"XB:B:c,1,2", b"XB:B:f,1.5", b"NM:i:", b"NM:i:+5", b"NM:i:5x",
                                                b"NM:i:1234567890123456789")]
    R.append((sam_line() + b"\t", True))                                                # an empty 12th field
    R.append((sam_line(tags=[b"NM:i:1", b""]), True))
    for bad in (b"+5", b" 5", b"", b"1234567890", b"5 ", b"5x", b"-", b"0x10"):
        for field in ("flag", "pos", "mapq", "pnext", "tlen"):
            R.append((sam_line(**{field: bad}), False))
    R += [(sam_line(cigar=b"10Q"), True), (sam_line(cigar=b"10M5"), False), (sam_line(cigar=b"M"), False),
          (sam_line(cigar=b""), False), (sam_line(cigar=b"268435456M"), False), (sam_line(cigar=b"1234567890M"), False),
          (sam_line(cigar=b"1M" * 65536), False), (sam_line(cigar=b"10m"), True)]
    R += [(sam_line(qname=b"n" * 255), False), (sam_line(qname=b""), False)]
    return R


def bwa_lines(n, seed=5, read_len=100):
    """bwa-mem-shaped lines: reads of read_len bases, 5 tags, about 320 bytes at 100 bases (220 at 50)."""
    rng = np.random.default_rng(seed)
    R = read_len
    out = []
    for k in range(n):
        s = int(rng.integers(0, 3 * R // 5))
        cigar = b"%dM" % R if s < R // 5 else b"%dM%dS" % (R - s, s) if s < 2 * R // 5 else b"%dS%dM" % (s, R - s)
        chrom = NAMES[int(rng.integers(0, 5))]
        pos = int(rng.integers(1, 10 ** 8))
        tags = [b"NM:i:%d" % rng.integers(0, 4), b"MD:Z:%d" % (R - s), b"AS:i:%d" % (R - s), b"XS:i:%d" % rng.integers(0, 60),
                b"SA:Z:%s,%d,%s,%dS%dM,%d,0;" % (chrom, pos + 2000, b"+-"[k & 1:][:1], R - s, s or 1, rng.integers(0, 61))]
        out.append(sam_line(qname=b"SRR1000000.%d" % (k // 2), flag=b"%d" % rng.choice([0, 16, 65, 129, 2048, 2064, 83, 163]),
                            rname=chrom, pos=b"%d" % pos, mapq=b"%d" % rng.integers(0, 61), cigar=cigar,
                            rnext=rng.choice([b"=", b"*", b"chr2"]), pnext=b"%d" % rng.integers(0, 10 ** 8),
                            tlen=b"%d" % rng.integers(-500, 500), seq=_seq(R, rng),
                            qual=bytes(33 + int(q) for q in rng.integers(2, 42, R)), tags=tags))
    return out


def mutations(n, seed=77):
    """n seeded mutations of bwa-shaped lines: byte flips, field deletions, digits -> letters, duplicated tabs."""
    rng = np.random.default_rng(seed)
    base = bwa_lines(200, seed)
    out = []
    for k in range(n):
        line = bytearray(base[int(rng.integers(len(base)))])
        kind = k % 4
        if kind == 0:                                                                   # byte flips
            for _ in range(int(rng.integers(1, 4))):
                line[int(rng.integers(len(line)))] = int(rng.integers(256))
        elif kind == 1:                                                                 # a field deleted
            f = bytes(line).split(b"\t")
            del f[int(rng.integers(len(f)))]
            line = bytearray(b"\t".join(f))
        elif kind == 2:                                                                 # a digit becomes a letter
            digits = [i for i, c in enumerate(line) if 48 <= c <= 57]
            line[digits[int(rng.integers(len(digits)))]] = int(rng.choice(list(b"xMq+- ")))
        else:                                                                           # a tab twice
            tabs = [i for i, c in enumerate(line) if c == 9]
            at = tabs[int(rng.integers(len(tabs)))]
            line[at:at] = b"\t"
        out.append(bytes(line))
    return out
