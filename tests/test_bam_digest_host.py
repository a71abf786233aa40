"""fc2_bam_digest_host (include/fc2_ingest.h) -- one record's digest row, made from the ingest's own BAM
parser -- against an independent decoder written here (struct, and Python's own slices for the query
length), on hand-built records: every CIGAR shape the clips and spans depend on, AS and XS in each of the
eleven BAM tag types, and every malformation after which the host must parse the record itself (state 0).
Each record is placed at all four start residues mod 4.  The records (cases()) are also what the kernel's
test launches (test_gpu_bam_digest.py)."""
import ctypes
import functools
import struct

import numpy as np
import pytest

from find_circ2_amd import _native as N

ROW = np.dtype([("state", "u1"), ("as_type", "u1"), ("xs_type", "u1"), ("has_qual", "u1"), ("block_size", "<u4"),
                ("astart", "<i4"), ("qlen", "<i4"), ("as_bits", "<u4"), ("xs_bits", "<u4"), ("aend", "<i8")])
assert ROW.itemsize == 32 == ctypes.sizeof(N.BamDigest)

M, I, D, SKIP, S, H, P, EQ, X = range(9)          # CIGAR operation codes ("MIDNSHP=X")


# ---- the independent decoder ----------------------------------------------------------------------
def _tag_value(ty, v):
    """(size, bits) of an aux value of type ty at the head of v, None where the data is corrupt."""
    fixed = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
    if ty in fixed:
        n = struct.calcsize(fixed[ty])
        return (n, struct.unpack(fixed[ty], v[:n])[0] & 0xFFFFFFFF) if len(v) >= n else None
    if ty == "f":
        return (4, struct.unpack("<I", v[:4])[0]) if len(v) >= 4 else None
    if ty == "A":
        return (1, 0) if len(v) >= 1 else None
    if ty in "ZH":
        z = v.find(b"\0")
        return (z + 1, 0) if z >= 0 else None
    if ty == "B":
        if len(v) < 5:
            return None
        w = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}.get(chr(v[0]))
        cnt, = struct.unpack("<i", v[1:5])
        if w is None or cnt < 0 or 5 + w * cnt > len(v):
            return None
        return 5 + w * cnt, 0
    return None


def py_digest(d: bytes, n_bytes: int, at: int):
    """The digest row of the record start at byte `at` of d[:n_bytes], as a tuple in ROW's field order."""
    def zero(bs=0):
        return (0, 0, 0, 0, bs, 0, 0, 0, 0, 0)
    if at + 4 > n_bytes:
        return zero()
    bs, = struct.unpack_from("<I", d, at)
    if bs < 32 or bs >= 1 << 28 or at + 4 + bs > n_bytes:
        return zero(bs)
    b = d[at + 4:at + 4 + bs]
    _ref, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, 0)
    if l_seq < 0 or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return zero(bs)
    if l_name == 0 or b[32 + l_name - 1] != 0:
        return zero(bs)
    o = 32 + l_name
    ops = [(c & 0xF, c >> 4) for c in struct.unpack_from("<%dI" % n_cig, b, o)]
    o += 4 * n_cig
    ref_span = sum(ln for op, ln in ops if op in (M, D, SKIP, EQ, X))
    astart = 0
    for op, ln in ops:                              # the clips before the first M
        if op in (S, H):
            astart += ln
        elif op == M:
            break
    def soft(seq):                                  # soft clips at one end, hard clips skipped
        t = 0
        for op, ln in seq:
            if op == S:
                t += ln
            elif op != H:
                break
        return t
    lead, trail = soft(ops), soft(reversed(ops))
    if max(ref_span, astart, lead, trail) >= 1 << 31:
        return zero(bs)
    aend = -1 if (flag & 4) or not ops else pos + ref_span
    qlen = -1 if l_seq == 0 else len(range(l_seq)[lead:l_seq - trail])
    has_qual = int(not (l_seq == 0 or b[o + (l_seq + 1) // 2] == 0xFF))
    o += (l_seq + 1) // 2 + l_seq
    found = {"AS": [], "XS": []}
    while o < bs:
        if bs - o < 3:
            return zero(bs)
        tag, ty = b[o:o + 2].decode("latin-1"), chr(b[o + 2])
        o += 3
        v = _tag_value(ty, b[o:])
        if v is None:
            return zero(bs)
        if tag in found:
            found[tag].append((ord(ty), v[1]))
        o += v[0]
    if len(found["AS"]) > 1 or len(found["XS"]) > 1:
        return zero(bs)
    (as_ty, as_bits), (xs_ty, xs_bits) = [(found[t] or [(0, 0)])[0] for t in ("AS", "XS")]
    return (1, as_ty, xs_ty, has_qual, bs, astart, qlen, as_bits, xs_bits, aend)


def host_digest(buf: np.ndarray, n_bytes: int, at: int):
    """fc2_bam_digest_host at byte `at` of buf[:n_bytes] (a uint8 array), as a tuple in ROW's field order."""
    rows = np.full(3, 0xA5, np.uint8).repeat(32).view(ROW)
    N.check(N.lib().fc2_bam_digest_host(buf.ctypes.data, n_bytes, at,
                                        ctypes.cast(rows[1:].ctypes.data, ctypes.POINTER(N.BamDigest))))
    assert (rows[[0, 2]].view(np.uint8) == 0xA5).all(), "a neighbouring row was written"
    return tuple(int(x) for x in rows[1].item())


# ---- hand-built records ---------------------------------------------------------------------------
def rec(cigar=((M, 50),), l_seq=50, tags=b"NMC\x01", flag=0, pos=1000, name=b"read/1", nul=True, qual0=None,
        block_size=None, l_name=None):
    """One BAM record: block_size and body (block_size / l_read_name as given, if given)."""
    qn = name + (b"\0" if nul else b"x")
    cig = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
    seq = bytes([0x12, 0x48, 0x84, 0x21][k % 4] for k in range((l_seq + 1) // 2))
    qual = bytearray(30 + k % 10 for k in range(l_seq))
    if qual0 is not None and l_seq:
        qual[0] = qual0
    body = struct.pack("<iiBBHHHiiii", 1, pos, len(qn) if l_name is None else l_name, 60, 4681, len(cigar), flag, l_seq,
                       -1, -1, 0) + qn + cig + seq + bytes(qual) + tags
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def tag(name, ty, value=b""):
    return name + ty + value


@functools.lru_cache(maxsize=None)
def cases():
    """[(label, record bytes, state expected)]: state 1 where the row must hold the parser's fields."""
    C = []
    add = lambda label, r, state=1: C.append((label, r, state))  # noqa: E731
    # CIGAR shapes
    add("plain 50M", rec())
    add("H S lead, S H trail", rec(((H, 7), (S, 5), (M, 30), (S, 15), (H, 3))))
    add("no M", rec(((S, 10), (I, 30), (S, 10))))
    add("= X D N P I", rec(((EQ, 10), (X, 5), (D, 3), (SKIP, 400), (P, 2), (I, 4), (M, 31))))
    add("S after an I before the first M", rec(((S, 4), (I, 6), (S, 2), (M, 38))))
    add("no CIGAR", rec((), tags=b""))
    add("unmapped flag with a CIGAR", rec(((S, 5), (M, 45)), flag=4))
    add("clips longer than SEQ: empty slice", rec(((S, 60), (M, 5), (S, 10)), l_seq=50))
    add("clips longer than SEQ: negative end", rec(((S, 3), (M, 5), (S, 70)), l_seq=50))
    add("trailing clip over twice SEQ", rec(((M, 5), (S, 120)), l_seq=50))
    add("l_seq 0", rec(((M, 20),), l_seq=0))
    add("l_seq 0, no CIGAR, no tags", rec((), l_seq=0, tags=b""))
    add("odd l_seq", rec(((S, 1), (M, 30), (S, 2)), l_seq=33))
    add("QUAL 0xFF", rec(qual0=0xFF))
    add("QUAL 0", rec(qual0=0))
    add("negative pos", rec(pos=-1))
    add("long name", rec(name=b"q" * 253))
    add("255-byte name field", rec(name=b"q" * 254))
    add("ref_span 2^31 - 1", rec(((SKIP, (1 << 28) - 1),) * 8 + ((M, 7),)))
    add("ref_span 2^31", rec(((SKIP, (1 << 28) - 1),) * 8 + ((M, 8),)), 0)
    add("leading soft clips 2^31", rec(((S, (1 << 28) - 1),) * 8 + ((S, 8), (M, 9))), 0)
    add("trailing soft clips 2^31", rec(((M, 9),) + ((S, (1 << 28) - 1),) * 8 + ((S, 8),)), 0)
    add("aligned start 2^31 through H", rec(((H, (1 << 28) - 1),) * 8 + ((H, 8), (M, 9))), 0)
    # AS and XS in each of the eleven types, alone and together
    vals = {"c": [b"\x80", b"\x7f", b"\xff"], "C": [b"\xff", b"\x00"], "s": [b"\x00\x80", b"\xff\x7f"],
            "S": [b"\xff\xff", b"\x01\x00"], "i": [b"\x00\x00\x00\x80", b"\xff\xff\xff\x7f"],
            "I": [b"\xff\xff\xff\xff", b"\x00\x00\x00\x80"],
            "f": [struct.pack("<f", -36.5), struct.pack("<f", 0.1), b"\x01\x00\xa0\x7f"],   # (the last: a signalling NaN)
            "A": [b"x"], "Z": [b"text\0", b"\0"], "H": [b"1AE301\0"],
            "B": [b"c\x03\x00\x00\x00\x01\x02\x03", b"S\x02\x00\x00\x00\x01\x00\x02\x00", b"f\x00\x00\x00\x00"]}
    assert len(vals) == 11
    for ty, vs in vals.items():
        for k, v in enumerate(vs):
            t = ty.encode()
            add("AS:%s #%d" % (ty, k), rec(tags=b"NMC\x01" + tag(b"AS", t, v) + b"MDZ50\0"))
            add("XS:%s #%d" % (ty, k), rec(tags=tag(b"XS", t, v)))
            add("AS:i with XS:%s #%d" % (ty, k), rec(tags=tag(b"AS", b"i", b"\x2a\0\0\0") + tag(b"XS", t, v) + b"XAA!"))
    add("tags named As, SA and X S are not AS / XS", rec(tags=b"AsC\x05SAZchr1,5,+,50M,60,0;\0XsC\x06"))
    add("duplicated AS", rec(tags=b"ASC\x30NMC\x01ASC\x31"), 0)
    add("duplicated XS", rec(tags=b"XSC\x30XSf\0\0\x80\x3f"), 0)
    add("duplicated AS behind one XS", rec(tags=b"XSC\x30ASC\x05ASC\x05"), 0)
    # corruption
    add("unknown tag type", rec(tags=b"NMC\x01XX?\x01"), 0)
    add("Z without a NUL", rec(tags=b"NMC\x01MDZ50"), 0)
    add("H without a NUL", rec(tags=b"XHH1AE3"), 0)
    add("empty Z at the very end, no NUL", rec(tags=b"MDZ"), 0)
    add("B with a bad subtype", rec(tags=b"XBBd\x01\0\0\0\0\0\0\0"), 0)
    add("B with a negative count", rec(tags=b"XBBc\xff\xff\xff\xff"), 0)
    add("B count past the end", rec(tags=b"XBBi\x03\0\0\0" + b"\0" * 11), 0)
    add("B header cut short", rec(tags=b"XBBi\x03\0"), 0)
    add("value running past the end", rec(tags=b"NMC\x01ASi\x01\x02"), 0)
    add("s value running past the end", rec(tags=b"ASs\x01"), 0)
    add("1 trailing byte", rec(tags=b"NMC\x01A"), 0)
    add("2 trailing bytes", rec(tags=b"NMC\x01AS"), 0)
    add("3 trailing bytes: a tag without its value", rec(tags=b"NMC\x01ASC"), 0)
    add("l_read_name 0", rec(name=b"", nul=True, l_name=0), 0)
    add("name without a NUL", rec(nul=False), 0)
    good = rec()
    add("fields exceed block_size", good[:4] + good[4:20] + struct.pack("<i", 5000) + good[24:], 0)
    add("negative l_seq", good[:4] + good[4:20] + struct.pack("<i", -1) + good[24:], 0)
    add("n_cigar_op exceeds block_size", good[:16] + struct.pack("<H", 60000) + good[18:], 0)
    add("block_size 31", struct.pack("<I", 31) + good[4:35], 0)
    add("block_size 2^28", struct.pack("<I", 1 << 28) + good[4:], 0)
    add("block_size 0xFFFFFFFF", struct.pack("<I", 0xFFFFFFFF) + good[4:], 0)
    add("block_size 32, nothing but fixed fields", struct.pack("<I", 32) + good[4:36], 0)    # (l_read_name 7 > 0 bytes left)
    return C


def placed(r: bytes, residue: int, tail: int = 9):
    """r behind `residue` + 4 bytes of other data and in front of `tail` more: (buffer, at)."""
    lead = bytes([0xEE] * (4 + residue))
    return np.frombuffer(lead + r + bytes([0x11] * tail), np.uint8).copy(), len(lead)


# ---- tests ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_hand_built_records(residue):
    seen = set()
    for label, r, state in cases():
        buf, at = placed(r, residue)
        want = py_digest(buf.tobytes(), len(buf), at)
        got = host_digest(buf, len(buf), at)
        assert got == want, (label, got, want)
        assert got[0] == state, (label, got)
        assert got[4] == struct.unpack_from("<I", r)[0], label
        if not state:
            assert got[:4] == (0, 0, 0, 0) and got[5:] == (0, 0, 0, 0, 0), (label, got)
        seen.add(got[0])
    assert seen == {0, 1}


def test_expected_values_by_hand():
    """A few rows spelled out, so that the two decoders cannot agree on a shared mistake."""
    want = {
        "H S lead, S H trail": (1, 0, 0, 1, None, 12, 30, 0, 0, 1030),
        "no M": (1, 0, 0, 1, None, 20, 30, 0, 0, 1000),
        "= X D N P I": (1, 0, 0, 1, None, 0, 50, 0, 0, 1000 + 10 + 5 + 3 + 400 + 31),
        "S after an I before the first M": (1, 0, 0, 1, None, 6, 46, 0, 0, 1038),
        "no CIGAR": (1, 0, 0, 1, None, 0, 50, 0, 0, -1),
        "unmapped flag with a CIGAR": (1, 0, 0, 1, None, 5, 45, 0, 0, -1),
        "clips longer than SEQ: empty slice": (1, 0, 0, 1, None, 60, 0, 0, 0, 1005),
        "clips longer than SEQ: negative end": (1, 0, 0, 1, None, 3, 27, 0, 0, 1005),    # seq[3:-20]
        "trailing clip over twice SEQ": (1, 0, 0, 1, None, 0, 0, 0, 0, 1005),            # seq[0:-70] -> seq[0:0]
        "l_seq 0": (1, 0, 0, 0, None, 0, -1, 0, 0, 1020),
        "QUAL 0xFF": (1, 0, 0, 0, None, 0, 50, 0, 0, 1050),
        "AS:c #0": (1, ord("c"), 0, 1, None, 0, 50, 0xFFFFFF80, 0, 1050),
        "AS:s #0": (1, ord("s"), 0, 1, None, 0, 50, 0xFFFF8000, 0, 1050),
        "XS:S #0": (1, 0, ord("S"), 1, None, 0, 50, 0, 0xFFFF, 1050),
        "XS:I #0": (1, 0, ord("I"), 1, None, 0, 50, 0, 0xFFFFFFFF, 1050),
        "AS:i with XS:f #0": (1, ord("i"), ord("f"), 1, None, 0, 50, 42, struct.unpack("<I", struct.pack("<f", -36.5))[0], 1050),
        "AS:i with XS:Z #0": (1, ord("i"), ord("Z"), 1, None, 0, 50, 42, 0, 1050),
        "XS:B #1": (1, 0, ord("B"), 1, None, 0, 50, 0, 0, 1050),
        "ref_span 2^31 - 1": (1, 0, 0, 1, None, 0, 50, 0, 0, 1000 + (1 << 31) - 1),
    }
    by_label = {label: r for label, r, _ in cases()}
    for label, w in want.items():
        buf, at = placed(by_label[label], 1)
        got = host_digest(buf, len(buf), at)
        assert got[:4] + got[5:] == w[:4] + w[5:], (label, got)


@pytest.mark.parametrize("residue", [0, 3])
def test_record_ends_at_and_past_the_bytes(residue):
    r = rec(tags=b"ASC\x30XSC\x10")
    buf, at = placed(r, residue, tail=0)
    n = len(buf)
    whole = host_digest(buf, n, at)
    assert whole == py_digest(buf.tobytes(), n, at) and whole[0] == 1      # ends exactly at n_bytes
    big = np.concatenate([buf, np.zeros(8, np.uint8)])                     # (readable, but not the record's)
    for cut in (1, 2, 40, len(r) - 4):
        got = host_digest(big, n - cut, at)
        assert got == (0, 0, 0, 0, len(r) - 4, 0, 0, 0, 0, 0), (cut, got)
        assert got == py_digest(big.tobytes(), n - cut, at)
    for k in (1, 2, 3):                                                    # not even a whole block_size
        assert host_digest(big, at + k, at) == (0,) * 10
    assert host_digest(big, at, at) == (0,) * 10


def test_arguments():
    L = N.lib()
    row = N.BamDigest()
    buf = np.zeros(64, np.uint8)
    assert L.fc2_bam_digest_host(None, 4, 0, ctypes.byref(row)) == N.FC2_E_PARAM
    assert L.fc2_bam_digest_host(buf.ctypes.data, 64, 0, None) == N.FC2_E_PARAM
    assert L.fc2_bam_digest_host(buf.ctypes.data, 64, 65, ctypes.byref(row)) == N.FC2_E_RANGE
    assert L.fc2_bam_digest_host(None, 0, 0, ctypes.byref(row)) == 0 and row.state == 0
    assert L.fc2_bam_digest_launch(None, 0, None, None, None, None, None, None, None, 0, None) == 0
    assert L.fc2_bam_digest_launch(None, 4, None, None, None, None, None, None, None, 3, None) == N.FC2_E_PARAM
    p = ctypes.c_void_p(64)
    assert L.fc2_bam_digest_launch(p, 4, p, p, None, p, p, p, p, N.BAM_DIGEST_MAX_BLOCKS + 1, None) == N.FC2_E_PARAM
    assert L.fc2_ingest_set_gpu_digest(None, 1) == N.FC2_E_PARAM
    assert L.fc2_ingest_digest_counts(None, None, None) == N.FC2_E_PARAM


def test_ingest_switch_without_a_gpu(tmp_path):
    """set_gpu_digest on an ingest with no GPU inflate changes nothing: the same fragments, no counts."""
    from find_circ2_amd.ingest import NativeIngest
    from samgen import sam_to_bam
    from test_native_caller import _rich_sam
    sam, bam = str(tmp_path / "r.sam"), str(tmp_path / "r.bam")
    _rich_sam(sam, 60, seed=11)
    sam_to_bam(open(sam).read(), bam)
    res = []
    for on in (None, True, False):
        ing = NativeIngest(bam, True)
        if on is not None:
            ing.set_gpu_digest(on)
        frags = []
        while not ing.eof:
            frags += [[(r.qname, r.flag, r.pos, str(r.cigar), str(r.tags)) for r in f] for f in ing.next_chunk(13, False, False, 50)]
        assert ing.digest_counts() == (0, 0)
        ing.close()
        res.append(frags)
    assert res[0] and res[0] == res[1] == res[2]
