"""Unspliced fragments of SAM text closed on the device (csrc/fc2_sam_frag_impl.h): the rule restated in Python, the
host twin's caller, the hand-built texts and the damaged generator-shaped lines, shared by the host, ingest and
device tests."""
import ctypes
import re

import numpy as np

from find_circ2_amd import _native as N
from sam_encode_helpers import NAMES, names_table, sam_line

HEAD = np.dtype([("flag", "<u4"), ("tid", "<i4"), ("l_name", "<u4"), ("state", "<u4")])
FRAG = np.dtype([("state", "u1"), ("n_records", "u1"), ("n_mates", "u1"), ("n_unmapped", "u1"), ("bytes", "<u4")])
assert HEAD.itemsize == 16 and FRAG.itemsize == 8
FRAG_CAP = 16                                           # FC2_BAM_FRAG_CAP
SEG = 1024                                              # FC2_SAM_GROUP_SEG
GUARD = 0xA5                                            # every byte of the outputs before a call
GUARD_ROWS = 8
TID_OF = {n: i for i, n in enumerate(NAMES)}            # (of a name listed twice the last index counts)


# ---- the rule, restated -------------------------------------------------------------------------------------

def py_head(line):
    """(flag, tid, l_name, 1) of a usable line, (0, 0, 0, 0) otherwise."""
    none = (0, 0, 0, 0)
    if line.endswith(b"\r"):
        return none
    f = line.split(b"\t")
    if len(f) < 11 or not 1 <= len(f[0]) <= 254:
        return none
    if not re.fullmatch(rb"[0-9]{1,5}", f[1]) or int(f[1]) > 65535:
        return none
    if f[5] != b"*" and not re.fullmatch(rb"[0-9MIDNSHP=X]*", f[5]):
        return none
    return (int(f[1]), -1 if f[2] == b"*" else TID_OF.get(f[2], -1), len(f[0]), 1)


def py_frag(k, heads, names, starts):
    """Line k's fragment row (state, n_records, n_mates, n_unmapped, bytes): fc2_bam_frag's five conditions."""
    none = (0, 0, 0, 0, 0)
    n = len(heads)
    flag, tid, _, ok = heads[k]
    if not ok or flag & 4:                              # 1.
        return none
    j, steps = k, 0                                     # 2.
    while True:
        if steps == 5 or j == 0:
            return none
        steps += 1
        j -= 1
        if not heads[j][3]:
            return none
        if heads[j][0] & 4:
            continue
        if names[j] == names[k]:
            return none
        break
    n_records, n_mates, n_unmapped, prim_flag, prim_ref = 1, 1, 0, flag, tid
    for j in range(k + 1, k + 2 + FRAG_CAP):            # 3. - 5.
        if j >= n or not heads[j][3]:
            return none
        rf, rt = heads[j][0], heads[j][1]
        if not rf & 4 and names[j] != names[k]:
            return (1, n_records, n_mates, n_unmapped, starts[j] - starts[k])
        n_records += 1
        if n_records > FRAG_CAP:
            return none
        if rf & 4:
            n_unmapped += 1
        elif rf & 0x40 == prim_flag & 0x40:
            if rt == prim_ref and rf & 0x10 == prim_flag & 0x10:
                return none
        else:
            if n_mates == 2:
                return none
            n_mates, prim_flag, prim_ref = 2, rf, rt
    return none


def py_rule(text):
    """(n_lines, starts, head rows, fragment rows) of a block of text, by the rule."""
    starts = [0] + [i + 1 for i, c in enumerate(text) if c == 10]
    n = len(starts) - 1
    lines = [text[starts[k]:starts[k + 1] - 1] for k in range(n)]
    heads = [py_head(l) for l in lines]
    names = [l[:h[2]] for l, h in zip(lines, heads)]
    return n, starts, heads, [py_frag(k, heads, names, starts) for k in range(n)]


# ---- the host twin ------------------------------------------------------------------------------------------

_table = None


def table():
    global _table
    if _table is None:
        _table = names_table()
    return _table


def outputs(cap):
    """(starts, head rows, fragment rows), cap (+ 1) entries and GUARD_ROWS more, every byte GUARD."""
    return (np.full(cap + 1 + GUARD_ROWS, GUARD * 0x01010101, np.uint32),
            np.frombuffer(bytes([GUARD]) * (16 * (cap + GUARD_ROWS)), HEAD).copy(),
            np.frombuffer(bytes([GUARD]) * (8 * (cap + GUARD_ROWS)), FRAG).copy())


def untouched(a, first):
    """Every byte of a[first:] still GUARD."""
    return bool((a[first:].view(np.uint8) == GUARD).all())


def check_guards(n, cap, starts, heads, frags):
    """What a call may write: starts[0 .. n] and n rows when n <= cap, nothing otherwise."""
    wrote = n <= cap
    assert untouched(starts, n + 1 if wrote else 0), "starts past the lines"
    assert untouched(heads, n if wrote else 0), "head rows past the lines"
    assert untouched(frags, n if wrote else 0), "fragment rows past the lines"


def group_host(text, cap=None):
    """fc2_sam_group_host on a block of text: (n_lines, starts, head rows, fragment rows), the arrays cut to the
    lines (empty when n_lines > cap), the guard rows after them checked."""
    n_want = text.count(b"\n")
    cap = n_want if cap is None else cap
    buf = np.frombuffer(text + b"\0", np.uint8).copy()
    starts, heads, frags = outputs(cap)
    n = ctypes.c_uint32(0xDEADBEEF)
    t = table()
    rc = N.lib().fc2_sam_group_host(buf.ctypes.data, len(text), t.ctypes.data, t.nbytes, starts.ctypes.data, heads.ctypes.data,
                                    frags.ctypes.data, ctypes.addressof(n), cap)
    assert rc == 0, N.lib().fc2_last_error()
    n = int(n.value)
    assert n == n_want
    check_guards(n, cap, starts, heads, frags)
    if n > cap:
        return n, starts[:0], heads[:0], frags[:0]
    return n, starts[:n + 1], heads[:n], frags[:n]


def same_as_rule(text):
    """The host twin's rows against the restated rule, row for row; returns the twin's."""
    n, starts, heads, frags = group_host(text)
    pn, pstarts, pheads, pfrags = py_rule(text)
    assert n == pn and list(starts) == pstarts
    assert [tuple(int(x) for x in h) for h in heads] == pheads
    assert [tuple(int(x) for x in f) for f in frags] == pfrags
    return n, starts, heads, frags


# ---- the read loop ------------------------------------------------------------------------------------------

def caller_run(path, sam_group=0, **opts):
    """group_inputs.caller_run over SAM text (a file, or '-' for stdin) with gpu_sam_group: what the loop handed out
    for evaluation (pair fields and read parts), the text streams, the counters or the error, the ingest's counts --
    then sam_group_counts()."""
    import group_inputs as G
    from find_circ2_amd.caller import CallerOptions
    from find_circ2_amd.native_caller import NativeCaller
    nc = NativeCaller(path, False, CallerOptions(**opts), G.NAMES, genome_dummy=True, gpu_sam_group=sam_group)
    nc.open()
    L = N.lib()
    out, texts, end = [], ["", "", ""], None
    try:
        try:
            while True:
                b, eof = N.CallerBatch(), ctypes.c_int(0)
                N.check(L.fc2_caller_next(nc.h, ctypes.byref(b), ctypes.byref(eof)))
                n = int(b.n)
                assert int(b.n_long) == 0
                if n:
                    pairs = np.frombuffer(ctypes.string_at(b.pairs, 16 * n), N.PAIR_DTYPE)
                    offs = np.frombuffer(ctypes.string_at(b.read_off, 8 * n), np.uint64)
                    reads = ctypes.string_at(b.reads, int((offs + pairs["read_len"]).max()))
                    out += [(pairs[k].tobytes(), reads[int(o):int(o) + int(pairs["read_len"][k])]) for k, o in enumerate(offs)]
                while L.fc2_caller_queued(nc.h) > 0:
                    res = np.zeros(max(n, 1), N.RESULT_DTYPE)
                    res["best_x"] = -1
                    N.check(L.fc2_caller_submit(nc.h, res.ctypes.data, None, 0, n))
                    for k in range(3):
                        texts[k] += nc._take(k)
                if eof.value:
                    break
            end = sorted(nc.counters().items())
        except N.Fc2Error as ex:
            end = ("error", str(ex))
        c = N.IngestCounts()                            # (after an error: the counts up to it)
        N.check(L.fc2_ingest_counts_get(L.fc2_caller_ingest(nc.h), ctypes.byref(c)))
        counts = tuple(int(getattr(c, f)) for f, _ in c._fields_)
        return (out, texts, end, counts), nc.sam_group_counts()
    finally:
        nc.close()


# ---- texts --------------------------------------------------------------------------------------------------

def ln(qname, flag=0, rname=b"chr1", **kw):
    return sam_line(qname=qname, flag=b"%d" % flag, rname=rname, **kw)


def un(qname=b"x"):
    return sam_line(qname=qname, flag=b"4", rname=b"*", pos=b"0", cigar=b"*")


def text_of(lines, newline=True):
    return b"\n".join(lines) + (b"\n" if newline and lines else b"")


def bad_lines():
    """[(what, line)]: every cause of an unusable line the rule names."""
    good = ln(b"bad")
    return [("9 tabs", b"\t".join(good.split(b"\t")[:10])), ("\\r\\n", good + b"\r"), ("blank", b""),
            ("FLAG 65536", ln(b"bad", 65536)), ("FLAG +4", sam_line(qname=b"bad", flag=b"+4")),
            ("FLAG ' 4'", sam_line(qname=b"bad", flag=b" 4")), ("FLAG 0x4", sam_line(qname=b"bad", flag=b"0x4")),
            ("FLAG empty", sam_line(qname=b"bad", flag=b"")), ("FLAG 000000", sam_line(qname=b"bad", flag=b"000000")),
            ("QNAME 0", ln(b"")), ("QNAME 255", ln(b"q" * 255)), ("CIGAR byte", ln(b"bad", cigar=b"5M1Q4M")),
            ("CIGAR lower case", ln(b"bad", cigar=b"10m")), ("tabs only", b"\t" * 11)]


def shapes():
    """[(what, the fragment's lines, whether its head's row must say state 1)]: every shape the rule tells apart.
    Each comes after a mapped line of another name and before one."""
    S = [("one mate", [ln(b"f")], True),
         ("two mates", [ln(b"f", 65), ln(b"f", 129)], True),
         ("two mates, the second unmapped", [ln(b"f", 65), sam_line(qname=b"f", flag=b"133", rname=b"*", cigar=b"*")], True),
         ("a segment elsewhere", [ln(b"f", 0, b"chr1"), ln(b"f", 2048, b"chr2")], True),
         ("a segment on the other strand", [ln(b"f", 0), ln(b"f", 2048 | 16)], True),
         ("a proper segment", [ln(b"f", 0), ln(b"f", 2048)], False),
         ("a proper segment of the second mate", [ln(b"f", 65), ln(b"f", 129, b"chr2"), ln(b"f", 129 | 2048, b"chr2")], False),
         ("a third mate", [ln(b"f", 65), ln(b"f", 129), ln(b"f", 65 | 256, b"chr3")], False),
         ("an unmapped head", [un(b"f")], False),
         ("QNAME of 254 bytes", [ln(b"q" * 254, 65), ln(b"q" * 254, 129)], True),
         ("a name that is a prefix of the next", [ln(b"lea")], True),
         ("RNAME *", [ln(b"f", 0, b"*"), ln(b"f", 2048, b"*")], False),           # -1 == -1: proper
         ("an unknown RNAME and *", [ln(b"f", 0, b"nowhere"), ln(b"f", 2048, b"*")], False),
         ("an unknown RNAME and a known one", [ln(b"f", 0, b"nowhere"), ln(b"f", 2048, b"chr1")], True),
         ("a name listed twice: its last index", [ln(b"f", 0, b"dup"), ln(b"f", 2048, b"dup")], False),
         ("CIGAR *", [ln(b"f", cigar=b"*")], True), ("an empty CIGAR", [ln(b"f", cigar=b"")], True),
         ("every CIGAR byte", [ln(b"f", cigar=b"0123456789MIDNSHP=X")], True),
         ("FLAG 65535", [ln(b"f", 65535 & ~4 & ~2048)], True), ("FLAG 00000", [sam_line(qname=b"f", flag=b"00000")], True),
         ("16 lines", [ln(b"f")] + [un()] * 15, True), ("17 lines", [ln(b"f")] + [un()] * 16, False)]
    S += [("%d unmapped lines before the head" % k, [un()] * k + [ln(b"f")], k <= 4) for k in range(6)]
    S += [("on the way forward: " + what, [ln(b"f", 65), bad, ln(b"f", 129)], False) for what, bad in bad_lines()]
    S += [("on the way back: " + what, [bad, ln(b"f")], False) for what, bad in bad_lines()]
    S += [("the closer: " + what, [ln(b"f"), bad], False) for what, bad in bad_lines()]
    return S


def shape_text(frag_lines):
    """A fragment between a mapped line of another name before it and one after it."""
    return text_of([ln(b"lead", 16, b"chr2")] + frag_lines + [ln(b"tail")])


def head_index(frag_lines):
    """The line number, in shape_text, of the fragment's first mapped usable line."""
    for k, l in enumerate(frag_lines):
        h = py_head(l)
        if h[3] and not h[0] & 4:
            return 1 + k
    return 1


def all_shapes_text():
    """Every shape in one block, each between mapped lines of other names."""
    lines = []
    for k, (_, frag, _) in enumerate(shapes()):
        lines += [ln(b"sep%d" % k, 16, b"chr2")] + frag
    return text_of(lines + [ln(b"tail")])


def reads_text(n_frags, seed, damage=0.0, newline=True):
    """Generator-shaped lines (scripts/gen_reads.c: bwa-mem's fields and tags, 100-base reads): unspliced
    fragments of one or two mates, some with a segment elsewhere or an unmapped line, among spliced ones (two
    proper segments); `damage` of the lines broken: a tab removed, a CIGAR byte changed, `\\r` appended or FLAG
    widened."""
    rng = np.random.default_rng(seed)
    seq = lambda: bytes(rng.choice(list(b"ACGT"), 100).astype(np.uint8))
    qual = lambda: bytes(rng.integers(35, 74, 100).astype(np.uint8))

    def mapped(qn, flag, chrom, cigar=b"100M"):
        return sam_line(qname=qn, flag=b"%d" % (flag | (16 if rng.random() < 0.4 else 0)), rname=chrom,
                        pos=b"%d" % rng.integers(1, 10 ** 8), mapq=b"60", cigar=cigar, rnext=b"=", pnext=b"%d" % rng.integers(1, 10 ** 8),
                        tlen=b"%d" % rng.integers(-500, 500), seq=seq(), qual=qual(),
                        tags=[b"NM:i:%d" % rng.integers(0, 4), b"MD:Z:100", b"AS:i:%d" % rng.integers(60, 101), b"XS:i:%d" % rng.integers(0, 60)])

    lines = []
    for k in range(n_frags):
        qn = b"SRR1000000.%d" % k
        chrom = NAMES[int(rng.integers(0, 3))]
        r = rng.random()
        if r < 0.4:                                     # spliced: two proper segments
            f = 0 if rng.random() < 0.5 else 16
            lines += [sam_line(qname=qn, flag=b"%d" % f, rname=chrom, cigar=b"60M40S", seq=seq(), qual=qual(), tags=[b"AS:i:60"]),
                      sam_line(qname=qn, flag=b"%d" % (f | 2048), rname=chrom, cigar=b"60H40M", seq=seq()[:40], qual=qual()[:40],
                               tags=[b"AS:i:40"])]
        elif r < 0.7:
            lines.append(mapped(qn, 0, chrom))
        else:
            lines += [mapped(qn, 65, chrom), mapped(qn, 129, chrom)]
            if rng.random() < 0.2:
                lines.append(mapped(qn, 65 | 256, b"chr3" if chrom != b"chr3" else b"chr1"))
        if rng.random() < 0.05:
            lines += [un(b"SRR1000000.u%d" % k)] * int(rng.integers(1, 7))
    if damage:
        for i in np.nonzero(rng.random(len(lines)) < damage)[0]:
            f = lines[i].split(b"\t")
            kind = int(rng.integers(0, 4))
            if kind == 0:
                j = int(rng.integers(0, len(f) - 1))
                f[j:j + 2] = [f[j] + f[j + 1]]
            elif kind == 1 and f[5] != b"*":
                f[5] = f[5][:-1] + b"Q"
            elif kind == 2:
                f[-1] += b"\r"
            else:
                f[1] = b"1" + f[1].rjust(5, b"0")
            lines[i] = b"\t".join(f)
    return text_of(lines, newline)
