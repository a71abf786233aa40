"""BAM records from SAM text, the rule on the host (csrc/fc2_sam_encode_impl.h through fc2_sam_encode_host) against
the yardstick, the -B encoder itself (fc2_sam_encode_line over encode_sam), line by line: every form the rule
must accept gives the yardstick's bytes, every form it must refuse a non-zero status and no bytes, and under
20,000 seeded mutations of bwa-shaped lines no accepted line has a byte that is not the yardstick's.  On the
unmutated lines of the golden SAM, the rich SAM and the generator's SAM nothing is refused.  A stand-alone
program runs the rule and the writer's stand-in mode under ASan and UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from find_circ2_amd import _native as N
from sam_encode_helpers import (CANARY, E_FORMAT, E_PARAM, MAX_LINES, NAMES, bound, bwa_lines, check_contract, encode_host,
                                encode_host_all, encode_line, mutations, names_table, pack, planted_lines, refused_lines,
                                sam_line)


def test_planted_lines_are_the_yardsticks_bytes():
    lines = planted_lines()
    st, recs = encode_host_all(lines)
    for i, line in enumerate(lines):
        rc, want, msg = encode_line(line)
        assert rc == 0, (i, line[:100], msg)
        assert st[i] == 0, (i, line[:100], st[i])
        assert recs[i] == want, (i, line[:100])


def test_names_follow_the_header_map():
    """A known name, an unknown one, `*`, `=`, and a name twice in the header: the last index."""
    import struct
    _, recs = encode_host_all([sam_line(rname=b"chr2", rnext=b"="), sam_line(rname=b"dup", rnext=b"chrX"),
                               sam_line(rname=b"nowhere", rnext=b"*"), sam_line(rname=b"*", rnext=b"chr1")])
    ids = [(struct.unpack_from("<i", r, 4)[0], struct.unpack_from("<i", r, 24)[0]) for r in recs]
    assert ids == [(1, 1), (5, 2), (-1, -1), (-1, 0)]
    # no names at all, and an empty name
    st, recs = encode_host_all([sam_line(rname=b"chr1"), sam_line(rname=b"")], names=[])
    assert st == [0, 0] and [struct.unpack_from("<i", r, 4)[0] for r in recs] == [-1, -1]
    assert check_contract([sam_line(rname=b""), sam_line(rname=b"a")], names=[b"a", b"", b"a"]) == [0, 0]


def test_refused_lines_get_a_status_and_no_bytes():
    cases = refused_lines()
    lines = [c[0] for c in cases]
    st, recs = encode_host_all(lines)
    for i, (line, host_fails) in enumerate(cases):
        assert st[i] != 0 and recs[i] is None, (i, line[:100])
        rc, _, msg = encode_line(line)
        assert (rc != 0) == host_fails, (i, line[:100], msg)
        if host_fails:
            assert rc == E_FORMAT and msg.startswith("ValueError: "), (i, msg)
    # between accepted lines a refused one takes no room
    status, size, out_off, total, out = encode_host([sam_line(), lines[0], sam_line(qname=b"second")])
    assert list(status != 0) == [False, True, False] and size[1] == 0 and out_off[1] == out_off[2] == size[0]
    assert out[:total].tobytes() == encode_line(sam_line())[1] + encode_line(sam_line(qname=b"second"))[1]


def test_contract_under_mutation():
    lines = mutations(20000)
    st = check_contract(lines)
    accepted = sum(s == 0 for s in st)
    assert 2000 < accepted < 19000, accepted      # both sides of the contract are exercised
    # a refused line is either one the yardstick fails on or one it is laxer on: both occur
    fails = sum(encode_line(l)[0] != 0 for l, s in zip(lines[:4000], st[:4000]) if s)
    assert 0 < fails < sum(s != 0 for s in st[:4000])


def _sam_lines(path_or_text):
    text = open(path_or_text, "rb").read() if isinstance(path_or_text, str) else path_or_text
    return [l for l in text.split(b"\n") if l and not l.startswith(b"@")], \
        [l.split(b"\tSN:")[1].split(b"\t")[0] for l in text.split(b"\n") if l.startswith(b"@SQ")]


def test_nothing_is_refused_on_unmutated_input(tmp_path):
    from bwa_emul import read_fasta
    from samgen import sam_text
    from test_cli import _reads
    from test_native_caller import _rich_sam
    rich = str(tmp_path / "rich.sam")
    _rich_sam(rich, 1500, seed=31)
    fa = os.path.join(GOLDEN, "test_ref.fa")
    gen = sam_text(read_fasta(fa), _reads(os.path.join(GOLDEN, "test_reads.fa"))).encode()
    for src in (os.path.join(GOLDEN, "test_norm.sam"), rich, gen):
        lines, names = _sam_lines(src)
        assert lines
        st = check_contract(lines, names)
        assert not any(st), [(i, s) for i, s in enumerate(st) if s][:5]
    assert not any(check_contract(bwa_lines(500)))


def test_batch_shapes_and_the_canary():
    base = bwa_lines(70)
    for n in (1, 2, 63, 64, 65):
        status, size, out_off, total, out = encode_host(base[:n])
        assert not status.any() and total == size.sum() and (out[total:] == CANARY).all()
        assert list(out_off) == [0] + list(np.cumsum(size))
        assert out[:total].tobytes() == b"".join(encode_line(l)[1] for l in base[:n])
    # a 40,000-base line alone and between short ones
    rng = np.random.default_rng(3)
    long = sam_line(seq=bytes(rng.choice(list(b"ACGTN"), 40000).astype(np.uint8)),
                    qual=bytes(rng.integers(33, 74, 40000).astype(np.uint8)), cigar=b"20000M5000N20000M",
                    tags=[b"MD:Z:" + b"7A" * 3000])
    for lines in ([long], [base[0], long, base[1]]):
        status, size, out_off, total, out = encode_host(lines)
        assert not status.any() and out[:total].tobytes() == b"".join(encode_line(l)[1] for l in lines)
        assert (out[total:] == CANARY).all()


def test_the_bound_holds_and_is_tight_enough():
    """2 * line + 40: never passed on the planted lines, and reached to within 4 bytes by a line of 1-byte fields."""
    for line in planted_lines():
        rc, rec, _ = encode_line(line)
        assert len(rec) <= bound(len(line), 1)
    worst = sam_line(qname=b"q", flag=b"0", rname=b"*", pos=b"0", mapq=b"0", cigar=b"1M" * 50, rnext=b"*", pnext=b"0",
                     tlen=b"0", seq=b"A" * 50, qual=b"*")
    assert check_contract([worst]) == [0]
    assert bound(len(worst), 1) - len(encode_line(worst)[1]) < 80


def test_entries_refuse_what_is_not_a_batch():
    L = N.lib()
    text, off = pack([sam_line(), sam_line()])
    table = names_table()
    n, nb = 2, int(off[-1])
    out = np.full(bound(nb, n), CANARY, np.uint8)
    st, sz, oo, tot = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32), ctypes.c_uint32(5)

    def call(text_p=text.ctypes.data, nb_=nb, off_p=off.ctypes.data, n_=n, tab_p=table.ctypes.data, tb=table.nbytes,
             out_p=out.ctypes.data, cap=out.nbytes):
        return L.fc2_sam_encode_host(text_p, nb_, off_p, n_, tab_p, tb, out_p, cap, oo.ctypes.data, sz.ctypes.data,
                                     st.ctypes.data, ctypes.addressof(tot))
    assert call() == 0 and tot.value == sz.sum() > 0
    for kw in (dict(text_p=None), dict(off_p=None), dict(tab_p=None), dict(out_p=None), dict(n_=0), dict(n_=MAX_LINES + 1),
               dict(nb_=(4 << 20) + 1), dict(tb=4), dict(tb=table.nbytes - 4), dict(cap=bound(nb, n) - 1)):
        tot.value = 5
        assert call(**kw) == E_PARAM, kw
        assert tot.value == 0
    # the same checks in front of the launch (no device is touched)
    assert L.fc2_sam_encode_launch(text.ctypes.data, nb, off.ctypes.data, 0, table.ctypes.data, table.nbytes, out.ctypes.data,
                                   out.nbytes, oo.ctypes.data, sz.ctypes.data, st.ctypes.data, ctypes.addressof(tot), None) == E_PARAM
    assert L.fc2_sam_encode_launch(text.ctypes.data, nb, off.ctypes.data, n, table.ctypes.data, table.nbytes, out.ctypes.data,
                                   out.nbytes - 1, oo.ctypes.data, sz.ctypes.data, st.ctypes.data, ctypes.addressof(tot), None) == E_PARAM
    # offsets that are not lines of the text: refused line by line, nothing read outside the text
    bad = off.copy()
    bad[1] = nb + 7
    assert L.fc2_sam_encode_host(text.ctypes.data, nb, bad.ctypes.data, n, table.ctypes.data, table.nbytes, out.ctypes.data,
                                 out.nbytes, oo.ctypes.data, sz.ctypes.data, st.ctypes.data, ctypes.addressof(tot)) == 0
    assert list(st) == [7, 7] and tot.value == 0
    need = ctypes.c_uint64()
    assert L.fc2_sam_names_table(None, None, 1, None, 0, ctypes.byref(need)) == E_PARAM
    small = np.zeros(2, np.uint32)
    from sam_encode_helpers import c_names
    assert L.fc2_sam_names_table(c_names(NAMES), None, len(NAMES), small.ctypes.data, 8, ctypes.byref(need)) == -4
    n_out = ctypes.c_uint64()
    assert L.fc2_sam_encode_line(None, 5, c_names(NAMES), len(NAMES), None, 0, ctypes.byref(n_out)) == E_PARAM
    assert L.fc2_sam_encode_line(sam_line(), len(sam_line()), c_names(NAMES), len(NAMES), None, 0, ctypes.byref(n_out)) == -4
    assert n_out.value == len(encode_line(sam_line())[1])
    assert L.fc2_gpu_sam_encode_bound(1000, 3) == bound(1000, 3)


def test_sam_encode_host_code_under_sanitizers(tmp_path):
    """tests/c/sam_encode_main.cpp: the rule over the planted lines and a slice of the mutations into buffers of
    exactly the bound, and the writer's stand-in mode (csrc/fc2_bamout.cpp and fc2_bamout_sam.cpp compiled into
    the program), for the host with ASan and UBSan."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    lines = planted_lines() + [c[0] for c in refused_lines()] + mutations(3000)
    data = str(tmp_path / "lines.bin")
    with open(data, "wb") as f:
        for l in lines:
            f.write(len(l).to_bytes(4, "little") + l)
    exe = str(tmp_path / "sam_encode_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "c", "sam_encode_main.cpp"), "-lz"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0 and (b"asan" in r.stdout.lower() or b"ubsan" in r.stdout.lower() or b"sanitize" in r.stdout.lower()):
        pytest.skip("the sanitizer runtime is absent")
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    r = subprocess.run([exe, data, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert b"ok" in r.stdout
