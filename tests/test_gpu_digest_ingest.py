"""The parse threads taking a record's derived fields from the device's digest rows
(fc2_ingest_set_gpu_digest; csrc/fc2_ingest.cpp sam_parse_loop, parse_bam_body's fast path) for the BGZF
blocks the GPU inflates: the native read loop hands out the same pairs, read parts and counters with
digests on, with them off and with the CPU inflating -- on the rich bwa-mem-shaped BAM in 3 kB blocks
(records cross BGZF blocks constantly) at batch sizes that put the chunk and batch edges everywhere, with
a corrupt aux field planted mid-file (the same error after the same fragments), on the reference's own
bwa-mem records (tests/golden/test_norm.sam), and through the command line, whose files are the same bytes
whatever FC2_GPU_DIGEST says."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = ["chr1", "chr2", "chr3"]


def _caller_run(path, names, gpu, digest=None):
    """The native read loop (fc2_caller_next, every result "no breakpoint") over a BAM, the CPU inflating
    or GPU 0 from the first batch it can take, digest rows as `digest` says (None: the default): what it
    handed out for evaluation (pair fields and read parts), the text streams, the counters -- or, in their
    place from the failing call on, the error -- then inflate_counts() and digest_counts()."""
    from find_circ2_amd import _native as N
    from find_circ2_amd.caller import CallerOptions
    from find_circ2_amd.native_caller import NativeCaller
    nc = NativeCaller(path, True, CallerOptions(), names, genome_dummy=True)
    nc.open()
    L = N.lib()
    out, texts, end = [], ["", "", ""], None
    try:
        if gpu:
            ing = L.fc2_caller_ingest(nc.h)
            N.check(L.fc2_ingest_set_gpu_inflate(ing, 0, 1))
            if digest is not None:
                N.check(L.fc2_ingest_set_gpu_digest(ing, int(digest)))
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
        return (out, texts, end), nc.inflate_counts(), nc.digest_counts()
    finally:
        nc.close()


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    """The rich input as a BGZF BAM of 3 kB blocks, over 1,300 of them (a batch of 1024 blocks leaves
    the GPU some), and the same with one record's aux data corrupt mid-file; with what the CPU inflate
    reads from each."""
    from samgen import bgzf_compress, sam_to_bam
    from test_native_caller import _rich_sam
    d = tmp_path_factory.mktemp("digest_ingest")
    sam, raw = str(d / "rich.sam"), str(d / "raw.bam")
    _rich_sam(sam, 9000, seed=4242)
    sam_to_bam(open(sam).read(), raw, compress="none")
    data = bytearray(open(raw, "rb").read())
    bam = str(d / "rich.bam")
    open(bam, "wb").write(bgzf_compress(bytes(data), block=3000, level=1))
    assert len(data) > 1300 * 3000
    # the record in the middle of the file: its first tag's type made one BAM does not know
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        o += 8 + l_name
    while o < len(data) // 2:
        o += 4 + struct.unpack_from("<i", data, o)[0]
    bs, _, _, l_name, _, _, n_cig, _, l_seq = struct.unpack_from("<iiiBBHHHi", data, o)
    t = o + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    assert t + 3 <= o + 4 + bs, "the record has tags"
    data[t + 2] = ord("?")
    bad = str(d / "bad_aux.bam")
    open(bad, "wb").write(bgzf_compress(bytes(data), block=3000, level=1))
    cpu, cpu_bad = _caller_run(bam, NAMES, False), _caller_run(bad, NAMES, False)
    assert cpu[1:] == ((0, 0), (0, 0)) and len(cpu[0][0]) > 3000
    assert cpu_bad[0][2][0] == "error" and "corrupted aux data" in cpu_bad[0][2][1], cpu_bad[0][2]
    assert 1000 < len(cpu_bad[0][0]) < len(cpu[0][0])
    return bam, cpu[0], bad, cpu_bad[0]


@pytest.mark.parametrize("batch", ["1", "3", "1024"])
def test_digest_rows_give_the_cpu_inflates_fragments(rich, monkeypatch, batch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    monkeypatch.setenv("FC2_PARSE_BLOCK", "7000")
    bam, cpu, _, _ = rich
    on, on_inf, on_dig = _caller_run(bam, NAMES, True, True)
    assert on == cpu
    off, off_inf, off_dig = _caller_run(bam, NAMES, True, False)
    assert off == cpu
    dflt, dflt_inf, dflt_dig = _caller_run(bam, NAMES, True)
    assert dflt == cpu
    assert on_inf == off_inf == dflt_inf and on_inf[0] > 200 and on_inf[1] == 0, (on_inf, off_inf)
    # the same records counted either way; with digests on most take their row (a record that runs out
    # of its chunk -- with a batch of one block, out of its block -- does not), with them off none
    assert off_dig[0] == 0 and off_dig[1] > 0 and off_dig == dflt_dig, (off_dig, dflt_dig)
    assert on_dig[0] + on_dig[1] == off_dig[1], (on_dig, off_dig)
    assert on_dig[0] > (0.5 if batch == "1" else 0.9) * off_dig[1], (on_dig, off_dig)


@pytest.mark.parametrize("batch", ["3", "1024"])
def test_corrupt_aux_field_is_the_hosts_error(rich, monkeypatch, batch):
    """The record with the corrupt aux field gets a row with state 0, so the host parses it and raises
    what the CPU path raises, after the same fragments."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    _, _, bad, cpu = rich
    on, on_inf, on_dig = _caller_run(bad, NAMES, True, True)
    assert on == cpu, (on[2], cpu[2])
    off, _, off_dig = _caller_run(bad, NAMES, True, False)
    assert off == cpu
    if batch == "3":
        assert on_dig[0] > 0 and off_dig[0] == 0


def test_text_hand_back_parses_on_the_host(rich, monkeypatch):
    """fc2_ingest_next wants SAM text of every record: no row is used, the fragments are the CPU's."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from find_circ2_amd.ingest import NativeIngest
    monkeypatch.setenv("FC2_BGZF_BATCH", "64")
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    res = []
    for gpu in (False, True):
        ing = NativeIngest(rich[0], True)
        if gpu:
            ing.set_gpu_inflate(0)
            ing.set_gpu_digest(True)
        frags = []
        while not ing.eof:
            frags += [[(r.qname, r.flag, r.tid, r.pos, str(r.cigar), r.seq, r.qual, str(r.tags)) for r in f]
                      for f in ing.next_chunk(13, False, False, 500)]
        c = ing.counts
        res.append((frags, tuple(getattr(c, f) for f, _ in c._fields_), ing.inflate_counts()[0] > 0, ing.digest_counts()[0]))
        ing.close()
    assert res[0][:2] == res[1][:2] and len(res[0][0]) > 3000
    assert res[1][2:] == (True, 0)


def test_norm_sam_records_through_the_digest_path(tmp_path, monkeypatch):
    """The reference's own bwa-mem records (tests/golden/test_norm.sam) as a BAM of 150-byte BGZF blocks,
    batches of four: the pairs of test_norm_sam.py's hand-derived table, with rows from the device."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from samgen import bgzf_compress, sam_to_bam
    from test_norm_sam import EXPECTED, NORM, _primary_seqs
    from find_circ2_amd import _native as N
    raw, bam = str(tmp_path / "raw.bam"), str(tmp_path / "norm_small.bam")
    sam_to_bam(open(NORM).read(), raw, compress="none")
    open(bam, "wb").write(bgzf_compress(open(raw, "rb").read(), block=150, level=6))
    monkeypatch.setenv("FC2_BGZF_BATCH", "4")
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    cpu, _, _ = _caller_run(bam, ["chr22"], False)
    on, on_inf, on_dig = _caller_run(bam, ["chr22"], True, True)
    assert on == cpu
    assert on_inf[0] > 0 and on_dig[0] >= 1 and on_dig[0] + on_dig[1] <= 6, (on_inf, on_dig)
    assert len(on[0]) == 3
    for (p, part), exp, seq in zip(on[0], EXPECTED, _primary_seqs()):
        p = np.frombuffer(p, N.PAIR_DTYPE)[0]
        assert (int(p["a_pos"]), int(p["b_aend"]), int(p["chrom"])) == (exp["a_pos"], exp["b_aend"], 0)
        assert part.decode() == seq[exp["q_start"]:exp["q_end"]]
    assert dict(on[2])["total_mates"] == 3


_CLI = """
import sys
sys.path[:0] = [%r]
from find_circ2_amd import cli
sys.exit(cli.main(sys.argv[1:]))
"""


@pytest.fixture(scope="module")
def cli_input(tmp_path_factory):
    from samgen import bgzf_compress, sam_to_bam
    from test_native_caller import _rich_sam
    d = tmp_path_factory.mktemp("digest_cli")
    sam, raw, bam = str(d / "rich.sam"), str(d / "raw.bam"), str(d / "small.bam")
    fa = _rich_sam(sam, 4000, seed=7)
    sam_to_bam(open(sam).read(), raw, compress="none")
    open(bam, "wb").write(bgzf_compress(open(raw, "rb").read(), block=3000, level=6))
    return fa, bam, d, {}


def _cli(cli_input, digest, bam_out):
    """One run of the command line (the GPU inflating from the start, small batches and parse blocks):
    its files and its "gpu digest:" counts; cached per setting."""
    fa, bam, d, cache = cli_input
    key = (digest, bam_out)
    if key not in cache:
        env = dict(os.environ, FC2_CALLER_TIMING="1", FC2_GPU_INFLATE="2", FC2_BGZF_BATCH="24", FC2_PARSE_BLOCK="20000")
        env.pop("FC2_GPU_DIGEST", None)
        if digest is not None:
            env["FC2_GPU_DIGEST"] = digest
        o = str(d / ("o_%s_%d" % (digest, bam_out)))
        script = _CLI % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run([sys.executable, "-c", script, "-G", fa, "-o", o, "-q"] + (["-B"] if bam_out else []) + [bam],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        m = re.search(r"gpu digest: (\d+) records' fields from the device, (\d+) parsed on the host", r.stderr)
        g = re.search(r"gpu inflate: \d+ batches \(\d+ pinned\), (\d+) blocks on the GPU, (\d+) on the CPU", r.stderr)
        assert m and g, r.stderr[-3000:]
        files = {f: open(os.path.join(o, f), "rb").read() for f in sorted(os.listdir(o)) if f != "run.log"}
        cache[key] = (files, (int(m.group(1)), int(m.group(2))), (int(g.group(1)), int(g.group(2))))
    return cache[key]


@pytest.mark.parametrize("digest,bam_out", [("0", False), ("1", False), ("1", True)])
def test_cli_writes_the_same_bytes(cli_input, digest, bam_out):
    """FC2_GPU_DIGEST unset, 0 and 1: every output file byte for byte the same (with -B,
    spliced_alignments.bam among them); rows are used only at 1, and not with -B, whose records are
    written while they are read, on the reader's own thread."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ref_files, ref_dig, ref_inf = _cli(cli_input, None, bam_out)
    files, dig, inf = _cli(cli_input, digest, bam_out)
    assert sorted(files) == sorted(ref_files) and len(files) >= (5 if bam_out else 4), sorted(files)
    for f in files:
        assert files[f] == ref_files[f], f
    assert ("spliced_alignments.bam" in files) == bam_out
    assert inf == ref_inf and inf[0] > 100 and inf[1] == 0, (inf, ref_inf)
    assert ref_dig[0] == 0
    if digest == "1" and not bam_out:
        assert dig[0] > 0.9 * ref_dig[1] and dig[0] + dig[1] == ref_dig[1], (dig, ref_dig)
    else:
        assert dig[0] == 0, dig
    assert files["lin_splice_sites.bed"].count(b"\n") > 100
