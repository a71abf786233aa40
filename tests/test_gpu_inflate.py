"""BGZF blocks inflated on the GPU (fc2_bgzf_inflate_launch, csrc/fc2_inflate.hip) against zlib: every
DEFLATE form zlib writes (stored, fixed and dynamic Huffman codes, every level and strategy), the
blocks of real BGZF BAMs (fc2_sam_to_bam at level 1, the test BGZF writer at level 6), long and
overlapping matches, empty and full 64-KiB blocks; and damaged payloads, which must end in a status
word (never a fault); CRC-32 and size are checked on the device too, the host checking them only on
the blocks it inflates itself."""
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_helpers import SLOT, inflate_run as _run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def _samples():
    rng = np.random.default_rng(1337)
    seqs = b"".join(open(os.path.join(GOLDEN, f), "rb").read() for f in ("test_ref.fa", "CDR1as_locus.fa"))
    acgt = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 70000)].tobytes()
    out = [b"", b"A", b"\x00" * 65536, b"AB" * 32768, bytes(rng.integers(0, 256, 65536, dtype=np.uint8)),
           acgt[:65280], (seqs * 30)[:65280], seqs[:1000], bytes(range(256)) * 200,
           b"".join(b"read%07d\tACGTNACGT\t" % i for i in range(3000))[:65536]]
    return out


@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("strategy", [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE,
                                      zlib.Z_FILTERED])
def test_inflate_equals_zlib(level, strategy):
    data = _samples()
    payloads = [_deflate(x, level, strategy) for x in data]
    got, st = _run(payloads, [len(x) for x in data])
    assert [int(x) for x in st] == [0] * len(data)
    assert got == data
    # the CRC-32 check on the device: the right ones pass, a wrong one is refused (status 16)
    crcs = [zlib.crc32(x) for x in data]
    _, st = _run(payloads, [len(x) for x in data], crcs)
    assert [int(x) for x in st] == [0] * len(data)
    _, st = _run(payloads, [len(x) for x in data], [c ^ (1 << (k % 32)) for k, c in enumerate(crcs)])
    assert [int(x) for x in st] == [16] * len(data)


def _bgzf_blocks(raw: bytes):
    """(payload, isize, crc) of every block of a BGZF file."""
    out, pos = [], 0
    while pos < len(raw):
        xlen = raw[pos + 10] | (raw[pos + 11] << 8)
        bsize = (raw[pos + 16] | (raw[pos + 17] << 8)) + 1
        payload = raw[pos + 12 + xlen:pos + bsize - 8]
        crc = int.from_bytes(raw[pos + bsize - 8:pos + bsize - 4], "little")
        isize = int.from_bytes(raw[pos + bsize - 4:pos + bsize], "little")
        out.append((payload, isize, crc))
        pos += bsize
    return out


def test_inflate_real_bam_blocks(tmp_path):
    """Every block of BAMs written by fc2_sam_to_bam (zlib level 1) and by the tests' BGZF writer
    (level 6, small blocks): the GPU output's CRC-32 equals the block's."""
    from samgen import bgzf_compress, sam_to_bam as py_sam_to_bam
    from test_native_caller import _rich_sam
    from find_circ2_amd.ingest import sam_to_bam
    sam = str(tmp_path / "rich.sam")
    _rich_sam(sam, 3000, seed=99)
    bam1 = str(tmp_path / "a.bam")
    sam_to_bam(sam, bam1)
    raw = str(tmp_path / "raw.bam")
    py_sam_to_bam(open(sam).read(), raw, compress="none")
    blocks = _bgzf_blocks(open(bam1, "rb").read()) + \
        _bgzf_blocks(bgzf_compress(open(raw, "rb").read(), block=3000, level=6))
    got, st = _run([b[0] for b in blocks], [b[1] for b in blocks], [b[2] for b in blocks])
    assert list(st) == [0] * len(blocks) and len(blocks) > 20
    assert [zlib.crc32(g) for g in got] == [b[2] for b in blocks]


def test_inflate_damaged_payloads_end_in_a_status():
    """Cut, bit-flipped, garbage and wrongly sized payloads: the launch completes, every block gets a
    status, and a block reported as inflated has the claimed size (its CRC-32 is the host's check)."""
    rng = np.random.default_rng(4711)
    data = _samples()
    good = [_deflate(x, lv) for x in data for lv in (1, 6)]
    sizes = [len(x) for x in data for _ in (1, 6)]
    payloads, want = [], []
    for p, n in zip(good, sizes):
        b = bytearray(p)
        kind = int(rng.integers(0, 5))
        if kind == 0 and len(b) > 4:
            b = b[:int(rng.integers(1, len(b)))]
        elif kind == 1 and len(b):
            for _ in range(8):
                k = int(rng.integers(0, len(b)))
                b[k] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:
            b = bytearray(rng.integers(0, 256, int(rng.integers(0, 4000)), dtype=np.uint8).tobytes())
        elif kind == 3:
            n = max(0, n - int(rng.integers(1, 100)))    # claimed size too small
        else:
            n = min(SLOT, n + int(rng.integers(1, 100)))  # claimed size too large
        payloads.append(bytes(b))
        want.append(n)
    payloads.append(_deflate(b"x" * 10))
    want.append(SLOT + 1)                               # over the BGZF limit
    got, st = _run(payloads, want)
    assert st[-1] != 0
    assert all(0 <= s <= 16 for s in st)
    for g, s, n in zip(got, st, want):
        if s == 0:
            assert len(g) == n


def _read_all(path, device=None, after=None):
    """Every handed-back fragment and the counts of a BAM read by the native ingest (GPU inflate on
    `device` -- from the start, or once `after` bytes were read -- or the CPU), and the inflate counts;
    or the error raised."""
    from find_circ2_amd.ingest import NativeIngest
    ing = None
    try:
        ing = NativeIngest(path, True)
        if device is not None and after is not None:
            ing.set_gpu_inflate_from(device, after)
        elif device is not None:
            ing.set_gpu_inflate(device)
        frags = []
        while not ing.eof:
            frags += [[(r.qname, r.flag, r.tid, r.pos, r.mapq, str(r.cigar), r.seq, r.qual, str(r.tags)) for r in f]
                      for f in ing.next_chunk(13, False, False, 97)]
        c = ing.counts
        return frags, tuple(getattr(c, f) for f, _ in c._fields_), ing.inflate_counts()
    except Exception as ex:          # noqa: BLE001 -- compared between the two paths
        return type(ex).__name__, str(ex), None
    finally:
        if ing is not None:
            ing.close()


def _bams(tmp_path):
    from samgen import bgzf_compress, sam_to_bam as py_sam_to_bam
    from test_native_caller import _rich_sam
    from find_circ2_amd.ingest import sam_to_bam
    sam = str(tmp_path / "rich.sam")
    _rich_sam(sam, 4000, seed=7)
    lvl1 = str(tmp_path / "lvl1.bam")
    sam_to_bam(sam, lvl1)                               # zlib level 1, 0xff00-byte blocks
    raw = str(tmp_path / "raw.bam")
    py_sam_to_bam(open(sam).read(), raw, compress="none")
    small = str(tmp_path / "small.bam")                 # level 6, 3000-byte blocks
    open(small, "wb").write(bgzf_compress(open(raw, "rb").read(), block=3000, level=6))
    tiny = str(tmp_path / "tiny.bam")                   # level 1, 700-byte blocks: GPU batches of chunks
    open(tiny, "wb").write(bgzf_compress(open(raw, "rb").read(), block=700, level=1))
    return lvl1, small, tiny


@pytest.mark.parametrize("batch", ["3", "64", "600"])
def test_ingest_gpu_inflate_equals_cpu(tmp_path, monkeypatch, batch):
    """The native ingest with its BGZF batches inflated on the GPU hands back the same fragments and
    counts as with the CPU inflate; every block after the batches read at the open went through the GPU."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    for bam in _bams(tmp_path):
        cpu = _read_all(bam)
        gpu = _read_all(bam, 0)
        assert isinstance(cpu[0], list) and cpu[0], cpu
        assert cpu[:2] == gpu[:2]
        # the first two batches were under way before set_gpu_inflate (the open reads the header
        # from the first and starts the second)
        n_blocks = len(_bgzf_blocks(open(bam, "rb").read()))
        ahead = min(16, int(batch)) + int(batch)
        assert gpu[2] == (max(0, n_blocks - ahead), 0), (bam, gpu[2], n_blocks)
        assert cpu[2] == (0, 0)


def test_ingest_gpu_inflate_oversized_member_in_a_chunked_batch(tmp_path, monkeypatch):
    """A gzip member that inflates to more than BGZF's 64 KiB (htslib reads such members) in the first
    chunk of a GPU batch of three chunks, 499 in-spec blocks behind it in the batch: the blocks lie in
    the batch at the sums of the true ISIZEs before them, on the device as on the host, so from the
    oversized member on the batch is the CPU's, and the fragments and counts are the CPU inflate's
    (when the device summed min(ISIZE, 64 KiB) instead, the later chunks' bytes lay where the host did
    not read them and this input ended in a BAM format error).
    The input is the `tiny` BAM of _bams() (700-byte blocks, level 1) with 100 of its blocks joined
    into one member.  The member is block 716 of the file, not one of its first 256: with batches of
    600 the first 616 blocks are read before set_gpu_inflate takes effect (see
    test_ingest_gpu_inflate_equals_cpu), so that is the first chunk of the first batch the GPU takes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from samgen import bgzf_compress
    monkeypatch.setenv("FC2_BGZF_BATCH", "600")
    data = _raw_rich_bam(tmp_path)
    a = 700 * (16 + 600 + 100)
    b = a + 70000
    big = bgzf_compress(data[a:b], block=b - a, level=1)[:-28]
    assert len(big) <= 65536 and len(_bgzf_blocks(big)) == 1
    packed = bgzf_compress(data[:a], block=700, level=1)[:-28] + big + bgzf_compress(data[b:], block=700, level=1)
    blocks = _bgzf_blocks(packed)
    assert blocks[716][1] == 70000 and all(isize <= 700 for _, isize, _ in blocks[:716] + blocks[717:])
    assert len(blocks) >= 616 + 2 * 600                   # the spilled batch whole, and one more for the GPU
    bam = str(tmp_path / "oversized.bam")
    open(bam, "wb").write(packed)
    cpu = _read_all(bam)
    gpu = _read_all(bam, 0)
    assert isinstance(cpu[0], list) and cpu[0], cpu
    print("inflate counts (GPU blocks, CPU blocks):", gpu[2])
    assert gpu[:2] == cpu[:2]
    assert gpu[2] is not None and gpu[2][0] > 0 and gpu[2][1] > 0, gpu[2]


def _block_spans(raw: bytes):
    """(start, size) of every block of a BGZF file, its 'BC' subfield found among any others."""
    out, pos = [], 0
    while pos < len(raw):
        xlen = raw[pos + 10] | (raw[pos + 11] << 8)
        q = pos + 12
        while raw[q:q + 2] != b"BC":
            q += 4 + (raw[q + 2] | (raw[q + 3] << 8))
            assert q < pos + 12 + xlen
        bsize = (raw[q + 4] | (raw[q + 5] << 8)) + 1
        out.append((pos, bsize))
        pos += bsize
    return out


def _raw_rich_bam(tmp_path):
    """The uncompressed BAM bytes of the rich SAM of _bams()."""
    from samgen import sam_to_bam as py_sam_to_bam
    from test_native_caller import _rich_sam
    sam = str(tmp_path / "rich.sam")
    _rich_sam(sam, 4000, seed=7)
    raw = str(tmp_path / "raw.bam")
    py_sam_to_bam(open(sam).read(), raw, compress="none")
    return open(raw, "rb").read()


@pytest.mark.parametrize("writer", ["libdeflate1", "libdeflate12", "extra_subfield"])
def test_ingest_gpu_inflate_other_writers(tmp_path, monkeypatch, writer):
    """BAMs as htslib built with libdeflate writes them (several DEFLATE blocks a BGZF block, levels 1
    and 12, 0xff00-byte blocks), and one with a 5-byte extra subfield before 'BC' in every block: the
    same fragments and counts as with the CPU inflate, every block after the read-ahead inflated on
    the GPU and none retried on the CPU."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from samgen import bgzf_compress
    from test_deflate_forge import LIBDEFLATE, libdeflate_deflate
    monkeypatch.setenv("FC2_BGZF_BATCH", "3")
    data = _raw_rich_bam(tmp_path)
    if writer == "extra_subfield":
        packed = bgzf_compress(data, block=0xff00, level=1, extra=b"XY\x01\x00\x5a")
    else:
        if LIBDEFLATE is None:
            pytest.skip("libdeflate.so.0 does not load")
        level = int(writer[len("libdeflate"):])
        packed = bgzf_compress(data, block=0xff00, deflate=lambda chunk: libdeflate_deflate(chunk, level))
    bam = str(tmp_path / (writer + ".bam"))
    open(bam, "wb").write(packed)
    cpu = _read_all(bam)
    gpu = _read_all(bam, 0)
    assert isinstance(cpu[0], list) and cpu[0], cpu
    assert cpu[:2] == gpu[:2]
    n_blocks = len(_block_spans(packed))
    assert n_blocks > 10
    assert gpu[2] == (n_blocks - (3 + 3), 0), (gpu[2], n_blocks)
    assert cpu[2] == (0, 0)


@pytest.mark.parametrize("form", ["dist_incomplete", "litlen_incomplete", "valid_15bit_trailing", "unused_codeword"])
def test_ingest_gpu_inflate_forged_block(tmp_path, monkeypatch, form):
    """The 10th block of a BAM (the GPU's) replaced by one carrying the same BAM bytes, CRC-32 and
    ISIZE in a forged DEFLATE stream: an incomplete distance code and an incomplete literal/length
    code (both CPU inflaters refuse them), 15-bit dynamic codes with bytes left over after the final
    block (valid), and the unused codeword of a single 1-bit distance code (zlib refuses it,
    libdeflate decodes the code's distance).  The GPU inflate gives the run the CPU inflate gives:
    the same fragments and counts, or the same error."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deflate_forge import Code, Forge, LenOnly, make_code
    from samgen import bgzf_compress
    from test_deflate_forge import D15, L15
    monkeypatch.setenv("FC2_BGZF_BATCH", "4")
    _, small, _ = _bams(tmp_path)
    raw = open(small, "rb").read()
    start, size = _block_spans(raw)[9]
    chunk = zlib.decompress(raw[start + 18:start + size - 8], -15)
    assert len(chunk) == 3000
    if form == "dist_incomplete":
        forged = bytes(Forge().dynamic(L15, [2, 2], list(chunk), True))
    elif form == "litlen_incomplete":
        forged = bytes(Forge().dynamic(L15[:285] + [0], D15, list(chunk), True))
    elif form == "valid_15bit_trailing":
        forged = bytes(Forge().dynamic(L15, D15, list(chunk), True).raw_bytes(b"left over"))
    else:
        k = next(i for i in range(1, len(chunk) - 3) if chunk[i - 1:i] * 3 == chunk[i:i + 3])
        toks = list(chunk[:k]) + [LenOnly(3), Code(1, 1)] + list(chunk[k + 3:])
        forged = bytes(Forge().dynamic(make_code(286, 9), [1], toks, True))
    block = bgzf_compress(chunk, block=len(chunk), deflate=lambda _: forged)[:-28]
    bam = str(tmp_path / (form + ".bam"))
    open(bam, "wb").write(raw[:start] + block + raw[start + size:])
    cpu, gpu = _read_all(bam), _read_all(bam, 0)
    if cpu[2] is None:                                   # refused: the same error
        assert "corrupt BGZF block" in cpu[1], cpu
        assert gpu == cpu
    else:
        assert isinstance(cpu[0], list) and cpu[0] and cpu[:2] == gpu[:2]
        assert cpu[:2] == _read_all(small)[:2]
    if form == "valid_15bit_trailing":
        assert cpu[2] == (0, 0) and gpu[2] is not None and gpu[2][0] > 0 and gpu[2][1] == 0, (cpu[2], gpu[2])
    if form in ("dist_incomplete", "litlen_incomplete"):
        assert cpu[2] is None


def test_ingest_gpu_inflate_from_a_threshold(tmp_path, monkeypatch):
    """fc2_ingest_set_gpu_inflate_from (the CLI's default, 256 MiB): an input smaller than the threshold
    never touches the device (no block counted on it); one past it switches to the GPU mid-stream (the
    device's buffers made in the background from there) -- the same fragments and counts as the CPU
    inflate either way, at every batch size."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.delenv("FC2_GPU_INFLATE", raising=False)
    for batch in ("3", "64"):
        monkeypatch.setenv("FC2_BGZF_BATCH", batch)
        for bam in _bams(tmp_path):
            cpu = _read_all(bam)
            size = os.path.getsize(bam)
            never = _read_all(bam, 0, after=10 * size)
            assert never[:2] == cpu[:2] and never[2] == (0, 0), (bam, never[2])
            for after in (1, size // 3):
                mid = _read_all(bam, 0, after=after)
                assert mid[:2] == cpu[:2], (bam, after)
                n_blocks = len(_bgzf_blocks(open(bam, "rb").read()))
                assert sum(mid[2]) <= n_blocks, (bam, after, mid[2])


def test_ingest_gpu_inflate_corrupt_block_same_error(tmp_path, monkeypatch):
    """A damaged block: the same error with the GPU inflate as with the CPU's (the device checks each
    block's CRC-32 and ISIZE and refuses this one; the CPU retry, which checks them itself, reports it)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", "4")
    _, small, _ = _bams(tmp_path)
    raw = bytearray(open(small, "rb").read())
    pos = 0
    for _ in range(9):                                   # the 10th block (the GPU's)
        pos += (raw[pos + 16] | (raw[pos + 17] << 8)) + 1
    for k in (40, 41, 300, 301):
        raw[pos + k] ^= 0x5A
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    cpu, gpu = _read_all(bad), _read_all(bad, 0)
    assert cpu[2] is None and "corrupt BGZF block" in cpu[1], cpu
    assert gpu == cpu


def test_cli_bam_input_inflated_on_the_gpu(tmp_path, monkeypatch):
    """The CLI on a BAM reads it with the GPU inflate (run.log's process phases count the blocks) and
    writes the same files as with FC2_GPU_INFLATE=0; and with the buffers made in the background (the
    default) the same files again."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_cli import run_cli
    from test_cli_gpu import _compare, _sim_reads
    monkeypatch.setenv("FC2_BGZF_BATCH", "1")
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")          # the device's buffers ready before the first read
    fa = os.path.join(GOLDEN, "CDR1as_locus.fa")
    rd = _sim_reads(fa, 3000, seed=5)
    rc1, o1 = run_cli(tmp_path, fa, rd, bam=True, evaluator=None, tag="gpu_inflate")
    monkeypatch.setenv("FC2_GPU_INFLATE", "0")
    rc2, o2 = run_cli(tmp_path, fa, rd, bam=True, evaluator=None, tag="cpu_inflate")
    assert rc1 == rc2 == 0
    _compare(o1, o2)

    def blocks(o):
        line = [l for l in open(os.path.join(o, "run.log")) if "process phases" in l][0]
        kv = dict(x.split("=") for x in line.split("process phases: ")[1].strip().split(", "))
        return float(kv["inflate_gpu_blocks"]), float(kv["inflate_cpu_blocks"])
    g1, c1 = blocks(o1)
    assert g1 >= 2 and c1 == 0
    assert blocks(o2) == (0.0, 0.0)
    monkeypatch.setenv("FC2_GPU_INFLATE", "1")
    rc3, o3 = run_cli(tmp_path, fa, rd, bam=True, evaluator=None, tag="gpu_inflate_background")
    assert rc3 == 0
    _compare(o1, o3)
    # the default: the GPU takes over past cli.GPU_INFLATE_AFTER bytes of input -- never for this
    # input; at a threshold of one byte, from the first batches whose device buffers are ready
    monkeypatch.delenv("FC2_GPU_INFLATE")
    rc4, o4 = run_cli(tmp_path, fa, rd, bam=True, evaluator=None, tag="gpu_inflate_default")
    assert rc4 == 0
    _compare(o1, o4)
    assert blocks(o4) == (0.0, 0.0)
    from find_circ2_amd import cli
    monkeypatch.setattr(cli, "GPU_INFLATE_AFTER", 1)
    rc5, o5 = run_cli(tmp_path, fa, rd, bam=True, evaluator=None, tag="gpu_inflate_default_low")
    assert rc5 == 0
    _compare(o1, o5)


def test_two_ingests_with_different_batches_share_the_pinned_pool(tmp_path, monkeypatch):
    """Two GPU-inflating ingests open at once with different batch sizes (so the pinned pool holds
    buffers of two sizes) read, interleaved, what each reads alone."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from find_circ2_amd.ingest import NativeIngest
    _, small, tiny = _bams(tmp_path)
    want = {}
    for bam, batch in ((small, "3"), (tiny, "600")):
        monkeypatch.setenv("FC2_BGZF_BATCH", batch)
        want[bam] = _read_all(bam)[:2]
    ings = []
    for bam, batch in ((small, "3"), (tiny, "600")):
        monkeypatch.setenv("FC2_BGZF_BATCH", batch)
        ing = NativeIngest(bam, True)
        ing.set_gpu_inflate(0)
        ings.append((bam, ing, []))
    try:
        while any(not ing.eof for _, ing, _ in ings):
            for _, ing, frags in ings:
                if not ing.eof:
                    frags += [[(r.qname, r.flag, r.tid, r.pos, r.mapq, str(r.cigar), r.seq, r.qual, str(r.tags))
                               for r in f] for f in ing.next_chunk(13, False, False, 31)]
        for bam, ing, frags in ings:
            c = ing.counts
            assert (frags, tuple(getattr(c, f) for f, _ in c._fields_)) == want[bam]
            assert ing.inflate_counts()[0] > 0 and ing.inflate_counts()[1] == 0
    finally:
        for _, ing, _ in ings:
            ing.close()
