"""The ingest's record lists taken from the device for the BGZF blocks the GPU inflates
(fc2_ingest_set_gpu_walk, on by default; csrc/fc2_ingest.cpp bgzf_batch): the same fragments and counts
as with the CPU inflate, with the device's lists and with the host's; every block the GPU inflated listed
there, a refused block walked on the host; and the splitter, which jumps through the lists, does exactly
the same walk either way (FC2_CALLER_TIMING's "bgzf split" line), the CLI writing the same bytes."""
import gzip
import os
import re
import subprocess
import sys

import pytest

from test_gpu_inflate import _bams, _bgzf_blocks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _read(path, device=None, walk=None):
    """The handed-back fragments and counts of a BAM through the native ingest -- the CPU inflating, or
    GPU `device`, its record lists as `walk` says (None: the default) -- then inflate_counts() and
    walk_counts(); an error is returned in place of the fragments, the counts still read."""
    from find_circ2_amd.ingest import NativeIngest
    ing = NativeIngest(path, True)
    try:
        if device is not None:
            ing.set_gpu_inflate(device)
        if walk is not None:
            ing.set_gpu_walk(walk)
        frags, res = [], None
        try:
            while not ing.eof:
                frags += [[(r.qname, r.flag, r.tid, r.pos, r.mapq, str(r.cigar), r.seq, r.qual, str(r.tags)) for r in f]
                          for f in ing.next_chunk(13, False, False, 97)]
            c = ing.counts
            res = (frags, tuple(getattr(c, f) for f, _ in c._fields_))
        except Exception as ex:          # noqa: BLE001 -- compared between the paths
            res = (type(ex).__name__, str(ex))
        return res, ing.inflate_counts(), ing.walk_counts()
    finally:
        ing.close()


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    """test_gpu_inflate's BAMs (fc2_sam_to_bam's blocks, 3000-byte and 700-byte blocks), what the CPU
    inflate reads from each, and their block counts."""
    tmp = tmp_path_factory.mktemp("walk_ingest")
    paths = _bams(tmp)
    return [(p, _read(p)[0], len(_bgzf_blocks(open(p, "rb").read()))) for p in paths]


@pytest.mark.parametrize("batch", ["3", "64", "600"])
def test_device_lists_give_the_cpu_inflates_fragments(bams, monkeypatch, batch):
    """Default (device lists) and set_gpu_walk(False): the CPU inflate's fragments and counts.  The
    blocks the GPU inflated are those after the two batches under way before set_gpu_inflate (as
    test_gpu_inflate.py counts them: none of a BAM with fewer blocks than that, so the count is asked
    to be positive per BAM where that leaves any, and over the three BAMs at every batch size); with
    the device lists every one of them is listed there, without them none."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    total = 0
    for path, cpu, n_blocks in bams:
        assert isinstance(cpu[0], list) and cpu[0]
        expect = max(0, n_blocks - (min(16, int(batch)) + int(batch)))
        on, on_inf, on_walk = _read(path, 0)
        assert on == cpu, path
        assert on_inf == (expect, 0), (path, on_inf, n_blocks)
        assert on_walk == (on_inf[0], 0), (path, on_walk)
        off, off_inf, off_walk = _read(path, 0, walk=False)
        assert off == cpu, path
        assert off_inf == on_inf and off_walk == (0, on_inf[0]), (path, off_inf, off_walk)
        explicit = _read(path, 0, walk=True)
        assert explicit == (on, on_inf, on_walk), path
        total += on_walk[0]
    assert total > 0


def test_refused_block_is_walked_on_the_host(bams, tmp_path, monkeypatch):
    """A block whose trailer carries a wrong CRC-32 (the 10th: the GPU's): the device refuses it and the
    CPU takes it -- and refuses it too, with the CPU path's error; the block counts on the host side of
    both pairs of counts, its batch's other blocks on the device's."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", "4")
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    raw = bytearray(open(bams[1][0], "rb").read())
    pos = 0
    for _ in range(9):
        pos += (raw[pos + 16] | (raw[pos + 17] << 8)) + 1
    size = (raw[pos + 16] | (raw[pos + 17] << 8)) + 1
    raw[pos + size - 8] ^= 0x5A                          # the CRC-32's first byte
    bad = str(tmp_path / "bad_crc.bam")
    open(bad, "wb").write(bytes(raw))
    cpu, cpu_inf, cpu_walk = _read(bad)
    assert isinstance(cpu[0], str) and "corrupt BGZF block" in cpu[1], cpu
    assert cpu_inf == cpu_walk == (0, 0)
    gpu, gpu_inf, gpu_walk = _read(bad, 0)
    assert gpu == cpu
    assert gpu_inf[1] == 1 and gpu_inf[0] >= 3, gpu_inf
    assert gpu_walk == gpu_inf, (gpu_walk, gpu_inf)


_CLI = """
import sys
sys.path[:0] = [%r]
from find_circ2_amd import cli
sys.exit(cli.main(sys.argv[1:]))
"""


def test_cli_splitter_walks_the_same_either_way(tmp_path):
    """The CLI on the rich input (3000-byte BGZF blocks, small batches and parse blocks, the GPU inflating
    from the start) with the device's lists and with FC2_GPU_WALK=0: the splitter reads the same number
    of records one at a time and makes the same number of jumps -- equal lists give equal walks -- and
    every output file holds the same bytes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from samgen import bgzf_compress, sam_to_bam
    from test_native_caller import _rich_sam
    sam, raw, bam = str(tmp_path / "rich.sam"), str(tmp_path / "raw.bam"), str(tmp_path / "small.bam")
    fa = _rich_sam(sam, 4000, seed=7)
    sam_to_bam(open(sam).read(), raw, compress="none")
    open(bam, "wb").write(bgzf_compress(open(raw, "rb").read(), block=3000, level=6))
    script = _CLI % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for tag, walk in (("device", None), ("host", "0")):
        env = dict(os.environ, FC2_CALLER_TIMING="1", FC2_GPU_INFLATE="2", FC2_BGZF_BATCH="24", FC2_PARSE_BLOCK="20000")
        env.pop("FC2_GPU_WALK", None)
        if walk is not None:
            env["FC2_GPU_WALK"] = walk
        o = str(tmp_path / tag)
        r = subprocess.run([sys.executable, "-c", script, "-G", fa, "-o", o, "-q", bam], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        m = re.search(r"bgzf split: (\d+) records read one at a time, (\d+) jumps", r.stderr)
        w = re.search(r"gpu walk: record lists of (\d+) blocks from the device, (\d+) walked on the host", r.stderr)
        g = re.search(r"gpu inflate: \d+ batches \(\d+ pinned\), (\d+) blocks on the GPU, (\d+) on the CPU", r.stderr)
        assert m and w and g, r.stderr[-3000:]
        files = {f: open(os.path.join(o, f), "rb").read() for f in sorted(os.listdir(o)) if f != "run.log"}
        runs.append(((int(m.group(1)), int(m.group(2))), (int(w.group(1)), int(w.group(2))),
                     (int(g.group(1)), int(g.group(2))), files))
    (split_d, walk_d, inf_d, files_d), (split_h, walk_h, inf_h, files_h) = runs
    assert split_d == split_h, (split_d, split_h)
    assert split_d[1] > 0
    assert inf_d == inf_h and inf_d[0] > 100 and inf_d[1] == 0
    assert walk_d == (inf_d[0], 0) and walk_h == (0, inf_h[0])
    assert sorted(files_d) == sorted(files_h) and len(files_d) >= 4, sorted(files_d)
    for f in files_d:
        assert files_d[f] == files_h[f], f
    assert gzip.decompress(files_d["spliced_reads.fastq.gz"]).count(b"\n") > 100
    assert files_d["lin_splice_sites.bed"].count(b"\n") > 100
