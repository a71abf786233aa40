"""The command line with spliced_reads.fastq.gz compressed on the GPU (FC2_GPU_GZIP=1): the reads
text is the same after decompression, every other file is byte-identical, run.log counts the
pieces; with another tile size, together with the GPU inflate of a BAM input, and for an empty
file."""
import gzip
import os

import pytest

from conftest import GOLDEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _pieces(o):
    line = [l for l in open(os.path.join(o, "run.log")) if "process phases" in l][0]
    kv = dict(x.split("=") for x in line.split("process phases: ")[1].strip().split(", "))
    return float(kv["gzip_gpu_pieces"]), float(kv["gzip_cpu_pieces"])


def test_cli_reads_gz_compressed_on_the_gpu(tmp_path, monkeypatch):
    from test_cli import run_cli
    from test_cli_gpu import _compare, _sim_reads
    fa = os.path.join(GOLDEN, "CDR1as_locus.fa")
    rd = _sim_reads(fa, 3000, seed=5)
    monkeypatch.setenv("FC2_GPU_GZIP", "1")
    rc1, o1 = run_cli(tmp_path, fa, rd, evaluator=None, tag="gpu_gzip")
    monkeypatch.setenv("FC2_GPU_GZIP", "0")
    rc2, o2 = run_cli(tmp_path, fa, rd, evaluator=None, tag="cpu_gzip")
    assert rc1 == rc2 == 0
    _compare(o1, o2)
    g1, c1 = _pieces(o1)
    assert g1 >= 1 and c1 == 0
    assert _pieces(o2) == (0.0, 0.0)
    with gzip.open(os.path.join(o1, "spliced_reads.fastq.gz"), "rb") as f:
        assert len(f.read()) > 10000             # (the comparison was not of two empty files)
    # small tiles: many members per piece
    monkeypatch.setenv("FC2_GPU_GZIP", "1")
    monkeypatch.setenv("FC2_GPU_GZIP_TILE", "997")
    rc3, o3 = run_cli(tmp_path, fa, rd, evaluator=None, tag="gpu_gzip_997")
    assert rc3 == 0
    _compare(o3, o2)
    assert os.path.getsize(os.path.join(o3, "spliced_reads.fastq.gz")) != \
        os.path.getsize(os.path.join(o1, "spliced_reads.fastq.gz"))


def test_cli_gpu_gzip_with_gpu_inflate_on_one_device(tmp_path, monkeypatch):
    from test_cli import run_cli
    from test_cli_gpu import _compare, _sim_reads
    fa = os.path.join(GOLDEN, "CDR1as_locus.fa")
    rd = _sim_reads(fa, 3000, seed=5)
    monkeypatch.setenv("FC2_BGZF_BATCH", "1")
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    monkeypatch.setenv("FC2_GPU_GZIP", "1")
    rc1, o1 = run_cli(tmp_path, fa, rd, bam=True, evaluator=None, tag="both_gpu")
    monkeypatch.setenv("FC2_GPU_INFLATE", "0")
    monkeypatch.setenv("FC2_GPU_GZIP", "0")
    rc2, o2 = run_cli(tmp_path, fa, rd, bam=True, evaluator=None, tag="both_cpu")
    assert rc1 == rc2 == 0
    _compare(o1, o2)
    g, c = _pieces(o1)
    assert g >= 1 and c == 0


def test_cli_gpu_gzip_of_no_reads(tmp_path, monkeypatch):
    from test_cli import run_cli
    fa = os.path.join(GOLDEN, "CDR1as_locus.fa")
    monkeypatch.setenv("FC2_GPU_GZIP", "1")
    rc, o = run_cli(tmp_path, fa, [], evaluator=None, tag="gpu_gzip_empty")
    assert rc == 0
    raw = open(os.path.join(o, "spliced_reads.fastq.gz"), "rb").read()
    assert len(raw) >= 18 and gzip.decompress(raw) == b""
