"""The command line with the GPU writers at level 2 and two passes: FC2_GPU_GZIP=1 FC2_GPU_GZIP_LEVEL=2
FC2_GPU_GZIP_PASSES=2 for spliced_reads.fastq.gz and -B FC2_GPU_BAM=1 FC2_GPU_BAM_LEVEL=2 FC2_GPU_BAM_PASSES=2 for
spliced_alignments.bam, in one run.  Both files inflate to the default run's bytes, the BAM is cut in the same
blocks, the device compressed every piece, run.log's "process phases" line carries gzip_gpu_passes=2 and
bam_gpu_passes=2, and the first payloads are the host model's (deflate_model_priced.py).  Passes without level 2, or
out of 1..3, end the run at its start with the library's message.  Sizes are not asserted here: they are the CPU
tests' (test_deflate_model_priced.py)."""
import gzip
import os
import zlib

import pytest

from bgzf_helpers import EOF_BLOCK, read_bam
from deflate_model_priced import model_priced
from find_circ2_amd import cli
from test_native_caller import _rich_sam

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VARS = ("FC2_GPU_GZIP", "FC2_GPU_GZIP_LEVEL", "FC2_GPU_GZIP_DEPTH", "FC2_GPU_GZIP_NICE", "FC2_GPU_GZIP_HISTORY",
        "FC2_GPU_GZIP_TILE", "FC2_GPU_GZIP_PASSES", "FC2_GPU_BAM", "FC2_GPU_BAM_LEVEL", "FC2_GPU_BAM_DEPTH",
        "FC2_GPU_BAM_NICE", "FC2_GPU_BAM_TILE", "FC2_GPU_BAM_HISTORY", "FC2_GPU_BAM_PASSES")


def _phases(o):
    line = [l for l in open(os.path.join(o, "run.log")) if "process phases" in l][0]
    return dict(x.split("=") for x in line.split("process phases: ")[1].strip().split(", "))


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("clipriced")
    sam = str(d / "rich.sam")
    return _rich_sam(sam, 1500, seed=31), sam


def _run(fa, sam, out):
    return cli.main(["-G", fa, "-o", out, "-n", "test", "-q", "-B", sam], evaluator_factory=None)


def test_cli_both_writers_with_two_passes(rich, tmp_path, monkeypatch):
    from test_cli_gpu import _compare
    fa, sam = rich
    for k in VARS:
        monkeypatch.delenv(k, raising=False)
    o0 = str(tmp_path / "default")
    assert _run(fa, sam, o0) == 0
    for k in ("FC2_GPU_GZIP", "FC2_GPU_BAM"):
        monkeypatch.setenv(k, "1")
        monkeypatch.setenv(k + "_LEVEL", "2")
        monkeypatch.setenv(k + "_PASSES", "2")
    o = str(tmp_path / "priced")
    assert _run(fa, sam, o) == 0
    _compare(o, o0)                                 # every other file; the two compressed ones by what they hold
    text = gzip.decompress(open(os.path.join(o, "spliced_reads.fastq.gz"), "rb").read())
    assert len(text) > 10000 and text == gzip.decompress(open(os.path.join(o0, "spliced_reads.fastq.gz"), "rb").read())
    p0, p = os.path.join(o0, "spliced_alignments.bam"), os.path.join(o, "spliced_alignments.bam")
    blocks0, data0, rec0 = read_bam(p0)
    blocks, data, rec = read_bam(p)
    assert data == data0 and rec == rec0 and len(data0) - rec0 > 400000
    assert [b[3] for b in blocks] == [b[3] for b in blocks0] and all(b[0] <= 65536 for b in blocks)
    assert blocks[0] == blocks0[0] and open(p, "rb").read().endswith(EOF_BLOCK)
    kv0, kv = _phases(o0), _phases(o)
    assert float(kv["gzip_gpu_pieces"]) > 0 and float(kv["gzip_cpu_pieces"]) == 0
    assert float(kv["bam_gpu_pieces"]) > 0 and float(kv["bam_cpu_pieces"]) == 0
    assert (kv["gzip_gpu_level"], kv["gzip_gpu_passes"]) == ("2", "2")
    assert (kv["bam_gpu_level"], kv["bam_gpu_passes"]) == ("2", "2")
    assert not [k for k in kv if k.endswith(("_depth", "_nice"))]
    assert not [k for k in kv0 if k.endswith(("_passes", "_level"))]
    # the first payloads are the model's with two passes at level 2's own search
    gz = open(os.path.join(o, "spliced_reads.fastq.gz"), "rb").read()
    z = zlib.decompressobj(-15)
    tile = z.decompress(gz[10:])
    assert z.eof and 0 < len(tile) <= 32768 and text.startswith(tile)
    assert gz[10:len(gz) - len(z.unused_data)] == model_priced(tile, 8, 32, 2)[0]
    n_head = next(k for k in range(1, len(blocks0)) if sum(b[3] for b in blocks0[:k]) == rec0)
    assert blocks[n_head][1] == model_priced(data0[rec0:rec0 + 0xff00], 8, 32, 2)[0]


def test_cli_passes_beside_a_search_tiles_and_a_history(rich, tmp_path, monkeypatch):
    fa, sam = rich
    for k in VARS:
        monkeypatch.delenv(k, raising=False)
    for k in ("FC2_GPU_GZIP", "FC2_GPU_BAM"):
        monkeypatch.setenv(k, "1")
        monkeypatch.setenv(k + "_LEVEL", "2")
        monkeypatch.setenv(k + "_DEPTH", "32")
        monkeypatch.setenv(k + "_NICE", "258")
        monkeypatch.setenv(k + "_HISTORY", "32768")
    monkeypatch.setenv("FC2_GPU_BAM_TILE", "16320")
    o1 = str(tmp_path / "one")
    assert _run(fa, sam, o1) == 0
    monkeypatch.setenv("FC2_GPU_GZIP_PASSES", "1")             # one pass, said aloud: the same bytes, no field
    monkeypatch.setenv("FC2_GPU_BAM_PASSES", "1")
    oe = str(tmp_path / "said")
    assert _run(fa, sam, oe) == 0
    monkeypatch.setenv("FC2_GPU_GZIP_PASSES", "3")
    monkeypatch.setenv("FC2_GPU_BAM_PASSES", "3")
    o3 = str(tmp_path / "three")
    assert _run(fa, sam, o3) == 0
    for f in ("spliced_reads.fastq.gz", "spliced_alignments.bam"):
        a, e, b = (open(os.path.join(o, f), "rb").read() for o in (o1, oe, o3))
        assert a == e and b != a and gzip.decompress(b) == gzip.decompress(a), f
    kv1, kve, kv3 = _phases(o1), _phases(oe), _phases(o3)
    assert list(kv1) == list(kve) and not [k for k in kv1 if k.endswith("_passes")]
    assert (kv3["gzip_gpu_passes"], kv3["bam_gpu_passes"], kv3["bam_gpu_depth"], kv3["bam_gpu_tile"]) == ("3", "3", "32", "16320")
    assert float(kv3["gzip_cpu_pieces"]) == 0 and float(kv3["bam_cpu_pieces"]) == 0 and float(kv3["bam_gpu_pieces"]) > 0


@pytest.mark.parametrize("env", [{"FC2_GPU_BAM": "1", "FC2_GPU_BAM_PASSES": "2"},
                                 {"FC2_GPU_BAM": "1", "FC2_GPU_BAM_LEVEL": "2", "FC2_GPU_BAM_PASSES": "4"},
                                 {"FC2_GPU_GZIP": "1", "FC2_GPU_GZIP_PASSES": "2"},
                                 {"FC2_GPU_GZIP": "1", "FC2_GPU_GZIP_LEVEL": "2", "FC2_GPU_GZIP_PASSES": "4"},
                                 {"FC2_GPU_GZIP": "1", "FC2_GPU_GZIP_LEVEL": "2", "FC2_GPU_GZIP_PASSES": "0"}])
def test_cli_refused_passes_end_the_run_at_its_start(rich, tmp_path, monkeypatch, capfd, env):
    fa, sam = rich
    for k in VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _run(fa, sam, str(tmp_path / "refused")) == 1
    err = capfd.readouterr().err
    assert "_device_passes" in err and ("level 2" in err or "1..3" in err)
