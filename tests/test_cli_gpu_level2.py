"""The command line with the GPU writers at the compressor's level 2: FC2_GPU_GZIP=1 FC2_GPU_GZIP_LEVEL=2
for spliced_reads.fastq.gz and -B FC2_GPU_BAM=1 FC2_GPU_BAM_LEVEL=2 for spliced_alignments.bam.  What the
files decompress to is the default run's, the compressed bytes are not level 1's, the device compressed
every piece, the BAM's blocks are cut where the default run cuts them and their payloads are the host
model's (deflate_model2.py), and run.log's "process phases" line says which level ran."""
import gzip
import os
import zlib

import pytest

from bgzf_helpers import EOF_BLOCK, read_bam
from conftest import GOLDEN
from deflate_model2 import model2
from find_circ2_amd import cli
from test_native_caller import _rich_sam

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _phases(o):
    line = [l for l in open(os.path.join(o, "run.log")) if "process phases" in l][0]
    return dict(x.split("=") for x in line.split("process phases: ")[1].strip().split(", "))


def test_cli_reads_gz_at_level_2(tmp_path, monkeypatch):
    from test_cli import run_cli
    from test_cli_gpu import _compare, _sim_reads
    fa = os.path.join(GOLDEN, "CDR1as_locus.fa")
    rd = _sim_reads(fa, 3000, seed=5)
    monkeypatch.delenv("FC2_GPU_GZIP", raising=False)
    monkeypatch.setenv("FC2_GPU_GZIP_LEVEL", "2")
    rc0, o0 = run_cli(tmp_path, fa, rd, evaluator=None, tag="default")
    monkeypatch.setenv("FC2_GPU_GZIP", "1")
    rc2, o2 = run_cli(tmp_path, fa, rd, evaluator=None, tag="level2")
    monkeypatch.setenv("FC2_GPU_GZIP_LEVEL", "1")
    rc1, o1 = run_cli(tmp_path, fa, rd, evaluator=None, tag="level1")
    assert rc0 == rc1 == rc2 == 0
    _compare(o2, o0)
    gz = [open(os.path.join(o, "spliced_reads.fastq.gz"), "rb").read() for o in (o0, o1, o2)]
    text = gzip.decompress(gz[2])
    assert len(text) > 10000 and text == gzip.decompress(gz[1])
    assert gz[2] != gz[1] and len(gz[2]) < len(gz[1])
    # the first member's stream is the model's of the tile it holds
    z = zlib.decompressobj(-15)
    tile = z.decompress(gz[2][10:])
    assert z.eof and 0 < len(tile) <= 32768 and text.startswith(tile)
    assert gz[2][10:len(gz[2]) - len(z.unused_data)] == model2(tile)[0]
    kv0, kv1, kv2 = _phases(o0), _phases(o1), _phases(o2)
    assert float(kv2["gzip_gpu_pieces"]) > 0 and float(kv2["gzip_cpu_pieces"]) == 0
    assert kv2["gzip_gpu_level"] == "2"
    assert "gzip_gpu_level" not in kv1 and "gzip_gpu_level" not in kv0 and float(kv0["gzip_gpu_pieces"]) == 0


def test_reads_gz_level_after_the_device_is_refused_and_changes_nothing(tmp_path, monkeypatch):
    """fc2_caller_set_reads_gz_device_level after fc2_caller_set_reads_gz_device: FC2_E_PARAM, and the file
    is written at the level set before -- the command line's own calls (level 1), then the late call from
    a wrapper around NativeCaller.open."""
    from deflate_model import model
    from find_circ2_amd import _native as N
    from find_circ2_amd.native_caller import NativeCaller
    from test_cli import run_cli
    from test_cli_gpu import _sim_reads
    fa = os.path.join(GOLDEN, "CDR1as_locus.fa")
    rd = _sim_reads(fa, 3000, seed=5)
    late, opened = [], NativeCaller.open

    def open_then_set_the_level(self):
        r = opened(self)
        late.append((self.gzip_device, N.lib().fc2_caller_set_reads_gz_device_level(self.h, 2),
                     N.lib().fc2_last_error().decode()))
        return r

    monkeypatch.setattr(NativeCaller, "open", open_then_set_the_level)
    monkeypatch.setenv("FC2_GPU_GZIP", "1")
    monkeypatch.delenv("FC2_GPU_GZIP_LEVEL", raising=False)
    rc, o = run_cli(tmp_path, fa, rd, evaluator=None, tag="late")
    assert rc == 0 and len(late) == 1
    device, status, message = late[0]
    assert device is not None and status == N.FC2_E_PARAM and "before fc2_caller_set_reads_gz_device" in message
    gz = open(os.path.join(o, "spliced_reads.fastq.gz"), "rb").read()
    z = zlib.decompressobj(-15)
    tile = z.decompress(gz[10:])
    stream = gz[10:len(gz) - len(z.unused_data)]
    assert z.eof and len(tile) > 10000
    assert stream == model(tile)[0] and stream != model2(tile)[0]
    kv = _phases(o)
    assert float(kv["gzip_gpu_pieces"]) > 0 and float(kv["gzip_cpu_pieces"]) == 0 and "gzip_gpu_level" not in kv


def test_cli_bam_records_at_level_2(tmp_path, monkeypatch):
    from test_cli_gpu import _compare
    sam = str(tmp_path / "rich.sam")
    fa = _rich_sam(sam, 1500, seed=31)

    def run(tag):
        out = str(tmp_path / tag)
        assert cli.main(["-G", fa, "-o", out, "-n", "test", "-q", "-B", sam], evaluator_factory=None) == 0
        return out

    monkeypatch.delenv("FC2_GPU_BAM", raising=False)
    monkeypatch.setenv("FC2_GPU_BAM_LEVEL", "2")
    o0 = run("default")
    monkeypatch.setenv("FC2_GPU_BAM", "1")
    o2 = run("level2")
    monkeypatch.delenv("FC2_GPU_BAM_LEVEL")
    o1 = run("level1")
    _compare(o2, o0)
    p0, p1, p2 = (os.path.join(o, "spliced_alignments.bam") for o in (o0, o1, o2))
    blocks0, data0, rec0 = read_bam(p0)
    blocks2, data2, rec2 = read_bam(p2)
    assert data2 == data0 and len(data0) - rec0 > 400000
    assert [b[3] for b in blocks2] == [b[3] for b in blocks0] and all(b[0] <= 65536 for b in blocks2)
    assert blocks2[0] == blocks0[0] and open(p2, "rb").read().endswith(EOF_BLOCK)
    assert os.path.getsize(p2) < os.path.getsize(p1) and read_bam(p1)[1] == data0
    n_head = next(k for k in range(1, len(blocks0)) if sum(b[3] for b in blocks0[:k]) == rec0)
    for i in range(2):
        assert blocks2[n_head + i][1] == model2(data0[rec0 + i * 0xff00:rec0 + (i + 1) * 0xff00])[0], i
    kv0, kv1, kv2 = _phases(o0), _phases(o1), _phases(o2)
    assert float(kv2["bam_gpu_pieces"]) > 0 and float(kv2["bam_cpu_pieces"]) == 0
    assert kv2["bam_gpu_level"] == "2"
    assert "bam_gpu_level" not in kv1 and "bam_gpu_level" not in kv0 and "bam_gpu_pieces" not in kv0
