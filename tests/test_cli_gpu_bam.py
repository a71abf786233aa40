"""The command line with -B and spliced_alignments.bam's records compressed on the GPU (FC2_GPU_BAM=1), on the
rich SAM and on its BAM: the inflated BAM stream is the default run's, the blocks are cut where the default
run cuts them, every other output file is byte-identical, run.log counts the pieces; at 0, at 2 and unset the
file is zlib's, byte for byte."""
import os

import pytest

from bgzf_helpers import EOF_BLOCK, read_bam
from find_circ2_amd import cli
from samgen import sam_to_bam
from test_native_caller import _rich_sam

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("clibam")
    sam = str(d / "rich.sam")
    fa = _rich_sam(sam, 1500, seed=31)
    bam = str(d / "rich.bam")
    sam_to_bam(open(sam).read(), bam)
    return fa, {"sam": sam, "bam": bam}


def _run(tmp_path, fa, inp, tag):
    out = str(tmp_path / tag)
    assert cli.main(["-G", fa, "-o", out, "-n", "test", "-q", "-B", inp], evaluator_factory=None) == 0
    return out


def _phases(o):
    line = [l for l in open(os.path.join(o, "run.log")) if "process phases" in l][0]
    return dict(x.split("=") for x in line.split("process phases: ")[1].strip().split(", "))


@pytest.mark.parametrize("kind", ["sam", "bam"])
def test_cli_bam_records_compressed_on_the_gpu(tmp_path, monkeypatch, rich, kind):
    from test_cli_gpu import _compare
    fa, inputs = rich
    monkeypatch.delenv("FC2_GPU_BAM", raising=False)
    o0 = _run(tmp_path, fa, inputs[kind], "unset")
    monkeypatch.setenv("FC2_GPU_BAM", "1")
    o1 = _run(tmp_path, fa, inputs[kind], "on")
    _compare(o1, o0)
    p0, p1 = (os.path.join(o, "spliced_alignments.bam") for o in (o0, o1))
    blocks0, data0, rec0 = read_bam(p0)
    blocks1, data1, rec1 = read_bam(p1)
    assert data1 == data0 and len(data0) - rec0 > 400000
    assert [b[3] for b in blocks1] == [b[3] for b in blocks0] and all(b[0] <= 65536 for b in blocks1)
    assert blocks1[0] == blocks0[0] and open(p1, "rb").read().endswith(EOF_BLOCK)
    assert open(p1, "rb").read() != open(p0, "rb").read()        # (the payloads are the device's)
    kv = _phases(o1)
    assert float(kv["bam_gpu_pieces"]) > 0 and float(kv["bam_cpu_pieces"]) == 0
    assert "bam_gpu_pieces" not in _phases(o0)
    for value in ("0", "2"):
        monkeypatch.setenv("FC2_GPU_BAM", value)
        o = _run(tmp_path, fa, inputs[kind], "at_" + value)
        assert open(os.path.join(o, "spliced_alignments.bam"), "rb").read() == open(p0, "rb").read()
        assert "bam_gpu_pieces" not in _phases(o)
