"""The command line with -B and spliced_alignments.bam's records encoded from the SAM input's lines on the GPU
(FC2_GPU_BAM_ENCODE=1), on the rich SAM and on its BAM: the file is the default run's byte for byte -- with the
zlib writer, and with FC2_GPU_BAM=1 the file of FC2_GPU_BAM=1 alone -- every other output file is equal,
run.log counts the batches; a line with an `f` tag sends its batch to the host and changes no byte; on the BAM
input nothing changes and nothing is counted; at 0, at 2 and unset the stage is off."""
import os

import pytest

from find_circ2_amd import cli
from samgen import sam_to_bam
from test_native_caller import _rich_sam

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("clienc")
    sam = str(d / "rich.sam")
    fa = _rich_sam(sam, 1500, seed=31)
    bam = str(d / "rich.bam")
    sam_to_bam(open(sam).read(), bam)
    # the same with an `f` tag on the lines of the read whose record is the middle one -B writes
    from test_sam_encode_writer_host import _tagged, write_bam
    mode0 = str(d / "mode0.bam")
    assert write_bam(sam, False, mode0) == ((0, 0), None)
    return fa, {"sam": sam, "bam": bam, "ftag": _tagged((d, sam, mode0), d, b"XF:f:0.5")}


def _run(tmp_path, fa, inp, tag):
    out = str(tmp_path / tag)
    assert cli.main(["-G", fa, "-o", out, "-n", "test", "-q", "-B", inp], evaluator_factory=None) == 0
    return out


def _phases(o):
    line = [l for l in open(os.path.join(o, "run.log")) if "process phases" in l][0]
    return dict(x.split("=") for x in line.split("process phases: ")[1].strip().split(", "))


def _bam(o):
    return open(os.path.join(o, "spliced_alignments.bam"), "rb").read()


def test_cli_bam_records_encoded_on_the_gpu(tmp_path, monkeypatch, rich):
    from test_cli_gpu import _compare
    fa, inputs = rich
    monkeypatch.delenv("FC2_GPU_BAM", raising=False)
    monkeypatch.delenv("FC2_GPU_BAM_ENCODE", raising=False)
    o0 = _run(tmp_path, fa, inputs["sam"], "unset")
    monkeypatch.setenv("FC2_GPU_BAM_ENCODE", "1")
    o1 = _run(tmp_path, fa, inputs["sam"], "on")
    _compare(o1, o0)
    assert _bam(o1) == _bam(o0) and len(_bam(o0)) > 100000
    kv = _phases(o1)
    assert float(kv["bam_enc_gpu_batches"]) > 0 and float(kv["bam_enc_host_batches"]) == 0
    assert "bam_enc_gpu_batches" not in _phases(o0) and "bam_gpu_pieces" not in kv
    for value in ("0", "2"):
        monkeypatch.setenv("FC2_GPU_BAM_ENCODE", value)
        o = _run(tmp_path, fa, inputs["sam"], "at_" + value)
        assert _bam(o) == _bam(o0) and "bam_enc_gpu_batches" not in _phases(o)


def test_cli_encode_in_front_of_the_gpu_bgzf_writer(tmp_path, monkeypatch, rich):
    from test_cli_gpu import _compare
    fa, inputs = rich
    monkeypatch.setenv("FC2_GPU_BAM", "1")
    monkeypatch.delenv("FC2_GPU_BAM_ENCODE", raising=False)
    o0 = _run(tmp_path, fa, inputs["sam"], "bgzf")
    monkeypatch.setenv("FC2_GPU_BAM_ENCODE", "1")
    o1 = _run(tmp_path, fa, inputs["sam"], "both")
    _compare(o1, o0)
    assert _bam(o1) == _bam(o0)
    kv = _phases(o1)
    assert float(kv["bam_enc_gpu_batches"]) > 0 and float(kv["bam_enc_host_batches"]) == 0
    assert float(kv["bam_gpu_pieces"]) > 0 and float(kv["bam_cpu_pieces"]) == 0


def test_cli_bam_input_is_untouched(tmp_path, monkeypatch, rich):
    from test_cli_gpu import _compare
    fa, inputs = rich
    monkeypatch.delenv("FC2_GPU_BAM", raising=False)
    monkeypatch.delenv("FC2_GPU_BAM_ENCODE", raising=False)
    o0 = _run(tmp_path, fa, inputs["bam"], "unset")
    monkeypatch.setenv("FC2_GPU_BAM_ENCODE", "1")
    o1 = _run(tmp_path, fa, inputs["bam"], "on")
    _compare(o1, o0)
    assert _bam(o1) == _bam(o0)
    assert "bam_enc_gpu_batches" not in _phases(o1) and "bam_enc_host_batches" not in _phases(o1)


def test_cli_an_f_tag_goes_to_the_host(tmp_path, monkeypatch, rich):
    from test_cli_gpu import _compare
    fa, inputs = rich
    monkeypatch.delenv("FC2_GPU_BAM", raising=False)
    monkeypatch.delenv("FC2_GPU_BAM_ENCODE", raising=False)
    o0 = _run(tmp_path, fa, inputs["ftag"], "unset")
    assert b"XFf" in __import__("gzip").decompress(_bam(o0))          # (a tagged line is among those written)
    monkeypatch.setenv("FC2_GPU_BAM_ENCODE", "1")
    o1 = _run(tmp_path, fa, inputs["ftag"], "on")
    _compare(o1, o0)
    assert _bam(o1) == _bam(o0)
    assert float(_phases(o1)["bam_enc_host_batches"]) >= 1
