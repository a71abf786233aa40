"""The command line with -B, FC2_GPU_BAM=1 and tiles inside the blocks (FC2_GPU_BAM_TILE=16320,
FC2_GPU_BAM_HISTORY=32768), at the compressor's level 1 and 2: the inflated BAM stream is the default run's, the
blocks are cut where the default run cuts them, every other output file is byte-identical, and run.log names the
tile and the history and counts the pieces, all from the device."""
import os

import pytest

from bgzf_helpers import EOF_BLOCK, read_bam
from samgen import sam_to_bam
from test_cli_gpu_bam import _phases, _run
from test_native_caller import _rich_sam

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("clibamtiles")
    sam = str(d / "rich.sam")
    fa = _rich_sam(sam, 1500, seed=31)
    bam = str(d / "rich.bam")
    sam_to_bam(open(sam).read(), bam)
    return fa, bam


@pytest.mark.parametrize("level", ("1", "2"))
def test_cli_bam_blocks_in_tiles_on_the_gpu(tmp_path, monkeypatch, rich, level):
    from test_cli_gpu import _compare
    fa, bam = rich
    for k in ("FC2_GPU_BAM", "FC2_GPU_BAM_LEVEL", "FC2_GPU_BAM_TILE", "FC2_GPU_BAM_HISTORY"):
        monkeypatch.delenv(k, raising=False)
    o0 = _run(tmp_path, fa, bam, "unset")
    monkeypatch.setenv("FC2_GPU_BAM", "1")
    monkeypatch.setenv("FC2_GPU_BAM_LEVEL", level)
    o1 = _run(tmp_path, fa, bam, "untiled")
    monkeypatch.setenv("FC2_GPU_BAM_TILE", "16320")
    monkeypatch.setenv("FC2_GPU_BAM_HISTORY", "32768")
    o2 = _run(tmp_path, fa, bam, "tiles")
    _compare(o2, o0)
    p0, p1, p2 = (os.path.join(o, "spliced_alignments.bam") for o in (o0, o1, o2))
    blocks0, data0, rec0 = read_bam(p0)
    blocks2, data2, rec2 = read_bam(p2)
    assert data2 == data0 and len(data0) - rec0 > 400000
    assert [b[3] for b in blocks2] == [b[3] for b in blocks0] and all(b[0] <= 65536 for b in blocks2)
    assert blocks2[0] == blocks0[0] and open(p2, "rb").read().endswith(EOF_BLOCK)
    assert open(p2, "rb").read() != open(p1, "rb").read()        # (the payloads are the tiles')
    line = [l for l in open(os.path.join(o2, "run.log")) if "process phases" in l][0]
    assert "bam_gpu_tile=16320, bam_gpu_history=32768" in line
    assert ("bam_gpu_level=2" in line) == (level == "2")
    kv = _phases(o2)
    assert float(kv["bam_gpu_pieces"]) > 0 and float(kv["bam_cpu_pieces"]) == 0
    assert "bam_gpu_tile" not in _phases(o1) and "bam_gpu_tile" not in _phases(o0)
