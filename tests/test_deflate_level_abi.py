"""The compressor's level through the entry points that need no GPU: fc2_deflate_launch_level refuses a
level that is not 1 or 2 before it touches a device; the two setters of the writers' level take 1 and 2
and refuse the rest; fc2_ingest_set_bam_out_device_level refuses a call after the device mode is set or
the first record is read (fc2_caller_set_reads_gz_device_level after fc2_caller_set_reads_gz_device needs
a device: test_cli_gpu_level2.py); mode 2 of
spliced_alignments.bam's device mode (zlib on the host) ignores the level; and on the command line
FC2_GPU_GZIP_LEVEL / FC2_GPU_BAM_LEVEL without FC2_GPU_GZIP / FC2_GPU_BAM change no byte of any output
file and nothing in run.log's "process phases" line."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, TESTS
from find_circ2_amd import _native as N
from find_circ2_amd.ingest import NativeIngest
from test_bam_out_pieces_host import write_bam
from test_native_caller import _rich_sam
from test_reads_gz_device_abi import _open, _sam

E_PARAM = -1


def test_launch_level_refuses_other_levels_before_the_device():
    L = N.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    for level in (0, 3, -1):
        assert L.fc2_deflate_launch_level(p, 8, 32768, p, 32768 + 16, p, p, p, None, level) == E_PARAM
        assert b"level" in L.fc2_last_error()
    # the other arguments are checked as fc2_deflate_launch checks them, at either level
    for level in (1, 2):
        assert L.fc2_deflate_launch_level(p, 8, 65537, p, 65537 + 16, p, p, p, None, level) == E_PARAM
        assert L.fc2_deflate_launch_level(p, 8, 32768, p, 32768, p, p, p, None, level) == E_PARAM
        assert L.fc2_deflate_launch_level(p, 0, 32768, p, 32768 + 16, p, p, p, None, level) == 0       # nothing to do
    out_n = ctypes.c_uint64()
    for level in (0, 3):
        assert L.fc2_gpu_gzip_level(0, p, 8, 32768, level, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_bgzf_level(0, p, 8, 0xff00, 0, level, p, 64, ctypes.byref(out_n)) == E_PARAM


def test_reads_gz_level_setter(tmp_path):
    fa, sam = _sam(tmp_path)
    L, nc = _open(sam, reads_gz=(str(tmp_path / "r.fastq.gz"), 1, 1, 0))
    try:
        assert L.fc2_caller_set_reads_gz_device_level(None, 1) == E_PARAM
        for level in (0, 3, -1):
            assert L.fc2_caller_set_reads_gz_device_level(nc.h, level) == E_PARAM
        for level in (2, 1, 2):
            assert L.fc2_caller_set_reads_gz_device_level(nc.h, level) == 0
    finally:
        nc.close()


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("levelabi")
    sam = str(d / "rich.sam")
    fa = _rich_sam(sam, 1500, seed=31)
    return fa, sam


def test_bam_out_level_setter(rich, tmp_path):
    fa, sam = rich
    L = N.lib()
    ing = NativeIngest(sam, False)
    assert L.fc2_ingest_set_bam_out_device_level(None, 2) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == E_PARAM               # before fc2_ingest_set_bam_out
    ing.set_bam_out(str(tmp_path / "a.bam"))
    for level in (0, 3, -1):
        assert L.fc2_ingest_set_bam_out_device_level(ing.h, level) == E_PARAM
    for level in (2, 1, 2):
        assert L.fc2_ingest_set_bam_out_device_level(ing.h, level) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == 0
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == E_PARAM               # after the device mode is set
    ing.close()
    # after the first record the setter is refused, as fc2_ingest_set_bam_out_device is
    ing = NativeIngest(sam, False)
    ing.set_bam_out(str(tmp_path / "b.bam"))
    ing.next_chunk(15, False, False, 50)
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == E_PARAM
    ing.close()


def test_host_model_ignores_the_level(rich, tmp_path):
    fa, sam = rich
    a, b = str(tmp_path / "one.bam"), str(tmp_path / "two.bam")
    assert write_bam(sam, False, a, dict(mode=2)) == write_bam(sam, False, b, dict(mode=2, level=2))
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 100000


def _cli(fa, sam, out, env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, TESTS]))
    for k in ("FC2_GPU_GZIP", "FC2_GPU_BAM", "FC2_GPU_GZIP_LEVEL", "FC2_GPU_BAM_LEVEL"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "cli_oracle_main.py"), "-G", fa, "-o", out, "-n", "k", "-q",
                        "--threads", "1", "-B", sam], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f != "run.log"}
    line = [l for l in open(os.path.join(out, "run.log")) if "process phases" in l][0]
    return files, re.findall(r"(\w+)=", line.split("process phases: ")[1])


def test_cli_levels_alone_change_nothing(rich, tmp_path):
    fa, sam = rich
    files0, keys0 = _cli(fa, sam, str(tmp_path / "unset"), {})
    files2, keys2 = _cli(fa, sam, str(tmp_path / "levels"), {"FC2_GPU_GZIP_LEVEL": "2", "FC2_GPU_BAM_LEVEL": "2"})
    assert {"spliced_reads.fastq.gz", "spliced_alignments.bam"} <= set(files0) and len(files0["spliced_alignments.bam"]) > 100000
    assert files2 == files0
    assert keys2 == keys0 and not [k for k in keys0 if k.endswith("_level")]
