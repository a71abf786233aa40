"""Level 2's search effort through the entry points that need no GPU: fc2_deflate_launch_deep, fc2_gpu_gzip_deep and
fc2_gpu_bgzf_deep refuse a depth outside 1..128 and a nice outside 4..258 -- and whatever the existing entries
refuse -- before they touch a device; the two setters refuse the same values, a call while the level is 1, and the
calls their level setters refuse; a level set back to 1 behind a search makes the device call itself FC2_E_PARAM;
mode 2 of spliced_alignments.bam's device mode ignores the search as it ignores the level; and on the command
line FC2_GPU_GZIP_DEPTH / _NICE and FC2_GPU_BAM_DEPTH / _NICE without FC2_GPU_GZIP / FC2_GPU_BAM change no byte of
any output file and no key of run.log's "process phases" line."""
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
BAD = ((0, 32), (129, 32), (0xFFFFFFFF, 32), (8, 3), (8, 259), (8, 0), (0, 0), (8, 0xFFFFFFFF))
GOOD = ((1, 4), (8, 32), (32, 258), (128, 258))


def test_launch_deep_refuses_before_the_device():
    L = N.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    for group in (0, 0xff00):
        for depth, nice in BAD:
            assert L.fc2_deflate_launch_deep(p, 8, group, 16320, 32768, p, 16320 + 16, p, p, p, None, depth, nice) == E_PARAM
            assert b"depth" in L.fc2_last_error()
        for depth, nice in GOOD:
            # the other arguments are checked as the existing entries check them
            assert L.fc2_deflate_launch_deep(p, 8, group, 65537, 0, p, 65537 + 16, p, p, p, None, depth, nice) == E_PARAM
            assert L.fc2_deflate_launch_deep(p, 8, group, 0, 0, p, 16, p, p, p, None, depth, nice) == E_PARAM
            assert L.fc2_deflate_launch_deep(p, 8, group, 32768, 32769, p, 32768 + 16, p, p, p, None, depth, nice) == E_PARAM
            assert L.fc2_deflate_launch_deep(p, 8, group, 40000, 30000, p, 40000 + 16, p, p, p, None, depth, nice) == E_PARAM
            assert L.fc2_deflate_launch_deep(p, 8, group, 32768, 0, p, 32768, p, p, p, None, depth, nice) == E_PARAM   # stride
            assert L.fc2_deflate_launch_deep(p, 0, group, 32768, 0, p, 32768 + 16, p, p, p, None, depth, nice) == 0   # nothing to do
    out_n = ctypes.c_uint64()
    for depth, nice in BAD:
        assert L.fc2_gpu_gzip_deep(0, p, 8, 32768, 0, depth, nice, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_bgzf_deep(0, p, 8, 0xff00, 0, 0, 0, depth, nice, p, 64, ctypes.byref(out_n)) == E_PARAM
    for depth, nice in GOOD:
        assert L.fc2_gpu_gzip_deep(0, p, 8, 65537, 0, depth, nice, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_gzip_deep(0, p, 8, 40000, 30000, depth, nice, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_gzip_deep(-1, p, 8, 32768, 0, depth, nice, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_bgzf_deep(0, p, 8, 0xff01, 0, 0, 0, depth, nice, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_bgzf_deep(0, p, 8, 0xff00, 0, 100, 0, depth, nice, p, 64, ctypes.byref(out_n)) == E_PARAM   # 653 tiles
        assert L.fc2_gpu_bgzf_deep(0, p, 8, 0xff00, 0, 16320, 32769, depth, nice, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_bgzf_deep(0, p, 0, 0xff00, 0, 0, 0, depth, nice, p, 64, ctypes.byref(out_n)) == 0 and out_n.value == 0


def test_reads_gz_search_setter(tmp_path):
    fa, sam = _sam(tmp_path)
    L, nc = _open(sam, reads_gz=(str(tmp_path / "r.fastq.gz"), 1, 1, 0))
    try:
        assert L.fc2_caller_set_reads_gz_device_search(None, 32, 258) == E_PARAM
        assert L.fc2_caller_set_reads_gz_device_search(nc.h, 32, 258) == E_PARAM       # the level is 1
        assert b"level 2" in L.fc2_last_error()
        assert L.fc2_caller_set_reads_gz_device_level(nc.h, 2) == 0
        for depth, nice in BAD:
            assert L.fc2_caller_set_reads_gz_device_search(nc.h, depth, nice) == E_PARAM
        for depth, nice in GOOD:
            assert L.fc2_caller_set_reads_gz_device_search(nc.h, depth, nice) == 0
        # the level set back to 1 behind a search: the device call is refused before a device is needed
        assert L.fc2_caller_set_reads_gz_device_level(nc.h, 1) == 0
        assert L.fc2_caller_set_reads_gz_device(nc.h, 0) == E_PARAM
        assert b"level 2" in L.fc2_last_error()
        assert L.fc2_caller_set_reads_gz_device_search(nc.h, 32, 258) == E_PARAM
    finally:
        nc.close()


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("deepabi")
    sam = str(d / "rich.sam")
    fa = _rich_sam(sam, 1500, seed=31)
    return fa, sam


def test_bam_out_search_setter(rich, tmp_path):
    fa, sam = rich
    L = N.lib()
    ing = NativeIngest(sam, False)
    assert L.fc2_ingest_set_bam_out_device_search(None, 32, 258) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device_search(ing.h, 32, 258) == E_PARAM          # before fc2_ingest_set_bam_out
    ing.set_bam_out(str(tmp_path / "a.bam"))
    assert L.fc2_ingest_set_bam_out_device_search(ing.h, 32, 258) == E_PARAM          # the level is 1
    assert b"level 2" in L.fc2_last_error()
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == 0
    for depth, nice in BAD:
        assert L.fc2_ingest_set_bam_out_device_search(ing.h, depth, nice) == E_PARAM
    for depth, nice in GOOD:
        assert L.fc2_ingest_set_bam_out_device_search(ing.h, depth, nice) == 0
    # the level set back to 1 behind a search: both device modes are refused, mode 0 (off) is not
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 1) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 1, 0, 0, 0, 0.0) == E_PARAM
    assert b"level 2" in L.fc2_last_error()
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == 0
    assert L.fc2_ingest_set_bam_out_device_search(ing.h, 32, 258) == E_PARAM          # after the device mode is set
    ing.close()
    # after the first record the setter is refused, as the level's is
    ing = NativeIngest(sam, False)
    ing.set_bam_out(str(tmp_path / "b.bam"))
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == 0
    ing.next_chunk(15, False, False, 50)
    assert L.fc2_ingest_set_bam_out_device_search(ing.h, 32, 258) == E_PARAM
    ing.close()


def test_the_python_layer_hands_the_search_over_and_the_library_refuses(rich, tmp_path):
    fa, sam = rich
    for dev in (dict(mode=2, depth=32, nice=258), dict(mode=2, level=2, depth=129), dict(mode=2, level=2, nice=3),
                dict(mode=2, level=2, depth=-1)):
        with pytest.raises(N.Fc2Error) as e:
            write_bam(sam, False, str(tmp_path / "x.bam"), dev)
        assert "fc2_ingest_set_bam_out_device_search" in str(e.value)


def test_host_model_ignores_the_search(rich, tmp_path):
    fa, sam = rich
    a, b = str(tmp_path / "one.bam"), str(tmp_path / "two.bam")
    assert write_bam(sam, False, a, dict(mode=2)) == write_bam(sam, False, b, dict(mode=2, level=2, depth=32, nice=258))
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 100000


VARS = ("FC2_GPU_GZIP_DEPTH", "FC2_GPU_GZIP_NICE", "FC2_GPU_BAM_DEPTH", "FC2_GPU_BAM_NICE")


def _cli(fa, sam, out, env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, TESTS]))
    for k in ("FC2_GPU_GZIP", "FC2_GPU_BAM", "FC2_GPU_GZIP_LEVEL", "FC2_GPU_BAM_LEVEL") + VARS:
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "cli_oracle_main.py"), "-G", fa, "-o", out, "-n", "k", "-q",
                        "--threads", "1", "-B", sam], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f != "run.log"}
    line = [l for l in open(os.path.join(out, "run.log")) if "process phases" in l][0]
    return files, re.findall(r"(\w+)=", line.split("process phases: ")[1])


def test_cli_search_variables_alone_change_nothing(rich, tmp_path):
    fa, sam = rich
    files0, keys0 = _cli(fa, sam, str(tmp_path / "unset"), {})
    # (values the library would refuse among them: without the writers nothing reads them)
    files2, keys2 = _cli(fa, sam, str(tmp_path / "search"), {"FC2_GPU_GZIP_DEPTH": "32", "FC2_GPU_GZIP_NICE": "258",
                                                            "FC2_GPU_BAM_DEPTH": "999", "FC2_GPU_BAM_NICE": "x",
                                                            "FC2_GPU_GZIP_LEVEL": "2", "FC2_GPU_BAM_LEVEL": "2"})
    assert {"spliced_reads.fastq.gz", "spliced_alignments.bam"} <= set(files0) and len(files0["spliced_alignments.bam"]) > 100000
    assert files2 == files0
    assert keys2 == keys0 and not [k for k in keys0 if k.endswith(("_depth", "_nice", "_level"))]


def test_search_env_reads_both_or_neither(monkeypatch):
    from find_circ2_amd import cli
    for k in VARS:
        monkeypatch.delenv(k, raising=False)
    assert cli._search_env("FC2_GPU_BAM") is None and cli._search_note("bam", None) == ""
    monkeypatch.setenv("FC2_GPU_BAM_DEPTH", "")
    monkeypatch.setenv("FC2_GPU_BAM_NICE", "")
    assert cli._search_env("FC2_GPU_BAM") is None
    monkeypatch.setenv("FC2_GPU_BAM_DEPTH", "32")
    assert cli._search_env("FC2_GPU_BAM") == (32, 32) and cli._search_env("FC2_GPU_GZIP") is None
    monkeypatch.setenv("FC2_GPU_BAM_NICE", "258")
    monkeypatch.setenv("FC2_GPU_BAM_DEPTH", "")
    assert cli._search_env("FC2_GPU_BAM") == (8, 258)
    assert cli._search_note("bam", (32, 258)) == ", bam_gpu_depth=32, bam_gpu_nice=258"
