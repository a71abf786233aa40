"""Level 2's passes through the entry points that need no GPU: fc2_deflate_launch_priced, fc2_gpu_gzip_priced and
fc2_gpu_bgzf_priced refuse passes outside 1..3 -- and whatever the _deep entries refuse -- before they touch a
device; the two setters refuse the same values, a call while the level is 1, and the calls their level setters refuse;
a level set back to 1 behind the passes makes the device call itself FC2_E_PARAM; mode 2 of spliced_alignments.bam's
device mode ignores the passes as it ignores the level; the headers' constants are the ones the Python layers use;
bgz::level_with_search carries depth, nice and passes in one word; and on the command line FC2_GPU_GZIP_PASSES and
FC2_GPU_BAM_PASSES without FC2_GPU_GZIP / FC2_GPU_BAM change no byte of any output file and no key of run.log's
"process phases" line."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from find_circ2_amd import _native as N
from find_circ2_amd.ingest import NativeIngest
from test_bam_out_pieces_host import write_bam
from test_deflate_deep_abi import BAD, GOOD, _cli
from test_native_caller import _rich_sam
from test_reads_gz_device_abi import _open, _sam

E_PARAM = -1
BAD_PASSES = (0, 4, 5, 0xFFFFFFFF)
GOOD_PASSES = (1, 2, 3)
NEW = ("fc2_deflate_launch_priced", "fc2_gpu_gzip_priced", "fc2_gpu_bgzf_priced", "fc2_caller_set_reads_gz_device_passes",
       "fc2_ingest_set_bam_out_device_passes")


def test_the_new_entries_are_exported_and_the_headers_hold_the_constants():
    L = N.lib()
    for name in NEW:
        assert name in N.EXPORTED and getattr(L, name).argtypes is not None
    caller = open(os.path.join(ROOT, "include", "fc2_caller.h")).read()
    ingest = open(os.path.join(ROOT, "include", "fc2_ingest.h")).read()
    define = lambda text, name: int(re.search(r"#define %s (\d+)u" % name, text).group(1))
    assert (define(caller, "FC2_DEFLATE_PASSES_MIN"), define(caller, "FC2_DEFLATE_PASSES_MAX")) == (1, 3)
    assert (define(caller, "FC2_DEFLATE_LEVEL2_DEPTH"), define(caller, "FC2_DEFLATE_LEVEL2_NICE")) == (8, 32)
    import deflate_model2
    import deflate_model_priced
    assert deflate_model_priced.PASSES_RANGE == (1, 3) and (deflate_model2.DEPTH, deflate_model2.NICE) == (8, 32)
    for name in NEW[:4]:
        assert re.search(r"\b%s\(" % name, caller), name
    assert re.search(r"\bfc2_ingest_set_bam_out_device_passes\(", ingest)


def test_launch_priced_refuses_before_the_device():
    L = N.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    out_n = ctypes.c_uint64()
    for group in (0, 0xff00):
        for passes in BAD_PASSES:
            assert L.fc2_deflate_launch_priced(p, 8, group, 16320, 32768, p, 16320 + 16, p, p, p, None, 8, 32, passes) == E_PARAM
            assert b"passes is 1..3" in L.fc2_last_error()
        for passes in GOOD_PASSES:
            for depth, nice in BAD:                 # the deep entry's refusals, through the new entry
                assert L.fc2_deflate_launch_priced(p, 8, group, 16320, 32768, p, 16320 + 16, p, p, p, None, depth, nice, passes) == E_PARAM
                assert b"depth" in L.fc2_last_error()
            for depth, nice in GOOD:
                a = (depth, nice, passes)
                assert L.fc2_deflate_launch_priced(p, 8, group, 65537, 0, p, 65537 + 16, p, p, p, None, *a) == E_PARAM
                assert L.fc2_deflate_launch_priced(p, 8, group, 0, 0, p, 16, p, p, p, None, *a) == E_PARAM
                assert L.fc2_deflate_launch_priced(p, 8, group, 32768, 32769, p, 32768 + 16, p, p, p, None, *a) == E_PARAM
                assert L.fc2_deflate_launch_priced(p, 8, group, 40000, 30000, p, 40000 + 16, p, p, p, None, *a) == E_PARAM
                assert L.fc2_deflate_launch_priced(p, 8, group, 32768, 0, p, 32768, p, p, p, None, *a) == E_PARAM   # stride
                assert L.fc2_deflate_launch_priced(p, 0, group, 32768, 0, p, 32768 + 16, p, p, p, None, *a) == 0   # nothing to do
    for passes in BAD_PASSES:
        assert L.fc2_gpu_gzip_priced(0, p, 8, 32768, 0, 8, 32, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert b"passes" in L.fc2_last_error()
        assert L.fc2_gpu_bgzf_priced(0, p, 8, 0xff00, 0, 0, 0, 8, 32, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert b"passes" in L.fc2_last_error()
    for passes in GOOD_PASSES:
        for depth, nice in BAD:
            assert L.fc2_gpu_gzip_priced(0, p, 8, 32768, 0, depth, nice, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
            assert L.fc2_gpu_bgzf_priced(0, p, 8, 0xff00, 0, 0, 0, depth, nice, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_gzip_priced(0, p, 8, 65537, 0, 8, 32, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_gzip_priced(0, p, 8, 40000, 30000, 8, 32, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_gzip_priced(-1, p, 8, 32768, 0, 8, 32, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_bgzf_priced(0, p, 8, 0xff01, 0, 0, 0, 8, 32, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_bgzf_priced(0, p, 8, 0xff00, 0, 100, 0, 8, 32, passes, p, 64, ctypes.byref(out_n)) == E_PARAM   # 653 tiles
        assert L.fc2_gpu_bgzf_priced(0, p, 8, 0xff00, 0, 16320, 32769, 8, 32, passes, p, 64, ctypes.byref(out_n)) == E_PARAM
        assert L.fc2_gpu_bgzf_priced(0, p, 0, 0xff00, 0, 0, 0, 8, 32, passes, p, 64, ctypes.byref(out_n)) == 0 and out_n.value == 0


def test_reads_gz_passes_setter(tmp_path):
    fa, sam = _sam(tmp_path)
    L, nc = _open(sam, reads_gz=(str(tmp_path / "r.fastq.gz"), 1, 1, 0))
    try:
        assert L.fc2_caller_set_reads_gz_device_passes(None, 2) == E_PARAM
        assert L.fc2_caller_set_reads_gz_device_passes(nc.h, 2) == E_PARAM       # the level is 1
        assert b"level 2" in L.fc2_last_error()
        assert L.fc2_caller_set_reads_gz_device_level(nc.h, 2) == 0
        for passes in BAD_PASSES:
            assert L.fc2_caller_set_reads_gz_device_passes(nc.h, passes) == E_PARAM
            assert b"1..3" in L.fc2_last_error()
        for passes in GOOD_PASSES:
            assert L.fc2_caller_set_reads_gz_device_passes(nc.h, passes) == 0
        assert L.fc2_caller_set_reads_gz_device_search(nc.h, 32, 258) == 0        # beside a search, in either order
        assert L.fc2_caller_set_reads_gz_device_passes(nc.h, 2) == 0
        # the level set back to 1 behind the passes: the device call is refused before a device is needed
        assert L.fc2_caller_set_reads_gz_device_level(nc.h, 1) == 0
        assert L.fc2_caller_set_reads_gz_device(nc.h, 0) == E_PARAM
        assert b"level 2" in L.fc2_last_error()
        assert L.fc2_caller_set_reads_gz_device_passes(nc.h, 2) == E_PARAM
    finally:
        nc.close()


def test_reads_gz_passes_alone_are_refused_with_the_level_set_back(tmp_path):
    fa, sam = _sam(tmp_path)
    L, nc = _open(sam, reads_gz=(str(tmp_path / "r.fastq.gz"), 1, 1, 0))
    try:
        assert L.fc2_caller_set_reads_gz_device_level(nc.h, 2) == 0
        assert L.fc2_caller_set_reads_gz_device_passes(nc.h, 3) == 0              # (no search set)
        assert L.fc2_caller_set_reads_gz_device_level(nc.h, 1) == 0
        assert L.fc2_caller_set_reads_gz_device(nc.h, 0) == E_PARAM
        assert b"passes need level 2" in L.fc2_last_error()
    finally:
        nc.close()


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("pricedabi")
    sam = str(d / "rich.sam")
    fa = _rich_sam(sam, 1500, seed=31)
    return fa, sam


def test_bam_out_passes_setter(rich, tmp_path):
    fa, sam = rich
    L = N.lib()
    ing = NativeIngest(sam, False)
    assert L.fc2_ingest_set_bam_out_device_passes(None, 2) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device_passes(ing.h, 2) == E_PARAM          # before fc2_ingest_set_bam_out
    ing.set_bam_out(str(tmp_path / "a.bam"))
    assert L.fc2_ingest_set_bam_out_device_passes(ing.h, 2) == E_PARAM          # the level is 1
    assert b"level 2" in L.fc2_last_error()
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == 0
    for passes in BAD_PASSES:
        assert L.fc2_ingest_set_bam_out_device_passes(ing.h, passes) == E_PARAM
        assert b"1..3" in L.fc2_last_error()
    for passes in GOOD_PASSES:
        assert L.fc2_ingest_set_bam_out_device_passes(ing.h, passes) == 0
    assert L.fc2_ingest_set_bam_out_device_passes(ing.h, 2) == 0
    # the level set back to 1 behind the passes: both device modes are refused, mode 0 (off) is not
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 1) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 1, 0, 0, 0, 0.0) == E_PARAM
    assert b"passes need level 2" in L.fc2_last_error()
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == E_PARAM
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == 0
    assert L.fc2_ingest_set_bam_out_device(ing.h, 2, 0, 0, 0, 0.0) == 0
    assert L.fc2_ingest_set_bam_out_device_passes(ing.h, 2) == E_PARAM          # after the device mode is set
    ing.close()
    # after the first record the setter is refused, as the level's is
    ing = NativeIngest(sam, False)
    ing.set_bam_out(str(tmp_path / "b.bam"))
    assert L.fc2_ingest_set_bam_out_device_level(ing.h, 2) == 0
    ing.next_chunk(15, False, False, 50)
    assert L.fc2_ingest_set_bam_out_device_passes(ing.h, 2) == E_PARAM
    ing.close()


def test_the_python_layer_hands_the_passes_over_and_the_library_refuses(rich, tmp_path):
    fa, sam = rich
    for dev in (dict(mode=2, passes=2), dict(mode=2, level=2, passes=4), dict(mode=2, level=2, passes=0),
                dict(mode=2, level=2, passes=-1)):
        with pytest.raises(N.Fc2Error) as e:
            write_bam(sam, False, str(tmp_path / "x.bam"), dev)
        assert "fc2_ingest_set_bam_out_device_passes" in str(e.value)


def test_host_model_ignores_the_passes(rich, tmp_path):
    fa, sam = rich
    a, b = str(tmp_path / "one.bam"), str(tmp_path / "two.bam")
    assert write_bam(sam, False, a, dict(mode=2)) == write_bam(sam, False, b, dict(mode=2, level=2, depth=32, nice=258, passes=3))
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 100000


def test_cli_passes_variables_alone_change_nothing(rich, tmp_path):
    fa, sam = rich
    files0, keys0 = _cli(fa, sam, str(tmp_path / "unset"), {"FC2_GPU_GZIP_PASSES": "", "FC2_GPU_BAM_PASSES": ""})
    # (values the library would refuse among them: without the writers nothing reads them)
    files2, keys2 = _cli(fa, sam, str(tmp_path / "passes"), {"FC2_GPU_GZIP_PASSES": "2", "FC2_GPU_BAM_PASSES": "9",
                                                            "FC2_GPU_GZIP_LEVEL": "2", "FC2_GPU_BAM_LEVEL": "2"})
    assert {"spliced_reads.fastq.gz", "spliced_alignments.bam"} <= set(files0) and len(files0["spliced_alignments.bam"]) > 100000
    assert files2 == files0
    assert keys2 == keys0 and not [k for k in keys0 if k.endswith(("_passes", "_level"))]


def test_passes_env_and_note(monkeypatch):
    from find_circ2_amd import cli
    for k in ("FC2_GPU_BAM_PASSES", "FC2_GPU_GZIP_PASSES"):
        monkeypatch.delenv(k, raising=False)
    assert cli._passes_env("FC2_GPU_BAM") is None and cli._passes_note("bam", None) == ""
    monkeypatch.setenv("FC2_GPU_BAM_PASSES", "")
    assert cli._passes_env("FC2_GPU_BAM") is None
    monkeypatch.setenv("FC2_GPU_BAM_PASSES", "3")
    assert cli._passes_env("FC2_GPU_BAM") == 3 and cli._passes_env("FC2_GPU_GZIP") is None
    monkeypatch.setenv("FC2_GPU_BAM_PASSES", "0")
    assert cli._passes_env("FC2_GPU_BAM") == 0           # (the library refuses it)
    assert cli._passes_note("bam", 1) == "" and cli._passes_note("gzip", 2) == ", gzip_gpu_passes=2"


def test_level_with_search_carries_depth_nice_and_passes(tmp_path):
    """tests/c/level_word_main.cpp prints bgz::level_with_search over a grid; the word is taken apart here as
    bgz::gpu_open takes it apart: the level in bits 0..7, depth in 8..15, nice in 16..24, passes in 25..26."""
    cxx = next((c for c in map(shutil.which, ("g++", "c++", "clang++", "hipcc")) if c), None)
    assert cxx is not None, "no C++ compiler (g++, c++, clang++ or hipcc) to build tests/c/level_word_main.cpp with"
    exe = str(tmp_path / "level_word_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "c", "level_word_main.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(rows) == 5 * 3 * 4
    for depth, nice, passes, word in rows:
        assert 0 < word < 1 << 27
        got = (word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0x1FF, (word >> 25) & 3)
        assert got == (2, depth, nice if depth else 0, passes if passes > 1 else 0), (depth, nice, passes, word)
