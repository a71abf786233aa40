"""The history of the GPU gzip writer through the entry points that need no GPU: the three symbols exist;
fc2_deflate_launch_hist and fc2_gpu_gzip_hist refuse a tile, history or level outside their rules before they
touch a device; fc2_caller_set_reads_gz_device_history takes 0..32768, and fc2_caller_set_reads_gz_device
refuses a tile and history of more than 65536 bytes together and leaves the CPU writer in place (the setter
after fc2_caller_set_reads_gz_device needs a device: test_cli_gpu_gzip_hist.py); and on the command line
FC2_GPU_GZIP_HISTORY without FC2_GPU_GZIP=1 changes no byte of the reads file and nothing in run.log's
"process phases" line."""
import ctypes
import gzip
import os
import re
import subprocess
import sys

from conftest import ROOT, TESTS
from find_circ2_amd import _native as N
from test_reads_gz_device_abi import _open, _sam

E_PARAM = -1


def test_the_three_symbols_exist():
    L = N.lib()
    for name in ("fc2_deflate_launch_hist", "fc2_gpu_gzip_hist", "fc2_caller_set_reads_gz_device_history"):
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
    assert len(L.fc2_deflate_launch_hist.argtypes) == 11 and len(L.fc2_gpu_gzip_hist.argtypes) == 9


def test_launch_hist_refuses_before_the_device():
    L = N.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    for tile, hist, level in [(0, 0, 1), (65537, 0, 1), (32768, 32769, 1), (32769, 32768, 2), (65536, 1, 1), (8192, 4096, 0),
                              (8192, 4096, 3), (8192, 0, 3), (0xFFFFFFFF, 2, 1), (2, 0xFFFFFFFF, 1)]:
        assert L.fc2_deflate_launch_hist(p, 8, tile, hist, p, (tile + 16) & 0xFFFFFFFF, p, p, p, None, level) == E_PARAM, (tile, hist, level)
        assert b"fc2_deflate_launch_hist" in L.fc2_last_error()
    # the other arguments are checked as fc2_deflate_launch checks them; nothing to do is no error
    for level in (1, 2):
        assert L.fc2_deflate_launch_hist(p, 8, 8192, 4096, p, 8192, p, p, p, None, level) == E_PARAM    # the stride
        assert L.fc2_deflate_launch_hist(p, 8, 8192, 4096, p, 8192 + 16, None, p, p, None, level) == E_PARAM
        assert L.fc2_deflate_launch_hist(p, 0, 8192, 4096, p, 8192 + 16, p, p, p, None, level) == 0
        assert L.fc2_deflate_launch_hist(p, 0, 32768, 32768, p, 32768 + 16, p, p, p, None, level) == 0
    out_n = ctypes.c_uint64()
    for tile, hist, level in [(32768, 32769, 1), (32769, 32768, 1), (8192, 4096, 3), (0, 4096, 1)]:
        assert L.fc2_gpu_gzip_hist(0, p, 8, tile, hist, level, p, 64, ctypes.byref(out_n)) == E_PARAM


def test_reads_gz_history_setter_and_the_sum_of_tile_and_history(tmp_path):
    fa, sam = _sam(tmp_path)
    path = str(tmp_path / "r.fastq.gz")
    L, nc = _open(sam, reads_gz=(path, 1, 1, 0))
    try:
        assert L.fc2_caller_set_reads_gz_device_history(None, 0) == E_PARAM
        for hist in (32769, 65536, 0xFFFFFFFF):
            assert L.fc2_caller_set_reads_gz_device_history(nc.h, hist) == E_PARAM
        for hist in (32768, 0, 1, 4096, 32768):
            assert L.fc2_caller_set_reads_gz_device_history(nc.h, hist) == 0
        # tile 32769 and history 32768: refused before a device is looked for, the CPU writer stays
        assert L.fc2_caller_set_reads_gz_device_tuning(nc.h, 32769, 0.0) == 0
        assert L.fc2_caller_set_reads_gz_device(nc.h, 0) == E_PARAM
        assert b"65536" in L.fc2_last_error()
        assert L.fc2_caller_set_reads_gz_device_tuning(nc.h, 65536, 0.0) == 0
        assert L.fc2_caller_set_reads_gz_device_history(nc.h, 1) == 0
        assert L.fc2_caller_set_reads_gz_device(nc.h, 0) == E_PARAM
        assert L.fc2_caller_set_reads_gz_device_history(nc.h, 4096) == 0      # still before the device mode: taken
        assert nc.reads_gz_counts() == (0, 0)
        N.check(L.fc2_caller_close_reads(nc.h))
    finally:
        nc.close()
    assert gzip.decompress(open(path, "rb").read()) == b""     # the CPU writer's file: one empty member


def _cli(fa, sam, out, env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, TESTS]))
    for k in ("FC2_GPU_GZIP", "FC2_GPU_GZIP_LEVEL", "FC2_GPU_GZIP_HISTORY", "FC2_GPU_GZIP_TILE"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "cli_oracle_main.py"), "-G", fa, "-o", out, "-n", "k", "-q",
                        "--threads", "1", sam], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f != "run.log"}
    line = [l for l in open(os.path.join(out, "run.log")) if "process phases" in l][0]
    return files, re.findall(r"(\w+)=", line.split("process phases: ")[1])


def test_cli_history_alone_leaves_the_cpu_writers_bytes(tmp_path):
    fa, sam = _sam(tmp_path)
    files0, keys0 = _cli(fa, sam, str(tmp_path / "unset"), {})
    for k, env in enumerate(({"FC2_GPU_GZIP_HISTORY": "32768"}, {"FC2_GPU_GZIP_HISTORY": "32768", "FC2_GPU_GZIP": "0"},
                             {"FC2_GPU_GZIP_HISTORY": ""})):
        files, keys = _cli(fa, sam, str(tmp_path / ("hist%d" % k)), env)
        assert files == files0 and len(files0["spliced_reads.fastq.gz"]) > 18
        assert keys == keys0 and not [x for x in keys0 if x.endswith("_history")]
