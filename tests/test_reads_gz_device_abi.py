"""The entry points of spliced_reads.fastq.gz's device mode that need no GPU: argument checks of
fc2_caller_set_reads_gz_device (nothing touches a device before them), the size functions, and the
default -- without FC2_GPU_GZIP the command line writes the bytes it writes with FC2_GPU_GZIP=0."""
import ctypes
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT, TESTS
from find_circ2_amd import _native as N

E_PARAM = -1


def _sam(tmp_path):
    from bwa_emul import read_fasta
    from test_cli import _reads, sam_text
    fa = os.path.join(GOLDEN, "CDR1as_locus.fa")
    sam = str(tmp_path / "in.sam")
    open(sam, "w").write(sam_text(read_fasta(fa), _reads(os.path.join(GOLDEN, "cdr1as_reads.fa"))))
    return fa, sam


def _open(sam, reads_gz=None):
    from find_circ2_amd.caller import CallerOptions
    from find_circ2_amd.native_caller import NativeCaller
    nc = NativeCaller(sam, False, CallerOptions(), ["CDR1as_locus"], genome_dummy=True, reads_gz=reads_gz)
    nc.open()
    return N.lib(), nc


def test_set_reads_gz_device_needs_the_file_first(tmp_path):
    fa, sam = _sam(tmp_path)
    L, nc = _open(sam)
    try:
        assert L.fc2_caller_set_reads_gz_device(nc.h, 0) == E_PARAM
        assert nc.reads_gz_counts() == (0, 0)
        assert L.fc2_caller_set_reads_gz_device_tuning(nc.h, 65537, 0.0) == E_PARAM
        assert L.fc2_caller_set_reads_gz_device_tuning(nc.h, 997, -1.0) == E_PARAM
        assert L.fc2_caller_set_reads_gz_device_tuning(nc.h, 997, 5.0) == 0
    finally:
        nc.close()


def test_set_reads_gz_device_after_the_first_submit(tmp_path):
    fa, sam = _sam(tmp_path)
    L, nc = _open(sam, reads_gz=(str(tmp_path / "r.fastq.gz"), 1, 1, 0))
    try:
        b, eof = N.CallerBatch(), ctypes.c_int(0)
        N.check(L.fc2_caller_next(nc.h, ctypes.byref(b), ctypes.byref(eof)))
        res = (ctypes.c_uint64 * max(1, int(b.n)))()              # fc2_result, all zero: no hit
        N.check(L.fc2_caller_submit(nc.h, res, None, 0, 0))
        assert L.fc2_caller_set_reads_gz_device(nc.h, 0) == E_PARAM
        assert "before" in N.lib().fc2_last_error().decode()
    finally:
        nc.close()


def test_null_handle():
    L = N.lib()
    assert L.fc2_caller_set_reads_gz_device(None, 0) == E_PARAM
    assert L.fc2_caller_reads_gz_counts(None, None, None) == E_PARAM
    assert L.fc2_caller_set_reads_gz_device_tuning(None, 0, 0.0) == E_PARAM


def test_size_functions_are_monotone():
    L = N.lib()
    for tile in (1, 100, 997, 32768, 65536):
        sizes = [0, 1, 2, tile - 1, tile, tile + 1, 3 * tile, 3 * tile + 1, 10 << 20]
        sizes = sorted(set(s for s in sizes if s >= 0))
        sc = [int(L.fc2_deflate_scratch_bytes(n, tile)) for n in sizes]
        bd = [int(L.fc2_gpu_gzip_bound(n, tile)) for n in sizes]
        assert sc == sorted(sc) and bd == sorted(bd)
        assert all(s > 0 for n, s in zip(sizes, sc) if n > 0)
        assert all(b > 0 for b in bd)            # (an empty input still takes one empty member)
        # a token of 4 bytes per input byte fits; a member per tile fits
        assert all(s >= 4 * n for n, s in zip(sizes, sc))
        assert all(b >= n + 18 * max(1, -(-n // tile)) for n, b in zip(sizes, bd))


def _cli(fa, sam, out, env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, TESTS]))
    e.pop("FC2_GPU_GZIP", None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "cli_oracle_main.py"), "-G", fa, "-o", out, "-n", "k", "-q",
                        "--threads", "1", sam], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return open(os.path.join(out, "spliced_reads.fastq.gz"), "rb").read()


def test_default_writes_the_cpu_writers_bytes(tmp_path):
    fa, sam = _sam(tmp_path)
    a = _cli(fa, sam, str(tmp_path / "unset"), {})
    b = _cli(fa, sam, str(tmp_path / "zero"), {"FC2_GPU_GZIP": "0"})
    assert len(a) > 18 and a == b
