"""fc2_gpu_gzip: one buffer through the host path of spliced_reads.fastq.gz's device mode
(csrc/fc2_deflate_gpu.hip: two pieces in flight, every tile wrapped as a gzip member).  Any gzip
reader must see the input again, in ceil(n / tile) members, within the stated bound; an output buffer
one byte short is an error, not a write past its end."""
import ctypes
import gzip
import zlib

import numpy as np
import pytest

from deflate_helpers import fastq_text
from find_circ2_amd import _native as N

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_RANGE = -4
GUARD = 0xA5


@pytest.fixture(scope="module")
def inputs():
    big = fastq_text(1 << 20, seed=5) * 9        # 9 MiB: three pieces, two in flight
    return {"empty": b"", "one": b"Q", "fastq100k": fastq_text(100 << 10), "text9m": big}


def _gpu_gzip(data: bytes, tile: int, cap=None):
    L = N.lib()
    bound = int(L.fc2_gpu_gzip_bound(len(data), tile))
    cap = bound if cap is None else cap
    out = (ctypes.c_uint8 * (cap + 1))()
    out[cap] = GUARD
    n = ctypes.c_uint64(0)
    src = ctypes.create_string_buffer(data, len(data)) if data else None
    rc = L.fc2_gpu_gzip(0, src, len(data), tile, out, cap, ctypes.byref(n))
    assert out[cap] == GUARD, "a byte past the buffer was written"
    return rc, bytes(bytearray(out)[:int(n.value)]), bound


def _members(blob: bytes, tile: int):
    """Members walked one at a time (each is fed at most its largest possible size)."""
    k, pos = 0, 0
    while pos < len(blob):
        z = zlib.decompressobj(31)
        fed = blob[pos:pos + tile + 128]
        z.decompress(fed)
        assert z.eof
        pos += len(fed) - len(z.unused_data)
        k += 1
    return k


@pytest.mark.parametrize("tile", [32768, 65536, 997])
@pytest.mark.parametrize("name", ["empty", "one", "fastq100k", "text9m"])
def test_gpu_gzip_round_trip(inputs, name, tile):
    data = inputs[name]
    rc, out, bound = _gpu_gzip(data, tile)
    assert rc == 0
    assert 0 < len(out) <= bound
    assert gzip.decompress(out) == data
    assert _members(out, tile) == max(1, -(-len(data) // tile))


@pytest.mark.parametrize("name", ["empty", "fastq100k"])
def test_gpu_gzip_output_one_byte_short(inputs, name):
    data = inputs[name]
    rc, out, _ = _gpu_gzip(data, 32768)
    assert rc == 0
    rc2, _, _ = _gpu_gzip(data, 32768, cap=len(out) - 1)      # (_gpu_gzip checks the guard byte)
    assert rc2 == E_RANGE
    rc3, out3, _ = _gpu_gzip(data, 32768, cap=len(out))       # exactly enough
    assert rc3 == 0 and out3 == out


def test_gpu_gzip_bad_arguments():
    L = N.lib()
    n = ctypes.c_uint64(0)
    out = (ctypes.c_uint8 * 64)()
    src = ctypes.create_string_buffer(b"abc", 3)
    assert L.fc2_gpu_gzip(0, src, 3, 0, out, 64, ctypes.byref(n)) == -1
    assert L.fc2_gpu_gzip(0, src, 3, 65537, out, 64, ctypes.byref(n)) == -1
    assert L.fc2_gpu_gzip(0, None, 3, 32768, out, 64, ctypes.byref(n)) == -1
    assert L.fc2_gpu_gzip(0, src, 3, 32768, None, 64, ctypes.byref(n)) == -1
