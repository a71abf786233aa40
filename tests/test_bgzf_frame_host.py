"""fc2_bgzf_frame_host (csrc/fc2_bgzf_frame_impl.h through its host entry): the BGZF form of the slots the
GPU DEFLATE compressor fills, against a Python restatement of the rule on slots of arbitrary bytes -- every
destination alignment, a tile of the stored form's length, a short last tile, a canary after the output, each
invalid out_len, a refused tile size -- and on real raw DEFLATE streams, which any gzip reader must take.  A
stand-alone program runs the alignment sweep on the header itself under ASan and UBSan."""
import ctypes
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from bgzf_helpers import (CANARY, E_PARAM, SWEEP_TILES, check_blocks, frame_py, invalid_lengths, stride_of,
                          sweep_case, tile_bound)
from conftest import ROOT
from find_circ2_amd import _native as N


def frame_host(slots, stride, out_len, crc, n_bytes, tile, room):
    """(rc, the `room` output bytes and the 64 canary bytes after them, off, total)."""
    n = len(out_len)
    out = np.full(room + 64, CANARY, np.uint8)
    off = np.full(n + 1, 0xDEADBEEF, np.uint32)
    total = ctypes.c_uint32(0xDEADBEEF)
    slots, out_len, crc = np.ascontiguousarray(slots), np.ascontiguousarray(out_len, np.uint32), np.ascontiguousarray(crc, np.uint32)
    rc = N.lib().fc2_bgzf_frame_host(slots.ctypes.data, stride, out_len.ctypes.data, crc.ctypes.data, n, n_bytes, tile,
                                     out.ctypes.data, off.ctypes.data, ctypes.addressof(total))
    return rc, out, off, int(total.value)


@pytest.mark.parametrize("n_tiles", SWEEP_TILES)
def test_frame_host_follows_the_rule(n_tiles):
    slots, stride, out_len, crc, n_bytes, tile = sweep_case(n_tiles)
    want, want_off, want_total = frame_py(slots, stride, [int(x) for x in out_len], [int(x) for x in crc], n_bytes, tile)
    assert want_total == sum(26 + int(x) for x in out_len) and (n_tiles < 16 or len({o % 16 for o in want_off}) == 16)
    rc, out, off, total = frame_host(slots, stride, out_len, crc, n_bytes, tile, want_total)
    assert rc == 0 and total == want_total
    assert [int(x) for x in off] == want_off
    assert out[:total].tobytes() == want
    assert (out[total:] == CANARY).all(), "bytes after total were written"


@pytest.mark.parametrize("n_tiles", [1, 65])
def test_frame_host_invalid_tile_leaves_the_output_unwritten(n_tiles):
    slots, stride, out_len, crc, n_bytes, tile = sweep_case(n_tiles)
    for bad in invalid_lengths(tile):
        for at in sorted({0, n_tiles // 3, n_tiles - 1}):
            ln = out_len.copy()
            ln[at] = bad
            rc, out, off, total = frame_host(slots, stride, ln, crc, n_bytes, tile, n_tiles * (26 + tile_bound(tile)))
            assert rc == 0 and total == 0 and not off.any()
            assert (out == CANARY).all(), "an unwritten piece was written"


def test_frame_host_refuses_what_cannot_be_a_piece():
    slots, stride, out_len, crc, n_bytes, tile = sweep_case(2)
    big = 0xff00 + 1                             # a block of 0xff01 input bytes could exceed 64 KiB
    s = np.zeros(2 * stride_of(big), np.uint8)
    for args in [(s, stride_of(big), out_len, crc, big + 1, big),         # the tile size
                 (slots, stride, out_len, crc, n_bytes, 0),
                 (slots, stride, out_len, crc, 2 * tile + 1, tile),       # n_bytes past the last tile
                 (slots, stride, out_len, crc, tile, tile),               # ... and before it
                 (slots, tile_bound(tile) - 1, out_len, crc, n_bytes, tile)]:
        rc, out, off, total = frame_host(*args, room=4096)
        assert rc == E_PARAM and total == 0
        assert (out == CANARY).all()
    # the largest tile is taken: its stored form is a block of 65280 + 5 + 26 = 65311 bytes
    ln = np.array([0xff00 + 5], np.uint32)
    rc, out, off, total = frame_host(np.zeros(stride_of(0xff00), np.uint8), stride_of(0xff00), ln, crc[:1], 0xff00, 0xff00, 65311)
    assert rc == 0 and total == 65311 and (out[total:] == CANARY).all()
    assert int(out[16]) | int(out[17]) << 8 == 65310


@pytest.mark.parametrize("tile", [0xff00, 1000, 37])
def test_frame_host_real_streams_read_back(tile):
    rng = np.random.default_rng(5)
    text = b"".join(b"chr%d\t%d\t%d\tname_%d\t+\n" % (rng.integers(1, 23), p, p + 100, k)
                    for k, p in enumerate(rng.integers(0, 10**8, 6000)))
    data = text[:3 * tile + tile // 2 + 1] if tile > 1000 else text[:41 * tile + 3]
    tiles = [data[i:i + tile] for i in range(0, len(data), tile)]
    stride = stride_of(tile)
    slots = np.full(len(tiles) * stride, 0xEE, np.uint8)
    ln, cr = [], []
    for i, t in enumerate(tiles):
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        s = z.compress(t) + z.flush()
        assert len(s) <= tile_bound(tile)
        slots[i * stride:i * stride + len(s)] = np.frombuffer(s, np.uint8)
        ln.append(len(s))
        cr.append(zlib.crc32(t))
    room = sum(26 + x for x in ln)
    rc, out, off, total = frame_host(slots, stride, ln, cr, len(data), tile, room)
    assert rc == 0 and total == room and (out[total:] == CANARY).all()
    blocks = check_blocks(out[:total].tobytes(), data, tile)
    assert [b[0] for b in blocks] == [26 + x for x in ln]
    assert [int(x) for x in off] == list(np.cumsum([0] + [b[0] for b in blocks]))


def test_frame_header_alone_under_sanitizers(tmp_path):
    """tests/c/bgzf_frame_main.cpp: the header's own sweep, compiled for the host with ASan and UBSan."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bgzf_frame_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "c", "bgzf_frame_main.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0 and (b"asan" in r.stdout.lower() or b"ubsan" in r.stdout.lower() or b"sanitize" in r.stdout.lower()):
        pytest.skip("the sanitizer runtime is absent")
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert b"ok" in r.stdout
