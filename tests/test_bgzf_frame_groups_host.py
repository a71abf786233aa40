"""fc2_bgzf_frame_groups_host (csrc/fc2_bgzf_frame_impl.h "groups" through its host entry): BGZF blocks made of
several tiles' streams, against a Python restatement of the rule on slots of arbitrary bytes -- 1, 2, 3 and 65
groups of 1, 2, 4 and 16 tiles, a short last group, a last tile of one byte, a canary after the output -- and on
real streams: the block's CRC-32, combined from the tiles' CRCs and lengths, is zlib's of the group's bytes at
tile lengths 1 .. 65280, and any gzip reader sees the input again.  One invalid out_len, or a block whose valid
tiles sum past 65510, leaves the piece unwritten; one tile a group is fc2_bgzf_frame_host byte for byte; every
argument that cannot be a piece of groups is refused.  A stand-alone program runs the rule and the combine on the
header itself, and the BAM writer's tile-by-tile zlib path, under ASan and UBSan."""
import ctypes
import gzip
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from bgzf_groups_helpers import (SWEEP_GROUPS, SWEEP_TPG, crc_append, frame_groups_py, sweep_case, tiles_of, zlib_slots)
from bgzf_helpers import CANARY, E_PARAM, GAVE_UP, check_blocks, parse_blocks, stride_of, tile_bound
from conftest import ROOT
from find_circ2_amd import _native as N
from test_bgzf_frame_host import frame_host


def frame_groups_host(slots, stride, out_len, crc, n_bytes, group, tile, room, n_tiles=None):
    """(rc, the `room` output bytes and the 64 canary bytes after them, off, total)."""
    n = len(out_len) if n_tiles is None else n_tiles
    n_groups = -(-n_bytes // group) if group else 1
    out = np.full(room + 64, CANARY, np.uint8)
    off = np.full(n_groups + 1, 0xDEADBEEF, np.uint32)
    total = ctypes.c_uint32(0xDEADBEEF)
    slots, out_len, crc = np.ascontiguousarray(slots), np.ascontiguousarray(out_len, np.uint32), np.ascontiguousarray(crc, np.uint32)
    rc = N.lib().fc2_bgzf_frame_groups_host(slots.ctypes.data, stride, out_len.ctypes.data, crc.ctypes.data, n, n_bytes,
                                            group, tile, out.ctypes.data, off.ctypes.data, ctypes.addressof(total))
    return rc, out, off, int(total.value)


def _ints(a):
    return [int(x) for x in a]


def test_crc_append_is_zlibs():
    rng = np.random.default_rng(9)
    a = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
    for n_b in (1, 2, 255, 256, 257, 16320, 65280):
        for n_a in (1, 4097):
            assert crc_append(zlib.crc32(a[:n_a]), zlib.crc32(a[n_a:n_a + n_b]), n_b) == zlib.crc32(a[:n_a + n_b])


@pytest.mark.parametrize("tpg", SWEEP_TPG)
@pytest.mark.parametrize("n_groups", SWEEP_GROUPS)
def test_frame_groups_host_follows_the_rule(n_groups, tpg):
    for last in (None, 7 if tpg == 1 else 64 + 9):                      # a last tile of 1 byte; a short last group
        slots, stride, out_len, crc, n_bytes, group, tile = sweep_case(n_groups, tpg, last)
        want, want_off, want_total = frame_groups_py(slots, stride, _ints(out_len), _ints(crc), n_bytes, group, tile)
        assert want_total == 26 * n_groups + sum(_ints(out_len))
        rc, out, off, total = frame_groups_host(slots, stride, out_len, crc, n_bytes, group, tile, want_total)
        assert rc == 0 and total == want_total
        assert _ints(off) == want_off
        assert out[:total].tobytes() == want
        assert (out[total:] == CANARY).all(), "bytes after total were written"


@pytest.mark.parametrize("group,tile", [(4, 1), (7, 2), (3 * 255 + 1, 255), (1024, 256), (1000, 257), (16320 + 1, 16320),
                                        (16320 + 2, 16320), (16320 + 255, 16320), (16320 + 256, 16320), (16320 + 257, 16320),
                                        (0xff00, 16320), (0xff00, 65280), (0xff00, 0xff00 // 16)])
def test_frame_groups_host_real_streams_read_back(group, tile):
    rng = np.random.default_rng(5)
    text = b"".join(b"chr%d\t%d\t%d\tname_%d\t+\n" % (rng.integers(1, 23), p, p + 100, k)
                    for k, p in enumerate(rng.integers(0, 10**8, 6000)))
    data = text[:2 * group + group // 3 + 1]
    slots, stride, ln, cr = zlib_slots(data, group, tile)
    room = 26 * 3 + sum(ln)
    rc, out, off, total = frame_groups_host(slots, stride, ln, cr, len(data), group, tile, room)
    assert rc == 0 and total == room and (out[total:] == CANARY).all()
    blob = out[:total].tobytes()
    blocks = check_blocks(blob, data, group)        # (the CRC-32 and ISIZE of every block against zlib.crc32)
    assert gzip.decompress(blob) == data
    assert _ints(off) == list(np.cumsum([0] + [b[0] for b in blocks]))
    assert blob == frame_groups_py(slots, stride, ln, cr, len(data), group, tile)[0]


@pytest.mark.parametrize("n_groups,tpg", [(1, 1), (1, 16), (65, 4)])
def test_frame_groups_host_invalid_tile_leaves_the_output_unwritten(n_groups, tpg):
    slots, stride, out_len, crc, n_bytes, group, tile = sweep_case(n_groups, tpg)
    n = len(out_len)
    for bad in (GAVE_UP, 0, tile_bound(tile) + 1):
        for at in sorted({0, n // 3, n - 1}):
            ln = out_len.copy()
            ln[at] = bad
            rc, out, off, total = frame_groups_host(slots, stride, ln, crc, n_bytes, group, tile, n_groups * 65536)
            assert rc == 0 and total == 0 and not off.any()
            assert (out == CANARY).all(), "an unwritten piece was written"


def test_frame_groups_host_a_block_past_64k_leaves_the_piece_unwritten():
    group, tile = 0xff00, 0xff00 // 16              # 16 tiles of 4080 bytes: each may take 4096
    stride = stride_of(tile)
    n_bytes = 2 * group + 5
    n = tiles_of(n_bytes, group, tile)
    assert n == 33
    slots = np.zeros((n + 1) * stride, np.uint8)
    crc = np.arange(n, dtype=np.uint32)
    ln = np.full(n, 100, np.uint32)
    ln[16:32] = [4096] * 15 + [65510 - 15 * 4096]   # the second block: exactly 65536 bytes
    rc, out, off, total = frame_groups_host(slots, stride, ln, crc, n_bytes, group, tile, 3 * 65536)
    assert rc == 0 and total == (26 + 1600) + 65536 + (26 + 100) and _ints(off) == [0, 1626, 1626 + 65536, total]
    ln[31] += 1                                     # every tile valid, the block one byte past 65536
    assert all(0 < int(x) <= tile_bound(tile) for x in ln)
    rc, out, off, total = frame_groups_host(slots, stride, ln, crc, n_bytes, group, tile, 3 * 65536)
    assert rc == 0 and total == 0 and not off.any()
    assert (out == CANARY).all(), "an unwritten piece was written"


@pytest.mark.parametrize("n_groups", SWEEP_GROUPS)
def test_one_tile_a_group_is_fc2_bgzf_frame_host(n_groups):
    _, _, out_len, crc, n_bytes, group, tile = sweep_case(n_groups, 1)
    assert group == tile
    stride = stride_of(tile) + 16                   # (room for a tile that is larger than the group)
    slots = np.random.default_rng(n_groups).integers(0, 256, (n_groups + 1) * stride, dtype=np.uint8)
    room = int(sum(26 + int(x) for x in out_len))
    rc0, want, want_off, want_total = frame_host(slots, stride, out_len, crc, n_bytes, tile, room)
    for t in (tile, tile + 1, stride - 16):         # any tile that holds the group
        rc, out, off, total = frame_groups_host(slots, stride, out_len, crc, n_bytes, group, t, room)
        assert rc0 == rc == 0 and total == want_total == room
        assert np.array_equal(off, want_off) and np.array_equal(out, want)


def test_frame_groups_host_refuses_what_cannot_be_a_piece():
    slots, stride, out_len, crc, n_bytes, group, tile = sweep_case(2, 4)
    n = len(out_len)
    big = np.zeros(70000 * 2, np.uint8)
    for args, kw in [((slots, stride, out_len, crc, n_bytes, 0, tile), {}),                  # the group
                     ((big, stride_of(0xff01), out_len[:2], crc[:2], 0xff01 + 1, 0xff01, 0xff01), {}),
                     ((slots, stride, out_len, crc, n_bytes, group, 0), {}),                 # the tile
                     ((big, 65536 + 32, out_len[:2], crc[:2], 65, 64, 65537), {}),
                     ((slots, stride, out_len, crc, 0, group, tile), {}),                    # no bytes
                     ((slots, stride, out_len, crc, n_bytes, 17 * tile, tile), {"n_tiles": 17}),   # 17 tiles a group
                     ((slots, stride, out_len, crc, n_bytes, group, tile), {"n_tiles": n - 1}),    # not the tiles of n_bytes
                     ((slots, stride, out_len, crc, n_bytes, group, tile), {"n_tiles": n + 1}),
                     ((slots, stride, out_len, crc, n_bytes + group, group, tile), {}),
                     ((slots, tile_bound(tile) - 1, out_len, crc, n_bytes, group, tile), {})]:      # the stride
        rc, out, off, total = frame_groups_host(*args, room=4096, **kw)
        assert rc == E_PARAM and total == 0, args[4:]
        assert (out == CANARY).all()
    # more than 65535 groups
    many = 0x10000
    rc, out, off, total = frame_groups_host(np.zeros(32, np.uint8), 32, np.ones(many, np.uint32), np.zeros(many, np.uint32),
                                            many, 1, 1, 4096)
    assert rc == E_PARAM and total == 0 and (out == CANARY).all()
    L = N.lib()
    t = ctypes.c_uint32(5)
    assert L.fc2_bgzf_frame_groups_host(None, stride, None, None, n, n_bytes, group, tile, None, None, ctypes.addressof(t)) == E_PARAM
    assert t.value == 0
    # 16 tiles of the largest block are taken, stored: 65280 + 16 * 5 + 26 = 65386 bytes
    tile16 = 0xff00 // 16
    ln = np.full(16, tile16 + 5, np.uint32)
    rc, out, off, total = frame_groups_host(np.zeros(17 * stride_of(tile16), np.uint8), stride_of(tile16), ln, np.zeros(16, np.uint32),
                                            0xff00, 0xff00, tile16, 65386)
    assert rc == 0 and total == 65386 and (out[total:] == CANARY).all()
    assert parse_blocks(out[:total].tobytes())[0][3] == 0xff00


def test_groups_host_code_under_sanitizers(tmp_path):
    """tests/c/bgzf_groups_main.cpp: the grouped frame_piece, the CRC combine and the BAM writer's tile-by-tile
    zlib path (mode 2), compiled for the host with ASan and UBSan."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bgzf_groups_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "c", "bgzf_groups_main.cpp"), "-lz"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0 and (b"asan" in r.stdout.lower() or b"ubsan" in r.stdout.lower() or b"sanitize" in r.stdout.lower()):
        pytest.skip("the sanitizer runtime is absent")
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    r = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert b"ok" in r.stdout
