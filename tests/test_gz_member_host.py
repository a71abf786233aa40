"""csrc/fc2_gzmember_impl.h -- one gzip member from the tile streams of a launch with a history -- through a
stand-alone program (tests/c/gz_member_main.cpp) built for the host with ASan and UBSan and run directly.  The
tile streams and CRCs come from zlib (raw deflate per tile, the 32 KiB before the tile as its dictionary, a
full flush between tiles: the form fc2_deflate_launch_hist writes); the member the program assembles must
inflate with zlib.decompressobj(31) to the text, ending at its last byte.  1, 2 and 129 tiles, a last tile of
one byte, each invalid out_len, and a piece over 4 GiB through the length arithmetic alone."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from deflate_helpers import fastq_text


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    path = str(tmp_path_factory.mktemp("gzmember") / "gz_member_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", path, os.path.join(ROOT, "tests", "c", "gz_member_main.cpp"), "-lz"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0 and (b"asan" in r.stdout.lower() or b"ubsan" in r.stdout.lower() or b"sanitize" in r.stdout.lower()):
        pytest.skip("the sanitizer runtime is absent")
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    return path


def tile_streams(text, tile, level=6):
    """[(stream, crc)] per tile: every stream but the last ends on a byte boundary with BFINAL = 0."""
    out = []
    for k in range(0, len(text), tile):
        kw = dict(zdict=text[max(0, k - 32768):k]) if k else {}
        z = zlib.compressobj(level, zlib.DEFLATED, -15, **kw)
        data = text[k:k + tile]
        s = z.compress(data) + (z.flush(zlib.Z_FINISH) if k + tile >= len(text) else z.flush(zlib.Z_FULL_FLUSH))
        out.append((s, zlib.crc32(data)))
    return out


def assemble(exe, tmp_path, streams, n_bytes, tile, stride=None, tag="p"):
    stride = stride or ((tile + 16 + 15) & ~15) + 16
    assert all(len(s) <= stride for s, _ in streams)
    blob = struct.pack("<IIIQ", len(streams), tile, stride, n_bytes)
    blob += struct.pack("<%dI" % len(streams), *[len(s) for s, _ in streams])
    blob += struct.pack("<%dI" % len(streams), *[c for _, c in streams])
    blob += b"".join(s + b"\xEE" * (stride - len(s)) for s, _ in streams)
    src, dst = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".gz"))
    open(src, "wb").write(blob)
    r = subprocess.run([exe, "assemble", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    return r.stdout.decode().split(), open(dst, "rb").read()


@pytest.mark.parametrize("n_tiles,last", [(1, 700), (2, 1), (2, 1000), (129, 1), (129, 517)])
def test_member_inflates_to_the_text(exe, tmp_path, n_tiles, last):
    tile = 1000
    text = fastq_text((n_tiles - 1) * tile + last)
    streams = tile_streams(text, tile)
    assert len(streams) == n_tiles and all(len(s) <= tile + 16 for s, _ in streams)
    said, member = assemble(exe, tmp_path, streams, len(text), tile)
    assert said == ["ok", str(18 + sum(len(s) for s, _ in streams))] and len(member) == int(said[1])
    assert member[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])
    assert member[10:-8] == b"".join(s for s, _ in streams)
    assert member[-8:] == struct.pack("<II", zlib.crc32(text), len(text))
    z = zlib.decompressobj(31)
    got = z.decompress(member[:-1])
    assert not z.eof                                # the end is the member's last byte, no sooner
    got += z.decompress(member[-1:])
    assert got == text and z.eof and z.unused_data == b"" and z.unconsumed_tail == b""


def test_an_invalid_tile_leaves_the_piece_unwritten(exe, tmp_path):
    tile = 1000
    text = fastq_text(3 * tile + 5)
    streams = tile_streams(text, tile)
    for k, bad in enumerate((0, 0xFFFFFFFF, tile + 17)):
        for at in (0, 2, 3):
            lens = [(s, c) for s, c in streams]
            said, member = assemble(exe, tmp_path, lens, len(text), tile, tag="bad%d_%d" % (k, at))
            assert said[0] == "ok"
            # the same slots with one length replaced: written through the header by hand
            src = str(tmp_path / ("bad%d_%d.in" % (k, at)))
            blob = bytearray(open(src, "rb").read())
            blob[20 + 4 * at:24 + 4 * at] = struct.pack("<I", bad)
            open(src, "wb").write(bytes(blob))
            dst = str(tmp_path / "unwritten.gz")
            r = subprocess.run([exe, "assemble", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
            assert r.returncode == 0 and r.stdout.decode().split() == ["unwritten"] and os.path.getsize(dst) == 0
    # n_bytes that does not end in the last tile: refused as a piece
    for n_bytes in (3 * tile, 4 * tile + 1):
        said, member = assemble(exe, tmp_path, streams, n_bytes, tile, tag="len%d" % n_bytes)
        assert said == ["unwritten"] and member == b""


def test_a_piece_over_4_gib_through_the_arithmetic(exe):
    tile, last = 65536, 4464
    n_tiles = 65536 + 2
    n_bytes = (n_tiles - 1) * tile + last
    assert n_bytes > 1 << 32
    zeros = bytes(1 << 20)
    crc = 0
    for _ in range(n_bytes >> 20):
        crc = zlib.crc32(zeros, crc)
    crc = zlib.crc32(zeros[:n_bytes & ((1 << 20) - 1)], crc)
    r = subprocess.run([exe, "arith", str(n_tiles), str(n_bytes), str(tile), str(zlib.crc32(zeros[:tile])),
                        str(zlib.crc32(zeros[:last]))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    ok, isize, last_bytes, combined = (int(x) for x in r.stdout.split())
    assert ok == 1 and isize == n_bytes - (1 << 32) == tile + last and last_bytes == last and combined == crc
    for bad_n in (n_bytes + tile, (n_tiles - 1) * tile):
        r = subprocess.run([exe, "arith", str(n_tiles), str(bad_n), str(tile), "0", "0"], stdout=subprocess.PIPE)
        assert r.stdout.split()[0] == b"0"
