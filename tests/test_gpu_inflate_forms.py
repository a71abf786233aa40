"""The GPU inflater (fc2_bgzf_inflate_launch, csrc/fc2_inflate.hip) on what zlib's compressor never
feeds it: the forged streams of test_deflate_forge.CASES (every form RFC 1951 allows, and the ones
it forbids), output sizes on either side of the kernel's granules, matches placed on the LDS ring's
wrap, the flush granule and the hand-over to the far-match path, and libdeflate's streams.  Every
launch here also checks containment: a block, inflated or refused, writes only inside its own slot
(gpu_helpers.inflate_run)."""
import zlib

import numpy as np
import pytest

from gpu_helpers import SLOT, inflate_run
from test_deflate_forge import CASES, LIBDEFLATE, geometry, libdeflate_deflate, zlib_inflate

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _crc(case):
    return zlib.crc32(case.want) if case.want is not None else 0x12345678


@pytest.mark.parametrize("crcs", ["none", "right", "flipped"])
def test_forms(crcs):
    """All of CASES in one launch.  valid: status 0 and the intended bytes (0 with the right CRC-32, 16
    with one bit of it flipped); invalid: refused, with or without a CRC; split: any status, and where
    it is 0 the bytes of the reference that accepted -- refused where the case says the device must."""
    given = {"none": None, "right": [_crc(c) for c in CASES],
             "flipped": [_crc(c) ^ (1 << (k % 32)) for k, c in enumerate(CASES)]}[crcs]
    got, st = inflate_run([c.payload for c in CASES], [c.size for c in CASES], given, contained=True)
    wrong = []
    for c, g, s in zip(CASES, got, (int(x) for x in st)):
        if c.cls == "valid":
            ok = s == (16 if crcs == "flipped" else 0) and (s != 0 or g == c.want)
        elif c.cls == "invalid" or c.device == "refuse":
            ok = 1 <= s <= 15
        else:
            ok = 0 <= s <= 16 and (s != 0 or g == c.want) and not (s == 0 and crcs == "flipped")
        if not ok:
            wrong.append((c.name, c.cls, s))
    assert not wrong, wrong


def test_damaged_forms_stay_in_their_slots():
    """Every case's payload cut short, with bits flipped, and with a claimed size too small and too
    large: each block ends in a status and writes only inside its slot."""
    rng = np.random.default_rng(99)
    payloads, sizes = [], []
    for c in CASES:
        b = bytearray(c.payload)
        for _ in range(4):
            if b:
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        payloads += [bytes(b), c.payload[:len(c.payload) // 2], c.payload, c.payload]
        sizes += [c.size, c.size, max(0, c.size - int(rng.integers(1, 40))), min(SLOT, c.size + int(rng.integers(1, 40)))]
    got, st = inflate_run(payloads, sizes, contained=True)
    assert all(0 <= s <= 16 for s in st)
    for k, c in enumerate(CASES):                # a wrong size is never status 0
        assert st[4 * k + 2] != 0 or c.size == 0, c.name
        assert st[4 * k + 3] != 0 or c.size == SLOT, c.name


SIZES = sorted({0, 1, 15, 16, 17, 65279, 65280} |
               {k + d for k in (1024, 4096, 8192, 16384, 20480, 32768, 65536) for d in (-1, 0, 1)} - {65537})


def test_sizes():
    """Outputs of every size on either side of the kernel's granules (a lane's 16 bytes, a row of
    1024, the 4 KiB flush, the 16 KiB ring, 64 KiB), as stored, fixed-code and default zlib streams."""
    from test_gpu_inflate import _deflate, _samples
    s = _samples()
    data, payloads = [], []
    for content in ((s[5] * 2)[:SLOT], s[9]):    # ACGT; text
        assert len(content) == SLOT
        for n in SIZES:
            for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_DEFAULT_STRATEGY)):
                data.append(content[:n])
                payloads.append(_deflate(content[:n], level, strategy))
    got, st = inflate_run(payloads, [len(x) for x in data], [zlib.crc32(x) for x in data], contained=True)
    assert [(len(x), int(v)) for x, v in zip(data, st) if v != 0] == []
    assert got == data


@pytest.mark.parametrize("kind", ["fixed", "dyn15"])
def test_match_geometry(kind):
    """Matches starting on and around the ring's wrap and the flush granule -- overlapping ones of
    every period around the wave's 64 lanes and the 258-byte maximum, dist + len on either side of
    the ring's 16 KiB, the window's full 32 KiB, dist == p -- under the fixed code and under 15-bit
    dynamic codes, against zlib's inflate of the same payloads."""
    payloads, _ = geometry(kind)
    want = [zlib_inflate(p) for p in payloads]
    assert all(w is not None and len(w) <= SLOT for w in want)
    got, st = inflate_run(payloads, [len(w) for w in want], [zlib.crc32(w) for w in want], contained=True)
    assert [int(x) for x in st] == [0] * len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            at = next(i for i in range(len(w)) if g[i] != w[i])
            pytest.fail("output %d differs from byte %d on" % (k, at))


def test_libdeflate_streams():
    """What htslib built with libdeflate writes: the samples compressed by libdeflate at levels 1, 6,
    9 and 12, and a 65280-byte sample of text, random bytes and ACGT on which it changes block type
    mid-stream -- inflated on the device, its CRC-32 check included."""
    if LIBDEFLATE is None:
        pytest.skip("libdeflate.so.0 does not load")
    from test_gpu_inflate import _samples
    s = _samples()
    mixed = (s[9][:22000] + s[4][:21000] + s[5])[:65280]
    data = [x for x in s + [mixed] for _ in (1, 6, 9, 12)]
    payloads = [libdeflate_deflate(x, lv) for x in s + [mixed] for lv in (1, 6, 9, 12)]
    assert all(zlib_inflate(p) == x for p, x in zip(payloads, data))
    crcs = [zlib.crc32(x) for x in data]
    got, st = inflate_run(payloads, [len(x) for x in data], crcs, contained=True)
    assert [int(x) for x in st] == [0] * len(data)
    assert got == data
    _, st = inflate_run(payloads, [len(x) for x in data], [c ^ (1 << (k % 32)) for k, c in enumerate(crcs)], contained=True)
    assert [int(x) for x in st] == [16] * len(data)
