"""The inputs that tests/test_deflate_model_hist.py and tests/test_gpu_deflate_hist.py share: launches of
fc2_deflate_launch_hist named for the branch of the history rule (deflate_model_hist.py) that they reach --
(text, tile, hist, level) -- each with the `without` name of deflate_model_hist that leaves the branch out."""
from functools import lru_cache

import numpy as np

from deflate_helpers import CONTENTS, fastq_text
from deflate_model_hist import launch_streams


def _rand(rng, n, lo=0, hi=256):
    return bytes(rng.integers(lo, hi, n, dtype=np.uint8))


def src_into_tile():
    """A period of 16 bytes across the boundary of two tiles of 1024: the second tile's first match starts in
    the history and runs on into the tile."""
    rng = np.random.default_rng(41)
    period = _rand(rng, 16, 0, 16)
    return _rand(rng, 1024 - 32, 0, 16) + period * 2 + period * 3 + _rand(rng, 1024 - 48, 0, 16), 1024, 64, 1


def _marker_tiles(lead):
    """Two tiles of 32768: 24 marked bytes and zeros, the second with `lead` bytes in front of the marker --
    the marker's four-byte words hash nowhere else, so the head still holds the first one."""
    marker = bytes(range(101, 125))
    return marker + bytes(32768 - 24) + lead + marker + bytes(32768 - 24 - len(lead))


def dist_32768():
    """The second tile's first position repeats the launch's first: a distance of exactly 32768."""
    return _marker_tiles(b""), 32768, 32768, 1


def dist_32769():
    """One byte later: 32769 back, not taken."""
    return _marker_tiles(b"\x07"), 32768, 32768, 1


def links_reused():
    """dist_32768 at level 2, tile + hist = 65536: position 32768 has rewritten position 0's link slot in its
    own step, so the walk ends before it looks there."""
    return _marker_tiles(b""), 32768, 32768, 2


def short_first_histories():
    """Lines of 100 bytes in tiles of 100 with hist = 4096: h is 0, 100, 200, 300 -- below hist on every tile."""
    return CONTENTS["line100"](3 * 100 + 17), 100, 4096, 1


def straddle():
    """tile 100, hist 65: the second tile's region starts 35 bytes into the text, and its steps are laid from
    there.  "abcd" six times from the region's position 124: 128 opens a step and finds 124 in the heads; with
    the steps laid from the tile's start (65) both would share a step, and the match would begin at 129."""
    rng = np.random.default_rng(61)
    return _rand(rng, 159, 0, 4) + b"abcd" * 6 + _rand(rng, 317 - 183, 0, 4), 100, 65, 1


def _short_history(h):
    """A key of 12 bytes whose first h end the first tile of 128; the second tile starts with the rest and
    holds the whole key at the region's position 92 - h: that match's source is the history's first byte.  No history position
    has its four bytes inside a history this short: they enter with bytes of the tile."""
    rng = np.random.default_rng(43 + h)
    key = bytes(range(16, 28))
    return (_rand(rng, 128 - h, 0, 16) + key[:h] + key[h:] + _rand(rng, 80 - h, 0, 16) + key + _rand(rng, 128 - 92, 0, 16),
            128, h, 1)


def hist_1():
    return _short_history(1)


def hist_3():
    return _short_history(3)


def literal_cost():
    """12288 bytes of 'A', then 4096 random ones of CGTN: the history's bytes in the histogram would make a
    literal cheaper (28 sixteenths of a bit for 32) and refuse the tile's matches of 7, 8 and 9."""
    rng = np.random.default_rng(47)
    tile = np.frombuffer(b"CGTN", np.uint8)[rng.integers(0, 4, 4096)].tobytes()
    return b"A" * 12288 + tile, 4096, 12288, 1


def tile_of_1():
    """Tiles of one byte with three of history: stored blocks of six bytes, the last one final."""
    return b"abcabcabcabcabcabcab", 1, 3, 1


def stored_tiles():
    """Tiles of 256: text, random bytes, text, random bytes -- a stored tile in the middle and one at the end."""
    rng = np.random.default_rng(53)
    text = fastq_text(256)
    return text + _rand(rng, 256) + text + _rand(rng, 100), 256, 64, 1


def alignment_bytes():
    """Two tiles whose first is estimated below its stored form as a block alone and not with the empty stored
    block behind it (found by search: tests/test_deflate_model_hist.py asserts the estimates)."""
    rng = np.random.default_rng(ALIGN_SEED)
    return _rand(rng, ALIGN_N, 0, ALIGN_K) + b"end", ALIGN_N, 64, 1


ALIGN_SEED, ALIGN_N, ALIGN_K = 0, 1200, 207


def chain_into_history():
    """Level 2: 40 bytes in the first tile of 512; in the second their first 6, and 100 bytes on all 40: the
    head is the near occurrence, the link behind it leads into the history."""
    rng = np.random.default_rng(59)
    s = _rand(rng, 40, 16, 32)
    one = _rand(rng, 100, 0, 16) + s + _rand(rng, 512 - 140, 0, 16)
    two = _rand(rng, 80, 0, 16) + s[:6] + _rand(rng, 100, 0, 16) + s + _rand(rng, 512 - 226, 0, 16)
    return one + two, 512, 512, 2


# name: (the launch, the branch's `without` name, the tile that reaches it)
NAMED_HIST = {
    "src_into_tile": (src_into_tile, "histsrc", 1),
    "dist_32768": (dist_32768, "dist32768", 1),
    "dist_32769": (dist_32769, "maxdist", 1),
    "short_first_histories": (short_first_histories, "firsthist", 1),
    "straddle": (straddle, "straddle", 1),
    "hist_1": (hist_1, "shorthist", 1),
    "hist_3": (hist_3, "shorthist", 1),
    "literal_cost": (literal_cost, "litcost", 3),
    "tile_of_1": (tile_of_1, "nonfinal", 0),
    "stored_middle": (stored_tiles, "nonfinal", 1),
    "stored_end": (stored_tiles, "final", 3),
    "alignment_bytes": (alignment_bytes, "align", 0),
    "chain_into_history": (chain_into_history, "histsrc", 1),
    "links_reused": (links_reused, "window", 1),
}


@lru_cache(maxsize=None)
def named_hist(name):
    """(text, tile, hist, level, [(stream, crc, info)])"""
    text, tile, hist, level = NAMED_HIST[name][0]()
    return text, tile, hist, level, launch_streams(text, tile, hist, level)
