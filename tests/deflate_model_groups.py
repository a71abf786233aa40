"""The GPU DEFLATE compressor over groups (deflate_kernel<level, true, true> through fc2_deflate_launch_groups,
find_circ2_amd/csrc/fc2_deflate.hip), bit-exact in plain Python on deflate_model_hist.model_hist.

The rule (the kernel's header comment states the same).  The launch's bytes are cut into groups of `group`
bytes, the last group holding the rest, and every group into tiles of `tile` bytes, a group's last tile
holding its rest; tiles are numbered densely, group after group.  Tile k of a group has the
h = min(hist, k * tile) bytes before it as its history: never a byte before its group's first, and none for a
group's first tile.  A group is one raw DEFLATE stream whatever hist is, hist = 0 too: its last tile is written
with BFINAL = 1, every other tile in model_hist's non-final form (BFINAL = 0 and the empty stored block, or
non-final stored blocks).  So with one tile a group the launch is deflate_model.model / deflate_model2.model2
tile by tile, and with hist > 0 a group is deflate_model_hist.launch_streams over that group's bytes alone.

group_streams(text, group, tile, hist, level) -> [[(stream, crc, info)] per group]."""
from deflate_model_hist import model_hist


def group_tiles(n_bytes, group, tile):
    """fc2_deflate_group_tiles: the tiles of a launch."""
    tpg = (group - 1) // tile + 1
    return n_bytes // group * tpg + (n_bytes % group + tile - 1) // tile


def group_streams(text, group, tile, hist, level, without=()):
    text = bytes(text)
    assert group >= 1 and 1 <= tile <= 65536 and 0 <= hist <= 32768 and tile + hist <= 65536 and level in (1, 2)
    out = []
    for g0 in range(0, len(text), group):
        part = text[g0:g0 + group]
        tiles = []
        for k in range(0, len(part), tile):
            h = min(hist, k)                        # clamped at the group's start
            s, info = model_hist(part[k - h:k], part[k:k + tile], level, k + tile >= len(part), 0, without)
            tiles.append((s, info["crc"], info))
        out.append(tiles)
    assert sum(len(t) for t in out) == group_tiles(len(text), group, tile)
    return out


def boundary_input(group, seed=11):
    """2 * group + 17 bytes of text whose second group begins with a copy of the first group's last 300 bytes
    (group >= 600): a history that reached across the group boundary would find that match at distance 300."""
    import numpy as np

    from deflate2_inputs import planted_fastq
    assert group >= 600
    rng = np.random.default_rng(seed)
    text = bytearray(planted_fastq(2 * group + 17, 20))
    tail = bytes(rng.integers(33, 127, 300, dtype=np.uint8))      # (found nowhere else in the text)
    text[group - 300:group] = tail
    text[group:group + 300] = tail
    return bytes(text)
