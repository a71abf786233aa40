"""deflate_model_deep.py, the rule of fc2_deflate_launch_deep in Python: at depth 8 and nice 32 it is the three
existing models byte for byte on every named input they are tested on; every stream at every setting inflates to
its input; each planted input of deflate_deep_inputs.py reaches the branch it is there for exactly where `depth` or
`nice` opens it; and on FASTQ text and on BAM records in the shape of the generator's spliced reads the search at
depth 32, nice 258 gives a smaller stream than level 2's own 8 and 32.

The ratios to zlib level 6 that the size tests print (DESIGN.md §5 "Search effort at level 2" quotes them):
planted_fastq(32768, 40): 13325 B at (8, 32) and 12260 B at (32, 258) against zlib's 13158 B, 1.013 and 0.932;
one tile of 0xff00 bytes of bam_records: 17468 B and 17074 B against 16711 B, 1.045 and 1.022."""
import zlib

import pytest

import deflate_model2
import deflate_model_hist
from deflate2_inputs import NAMED2, named2, planted_fastq
from deflate_deep_inputs import KEY, bam_records, key_positions, named_deep
from deflate_hist_inputs import NAMED_HIST, named_hist
from deflate_model_deep import (LEVEL2, group_streams_deep, hist_streams_deep, launch_deep, model_deep, model_hist_deep,
                                search)
from deflate_model_groups import boundary_input, group_streams

SETTINGS = ((8, 32), (9, 32), (32, 258), (128, 258), (1, 32), (1, 4), (128, 4))


def _inflate(streams):
    z = zlib.decompressobj(-15)
    out = z.decompress(b"".join(streams))
    assert z.eof and z.unused_data == b""
    return out


def _matches(info):
    return [t for t in info["tokens"] if isinstance(t, tuple)]


# ---- depth 8, nice 32 is level 2 ------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(NAMED2))
def test_at_8_32_an_independent_tile_is_model2(name):
    data, stream, info = named2(name)
    got, ginfo = model_deep(data, *LEVEL2)
    assert got == stream and ginfo["l2"] == info["l2"] and ginfo["crc"] == info["crc"]


@pytest.mark.parametrize("name", sorted(NAMED_HIST))
def test_at_8_32_a_launch_with_a_history_is_launch_streams_at_level_2(name):
    text, tile, hist, _level, _ = named_hist(name)
    want = deflate_model_hist.launch_streams(text, tile, hist, 2)
    got = hist_streams_deep(text, tile, hist, *LEVEL2)
    assert [(s, c) for s, c, _ in got] == [(s, c) for s, c, _ in want]


@pytest.mark.parametrize("group,tile,hist", [(4113, 1029, 4096), (4113, 1029, 0), (4113, 5000, 300), (100, 26, 65)])
def test_at_8_32_groups_are_group_streams_at_level_2(group, tile, hist):
    texts = [planted_fastq(2 * group + 17, 20)] + ([boundary_input(group)] if group >= 600 else [])
    for text in texts:
        want = group_streams(text, group, tile, hist, 2)
        got = group_streams_deep(text, group, tile, hist, *LEVEL2)
        assert [[(s, c) for s, c, _ in g] for g in got] == [[(s, c) for s, c, _ in g] for g in want]
        assert [(s, c) for s, c, _ in launch_deep(text, group, tile, hist, *LEVEL2)] == [(s, c) for g in want for s, c, _ in g]


def test_the_setting_does_not_outlive_a_call():
    with search(32, 258):
        assert (deflate_model2.DEPTH, deflate_model2.NICE) == (deflate_model_hist.DEPTH, deflate_model_hist.NICE) == (32, 258)
    assert (deflate_model2.DEPTH, deflate_model2.NICE) == (deflate_model_hist.DEPTH, deflate_model_hist.NICE) == LEVEL2
    for bad in ((0, 32), (129, 32), (8, 3), (8, 259)):
        with pytest.raises(AssertionError):
            model_deep(b"abc", *bad)
    assert (deflate_model2.DEPTH, deflate_model2.NICE) == LEVEL2


# ---- every stream inflates to its input -----------------------------------------------------------------

@pytest.mark.parametrize("depth,nice", SETTINGS)
def test_every_stream_inflates_to_its_input(depth, nice):
    for name in sorted(NAMED2):
        if name in ("window_edge", "wrapped_links") and (depth, nice) not in ((32, 258), (1, 32)):
            continue                                # (the two long ones at two settings: the model takes seconds there)
        data = named2(name)[0]
        s, info = model_deep(data, depth, nice)
        assert _inflate([s]) == data and info["crc"] == zlib.crc32(data), name
    for name in sorted(NAMED_HIST):
        text, tile, hist, _level, _ = named_hist(name)
        if len(text) > 20000 and (depth, nice) != (32, 258):
            continue
        out = hist_streams_deep(text, tile, hist, depth, nice)
        assert _inflate([s for s, _, _ in out]) == text, name
        assert [c for _, c, _ in out] == [zlib.crc32(text[k:k + tile]) for k in range(0, len(text), tile)]
    for group, tile, hist in ((4113, 1029, 4096), (4113, 64, 65), (100, 26, 0)):
        text = boundary_input(group) if group >= 600 else planted_fastq(2 * group + 17, 20)
        for g, tiles in enumerate(group_streams_deep(text, group, tile, hist, depth, nice)):
            assert _inflate([s for s, _, _ in tiles]) == text[g * group:(g + 1) * group], (group, tile, hist, g)
    for name in ("bucket33_9", "bucket33_33", "nice40_120"):
        data = named_deep(name)[0]
        assert _inflate([model_deep(data, depth, nice)[0]]) == data, name


# ---- the planted inputs reach their branches -------------------------------------------------------------

@pytest.mark.parametrize("k", (9, 33))
def test_the_kth_candidate_is_found_exactly_when_depth_reaches_it(k):
    data, p, dist = named_deep("bucket33_%d" % k)
    at, pure = key_positions(data)
    assert pure and at == [64 * i for i in range(34)] and p == at[-1] and data[p:p + 4] == KEY
    short, sinfo = model_deep(data, k - 1, 32)
    full, finfo = model_deep(data, k, 32)
    assert ("m", 28, dist) in finfo["tokens"] and finfo["l2"]["deep"] == 1      # kept from the depth-th candidate
    assert ("m", 28, dist) not in sinfo["tokens"] and sinfo["l2"]["deep"] == 0
    # one candidate short, position p keeps a match of 4 (dropped for the longer one that p + 1 finds: the lazy step)
    assert sinfo["l2"]["lazy"] == 1 and ("m", 27, dist) in sinfo["tokens"]
    assert short != full and len(full) < len(short)
    # more than enough changes nothing; and without the walk ("depth": one candidate) the setting is depth 1
    assert model_deep(data, 128, 32)[0] == full
    assert model_deep(data, k, 32, without=("depth",))[0] == model_deep(data, 1, 32)[0] != full


def test_depth_1_is_one_candidate():
    data = planted_fastq(4096 + 65, 20)
    one, info = model_deep(data, 1, 32)
    assert one == deflate_model2.model2(data, 0, ("depth",))[0]
    assert info["l2"]["farther"] == 0 and info["l2"]["lazy"] > 0     # nothing behind the head; the lazy step stays
    assert one != model_deep(data, 2, 32)[0]


def test_nice_decides_between_the_near_40_and_the_far_120():
    data, p, (near, far) = named_deep("nice40_120")
    at, pure = key_positions(data)
    assert pure and at == [0, near, p]
    at32, i32 = model_deep(data, 8, 32)
    at258, i258 = model_deep(data, 8, 258)
    assert _matches(i32)[-2:] == [("m", 40, near), ("m", 80, far)] and i32["l2"]["nice"] > 0
    assert _matches(i258)[-1] == ("m", 120, far) and i258["l2"]["nice"] == 0
    assert model_deep(data, 8, 40)[1]["tokens"] != i258["tokens"]         # a kept 40 ends the walk at nice 40 ...
    assert model_deep(data, 8, 41)[0] == at258                           # ... and not at 41
    assert model_deep(data, 8, 32, without=("nice",))[0] == at258 != at32
    assert model_deep(data, 1, 258)[0] != at258                          # (the 120 are the second candidate's)


def test_a_deep_walk_ends_at_the_stale_slot():
    """The chain of 64 runs over more than 32768 positions of a 65536-byte region.  Position p's 32nd candidate is
    32768 back, where p itself has rewritten the link slot: a walk of 32 ends there, a walk of 31 never gets there;
    with the stale slot followed ("window") the candidate is compared and its 104 bytes are taken at 32768."""
    text, tile, hist, p = named_deep("stale_chain")
    at, pure = key_positions(text)
    assert pure and at == [500 + 1024 * i for i in range(64)] and at[-1] == p and at[31] == p - 32768
    history, data = text[:tile], text[tile:]
    assert len(history) == hist and len(text) == 65536
    s31, i31 = model_hist_deep(history, data, True, 31, 258)
    s32, i32 = model_hist_deep(history, data, True, 32, 258)
    assert i32["l2"]["window"] > i31["l2"]["window"] > 0
    assert not any(t[2] == 32768 for t in _matches(i31) + _matches(i32))
    s32w, i32w = model_hist_deep(history, data, True, 32, 258, without=("window",))
    assert i32w["l2"]["window"] == 0 and ("m", 104, 32768) in [t[:1] + (min(t[1], 104),) + t[2:] for t in _matches(i32w)]
    s31w, i31w = model_hist_deep(history, data, True, 31, 258, without=("window",))
    assert not any(t[1] >= 104 and t[2] == 32768 for t in _matches(i31w))     # (p + 1 finds 103 of them at once)
    assert s32w != s32
    for s in (s31, s32, s32w, s31w):
        z = zlib.decompressobj(-15, zdict=history)
        assert z.decompress(s) == data and z.eof


# ---- sizes ------------------------------------------------------------------------------------------------

def _zlib6(data):
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    return len(z.compress(data) + z.flush())


def test_the_planted_fastq_is_smaller_at_32_258():
    data = planted_fastq(32768, 40)
    base, deep, ref = len(model_deep(data, 8, 32)[0]), len(model_deep(data, 32, 258)[0]), _zlib6(data)
    print("planted_fastq(32768, 40): (8, 32) %d B, (32, 258) %d B, zlib level 6 %d B: %.4f and %.4f"
          % (base, deep, ref, base / ref, deep / ref))
    assert deep < base


def test_bam_records_in_one_tile_are_smaller_at_32_258():
    data = bam_records(0xff00)
    assert len(data) == 0xff00 and data[36:37] == b"s"      # (the first record's name)
    base, deep, ref = len(model_deep(data, 8, 32)[0]), len(model_deep(data, 32, 258)[0]), _zlib6(data)
    print("bam_records(0xff00): (8, 32) %d B, (32, 258) %d B, zlib level 6 %d B: %.4f and %.4f"
          % (base, deep, ref, base / ref, deep / ref))
    assert deep < base
