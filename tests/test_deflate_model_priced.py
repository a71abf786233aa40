"""deflate_model_priced.py, the rule of fc2_deflate_launch_priced in Python: with one pass it is deflate_model_deep
byte for byte in all three shapes on the named inputs those models are tested on; every stream at every number of
passes inflates to its input; each planted input of deflate_priced_inputs.py reaches the branch of the priced rule it
is there for, and gives other bytes when that branch is missing; and on BAM records in the generator's shape and on
FASTQ text the sizes are these, byte for byte (DESIGN.md §5 "Priced passes at level 2" quotes them against zlib
level 6's 16711 B and 13158 B):

    one tile of bam_records(0xff00)   (8, 32): 17468, 17033, 16945 B    (32, 258): 17074, 16682, 16594 B
    planted_fastq(32768, 40)          (8, 32): 13325, 13208, 13197 B    (32, 258): 12260, 12164, 12152 B

for 1, 2 and 3 passes.  The order 1 pass > 2 passes >= 3 passes is asserted beside them."""
import zlib

import pytest

import deflate_model_hist
from deflate2_inputs import NAMED2, named2, planted_fastq
from deflate_deep_inputs import bam_records, named_deep
from deflate_hist_inputs import NAMED_HIST, named_hist
from deflate_model import literal_cost
from deflate_model_deep import (LEVEL2, group_streams_deep, hist_streams_deep, launch_deep, model_deep, model_hist_deep,
                                search)
from deflate_model_groups import boundary_input
from deflate_model_priced import (group_streams_priced, hist_streams_priced, launch_priced, model_hist_priced, model_priced,
                                  pass_)
from deflate_priced_inputs import BRANCH, PLANTED, RARE, planted

SETTINGS = ((8, 32), (32, 258))
SIZES = {
    ("records", (8, 32)): (17468, 17033, 16945), ("records", (32, 258)): (17074, 16682, 16594),
    ("fastq", (8, 32)): (13325, 13208, 13197), ("fastq", (32, 258)): (12260, 12164, 12152),
}


def _inflate(streams, zdict=b""):
    z = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
    out = z.decompress(b"".join(streams))
    assert z.eof and z.unused_data == b""
    return out


def _pairs(tiles):
    return [(s, c) for s, c, _ in tiles]


# ---- one pass is deflate_model_deep ------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(NAMED2))
def test_one_pass_of_an_independent_tile_is_model_deep(name):
    data = named2(name)[0]
    for depth, nice in (LEVEL2, (32, 258)) if len(data) < 20000 else (LEVEL2,):
        want, winfo = model_deep(data, depth, nice)
        got, ginfo = model_priced(data, depth, nice, 1)
        assert got == want and ginfo["l2"] == winfo["l2"] and ginfo["crc"] == winfo["crc"]
        assert _pairs(launch_priced(data, 0, 65536, 0, depth, nice, 1)) == [(want, winfo["crc"])]


@pytest.mark.parametrize("name", sorted(NAMED_HIST))
def test_one_pass_of_a_launch_with_a_history_is_hist_streams_deep(name):
    text, tile, hist, _level, _ = named_hist(name)
    for depth, nice in (LEVEL2, (32, 258)) if len(text) < 20000 else (LEVEL2,):
        assert _pairs(hist_streams_priced(text, tile, hist, depth, nice, 1)) == _pairs(hist_streams_deep(text, tile, hist, depth, nice))


@pytest.mark.parametrize("group,tile,hist", [(4113, 1029, 4096), (4113, 1029, 0), (4113, 5000, 300), (100, 26, 65)])
def test_one_pass_of_groups_is_group_streams_deep(group, tile, hist):
    texts = [planted_fastq(2 * group + 17, 20)] + ([boundary_input(group)] if group >= 600 else [])
    for text in texts:
        for depth, nice in (LEVEL2, (32, 258)):
            want = group_streams_deep(text, group, tile, hist, depth, nice)
            got = group_streams_priced(text, group, tile, hist, depth, nice, 1)
            assert [_pairs(g) for g in got] == [_pairs(g) for g in want]
            assert _pairs(launch_priced(text, group, tile, hist, depth, nice, 1)) == _pairs(launch_deep(text, group, tile, hist, depth, nice))


@pytest.mark.parametrize("name", ("chain8", "lazy", "wrapped_links"))
def test_the_restated_pass_under_the_flat_rule_is_level_2s_pass_1(name):
    """pass_() is pass 1 written out again; with no price it must be deflate_model_hist's, history or none."""
    data = named2(name)[0]
    for h in (0, min(len(data) // 3, 5000)):
        lit16 = literal_cost(data[h:])
        for depth, nice in SETTINGS:
            with search(depth, nice):
                want = deflate_model_hist.find_matches_hist(data, h, lit16, 2)[:4]
            assert pass_(data, h, lit16, depth, nice)[:4] == want


def test_the_arguments_are_checked_and_nothing_outlives_a_call():
    first = deflate_model_hist.find_matches_hist
    for bad in ((8, 32, 0), (8, 32, 4), (0, 32, 2), (8, 259, 2)):
        with pytest.raises(AssertionError):
            model_priced(b"abcabcabcabc", *bad)
    assert model_priced(b"abcabcabcabc" * 9, 8, 32, 3)[1]["priced"]["passes"] == 3
    assert deflate_model_hist.find_matches_hist is first
    assert (deflate_model_hist.DEPTH, deflate_model_hist.NICE) == LEVEL2


# ---- every stream inflates to its input ---------------------------------------------------------------------

@pytest.mark.parametrize("passes", (2, 3))
def test_every_stream_inflates_to_its_input(passes):
    settings = (SETTINGS[passes - 2],)              # 2 passes at (8, 32), 3 at (32, 258): the model takes seconds on the long ones
    for name in sorted(NAMED2):
        data = named2(name)[0]
        for depth, nice in settings:
            s, info = model_priced(data, depth, nice, passes)
            assert _inflate([s]) == data and info["crc"] == zlib.crc32(data), name
            assert info["priced"]["passes"] == passes
    for name in sorted(NAMED_HIST):
        text, tile, hist, _level, _ = named_hist(name)
        for depth, nice in settings:
            out = hist_streams_priced(text, tile, hist, depth, nice, passes)
            if hist:
                assert _inflate([s for s, _, _ in out]) == text, name
            else:
                assert b"".join(_inflate([s]) for s, _, _ in out) == text, name
            assert [c for _, c, _ in out] == [zlib.crc32(text[k:k + tile]) for k in range(0, len(text), tile)]
    for group, tile, hist in ((4113, 1029, 4096), (4113, 64, 65), (100, 26, 0)):
        text = boundary_input(group) if group >= 600 else planted_fastq(2 * group + 17, 20)
        for g, tiles in enumerate(group_streams_priced(text, group, tile, hist, 8, 32, passes)):
            assert _inflate([s for s, _, _ in tiles]) == text[g * group:(g + 1) * group], (group, tile, hist, g)
    for name in ("bucket33_9", "nice40_120"):
        data = named_deep(name)[0]
        assert _inflate([model_priced(data, 32, 258, passes)[0]]) == data, name
    for name in sorted(PLANTED):
        history, data = planted(name)
        assert _inflate([model_hist_priced(history, data, True, 8, 32, passes)[0]], history) == data, name


# ---- the planted inputs reach their branches ----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PLANTED))
def test_a_planted_input_reaches_its_branch_and_the_switch_changes_its_bytes(name):
    history, data = planted(name)
    counter, switch = BRANCH[name]
    one = model_hist_priced(history, data, True, 8, 32, 1)[0]
    two, info = model_hist_priced(history, data, True, 8, 32, 2)
    assert info["priced"][counter] > 0 and info["priced"]["passes"] == 2
    assert info["priced"]["visits"] >= info["priced"]["fit"] > 0
    assert two != one
    other = model_hist_priced(history, data, True, 8, 32, 2, without=(switch,))[0]
    assert other != two
    assert _inflate([other], history) == data           # (another parse of the same bytes, not a broken stream)


def test_gained_is_the_phrase_of_rare_bytes():
    _, data = planted("gained")
    one, two = (model_priced(data, 8, 32, p)[1] for p in (1, 2))
    assert 8 * literal_cost(data) < 16 * 11              # the flat rule refuses eight bytes at any distance
    # pass 1 writes every phrase as literals; the priced pass writes the first so and the others as matches
    assert data.count(RARE) == 6 and one["tokens"].count(RARE[0]) == 6 and two["tokens"].count(RARE[0]) == 1
    assert two["priced"]["gained"] >= 5
    assert len(model_priced(data, 8, 32, 2)[0]) < len(model_priced(data, 8, 32, 1)[0])


def test_dropped_refuses_short_matches_of_cheap_literals():
    _, data = planted("dropped")
    info = model_priced(data, 8, 32, 2)[1]
    assert info["priced"]["dropped"] > 50 and info["priced"]["gained"] == 0


def test_uncoded_dist_prices_a_distance_code_of_dummies():
    _, data = planted("uncoded_dist")
    one = model_priced(data, 8, 32, 1)[1]
    assert not [t for t in one["tokens"] if isinstance(t, tuple)]
    assert one["dfreq"][:2] == [1, 1] and not any(one["dfreq"][2:])      # the two dummy symbols
    two = model_priced(data, 8, 32, 2)[1]
    assert [t for t in two["tokens"] if isinstance(t, tuple)] == [("m", 8, 500)]
    assert two["priced"]["uncoded"] > 0 and two["priced"]["gained"] == 1


def test_uncoded_literal_is_a_byte_the_tile_has_only_under_a_match():
    history, data = planted("uncoded_literal")
    assert data.count(b"\xf0") == 1 and history.count(b"\xf0") == 1
    for passes in (1, 2):
        info = model_hist_priced(history, data, True, 8, 32, passes)[1]
        assert 0xf0 not in [t for t in info["tokens"] if not isinstance(t, tuple)]
        assert ("m", 15, 64) in info["tokens"]           # the phrase, from the history
    assert info["priced"]["uncoded"] > 0


# ---- sizes --------------------------------------------------------------------------------------------------

def _zlib6(data):
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    return len(z.compress(data) + z.flush())


@pytest.mark.parametrize("which,setting", sorted(SIZES))
def test_the_sizes_are_the_tables_and_fall_with_the_passes(which, setting):
    data = bam_records(0xff00) if which == "records" else planted_fastq(32768, 40)
    got, infos = [], []
    for passes in (1, 2, 3):
        s, info = model_priced(data, *setting, passes)
        assert _inflate([s]) == data
        got.append(len(s))
        infos.append(info)
    ref = _zlib6(data)
    print("%s at %s: %s B for 1, 2, 3 passes, zlib level 6 %d B: %s; last pass visits %d, fit %d"
          % (which, setting, got, ref, ", ".join("%.4f" % (g / ref) for g in got), infos[2]["priced"]["visits"],
             infos[2]["priced"]["fit"]))
    assert got[0] > got[1] >= got[2]
    assert tuple(got) == SIZES[(which, setting)]
