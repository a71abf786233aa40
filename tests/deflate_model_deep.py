"""Level 2 of the GPU DEFLATE compressor with its search effort as arguments (deflate_kernel<2, .., .., true>
through fc2_deflate_launch_deep, find_circ2_amd/csrc/fc2_deflate.hip): bit-exact, plain Python, in all three
launch shapes.  Only two numbers of level 2's rule become arguments -- `depth`, the candidates a position walks
at most (1..128; level 2 itself: 8), and `nice`, the kept length that ends the walk (4..258; level 2 itself: 32)
-- so the three existing models are wrapped, not restated: deflate_model2.find_matches2 and
deflate_model_hist.find_matches_hist read their modules' DEPTH and NICE when they run, and search() sets those for
the length of a call and puts level 2's own back.  Everything else -- links written with the head read before the
step's positions enter, the walk's ends (no candidate, over 32768 back, c + 32768 < base + 64), the first found
among equal lengths, the cost rule, the lazy step, everything after pass 1 -- is those modules' code.

model_deep(data, depth, nice)                          one independent tile (deflate_model2.model2)
hist_streams_deep(text, tile, hist, depth, nice)       a launch with a history (deflate_model_hist.launch_streams)
group_streams_deep(text, group, tile, hist, depth, nice)   groups (deflate_model_groups.group_streams)
launch_deep(text, group, tile, hist, depth, nice)      fc2_deflate_launch_deep's slots in order: [(stream, crc, info)]

`without` takes the wrapped models' names: "depth" (one candidate), "nice" (no end at `nice`), "window" (the stale
slot is followed), "lazy", ...  info["l2"] counts what the search did; "deep" counts the matches kept from the
depth-th candidate, the last one the walk may look at."""
from contextlib import contextmanager

import deflate_model2
import deflate_model_hist
from deflate_model_groups import group_streams

DEPTH_RANGE, NICE_RANGE = (1, 128), (4, 258)
LEVEL2 = (deflate_model2.DEPTH, deflate_model2.NICE)      # (8, 32)


@contextmanager
def search(depth, nice):
    """Level 2's two limits set to (depth, nice) in the modules whose pass 1 reads them."""
    assert DEPTH_RANGE[0] <= depth <= DEPTH_RANGE[1] and NICE_RANGE[0] <= nice <= NICE_RANGE[1], (depth, nice)
    mods = (deflate_model2, deflate_model_hist)
    saved = [(m.DEPTH, m.NICE) for m in mods]
    assert all(s == LEVEL2 for s in saved), "a search setting is already in place"
    try:
        for m in mods:
            m.DEPTH, m.NICE = depth, nice
        yield
    finally:
        for m, (d, n) in zip(mods, saved):
            m.DEPTH, m.NICE = d, n


def model_deep(data, depth, nice, a=0, without=()):
    """deflate_model2.model2 searching with (depth, nice): (stream, info)."""
    with search(depth, nice):
        return deflate_model2.model2(data, a, without)


def model_hist_deep(history, data, last, depth, nice, a=0, without=()):
    """deflate_model_hist.model_hist at level 2 searching with (depth, nice): (stream, info)."""
    with search(depth, nice):
        return deflate_model_hist.model_hist(history, data, 2, last, a, without)


def hist_streams_deep(text, tile, hist, depth, nice, without=()):
    """deflate_model_hist.launch_streams at level 2 searching with (depth, nice); hist = 0: independent tiles."""
    with search(depth, nice):
        return deflate_model_hist.launch_streams(text, tile, hist, 2, without)


def group_streams_deep(text, group, tile, hist, depth, nice, without=()):
    """deflate_model_groups.group_streams at level 2 searching with (depth, nice): [[(stream, crc, info)] per group]."""
    with search(depth, nice):
        return group_streams(text, group, tile, hist, 2, without)


def launch_deep(text, group, tile, hist, depth, nice, without=()):
    """The slots of fc2_deflate_launch_deep in the launch's order: group = 0 is the history's shape (hist = 0:
    independent tiles), group >= 1 the groups'."""
    if group:
        return [t for tiles in group_streams_deep(text, group, tile, hist, depth, nice, without) for t in tiles]
    return hist_streams_deep(text, tile, hist, depth, nice, without)
