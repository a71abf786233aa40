"""The parse threads stepping over the fragments whose rows say the device closed them
(fc2_ingest_set_gpu_group; csrc/fc2_ingest.cpp sam_parse_loop / group_batch), without a GPU: with the test
setting 2 the rows of the batches the CPU inflates are made on the host by fc2_bam_frag_host, so the
parse-thread logic is the one a device's rows drive.  The native read loop and the command line over a
BAM shaped like the steady-state generator's -- 60 % unspliced fragments in runs, unmapped records and
mates, secondaries -- in 3 kB BGZF blocks, with batches and parse blocks small enough that fragments
straddle every boundary: the same pairs, read parts, text, counters and errors as with the setting off,
and the same files byte for byte."""
import os
import re

import pytest

import group_inputs as G
from find_circ2_amd import cli
from oracle_engine import oracle_evaluator_factory
from test_ingest import counters

# (FC2_BGZF_BATCH, FC2_PARSE_BLOCK): one block a batch and one record a parse block (nothing can be
# stepped over: a placeholder needs a mapped record before it and the next fragment's head behind it in
# its parse block), then sizes at which fragments straddle BGZF blocks, batches and parse blocks
SIZES = [("1", "1"), ("1", "700"), ("3", "3000"), ("64", "20000")]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_host")
    out = {}
    for kind, paired in (("single", False), ("paired", True)):
        sam = str(d / (kind + ".sam"))
        fa = G.group_sam(sam, 1500, 11 + paired, paired)
        out[kind] = (fa, G.bam_of(sam, str(d / (kind + ".bam"))), G.bam_of(sam, str(d / (kind + "_bad.bam")), damage=0.5))
    return out


@pytest.fixture(scope="module")
def off(inputs):
    """The runs with the setting off, one per (input, options), shared by the tests."""
    cache = {}

    def run(path, **opts):
        key = (path, tuple(sorted(opts.items())))
        if key not in cache:
            cache[key] = G.caller_run(path, **opts)
        return cache[key]
    return run


@pytest.mark.parametrize("batch,block", SIZES)
@pytest.mark.parametrize("kind", ["single", "paired"])
def test_read_loop_gives_the_same_fragments(inputs, off, monkeypatch, kind, batch, block):
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    monkeypatch.setenv("FC2_PARSE_BLOCK", block)
    _, bam, _ = inputs[kind]
    ref, _, ref_grp = off(bam)
    got, inf, grp = G.caller_run(bam, group=2)
    assert got == ref
    assert len(ref[0]) > 500 and inf == (0, 0)
    n_reads = ref[3][0]
    assert ref_grp == (0, n_reads) and sum(grp) == n_reads, (ref_grp, grp)
    if block == "1":
        assert grp[0] == 0
    else:
        assert grp[0] > (0.05 if batch == "1" else 0.3) * n_reads, (grp, n_reads)


@pytest.mark.parametrize("opts", [dict(noop=True), dict(chunksize=1), dict(chunksize=7), dict(nolinear=True)],
                         ids=["noop", "max_frags1", "max_frags7", "nolinear"])
def test_options_and_chunk_sizes(inputs, off, monkeypatch, opts):
    """noop (no unspliced_mates, nothing handed), chunks of 1 and of 7 fragments (a chunk ends inside a
    region a parse thread grouped, between and at stepped-over fragments), --no-linear."""
    monkeypatch.setenv("FC2_BGZF_BATCH", "3")
    monkeypatch.setenv("FC2_PARSE_BLOCK", "3000")
    _, bam, _ = inputs["paired"]
    ref, _, _ = off(bam, **opts)
    got, _, grp = G.caller_run(bam, group=2, **opts)
    assert got == ref
    assert grp[0] > 0.3 * ref[3][0], grp


@pytest.mark.parametrize("batch,block", SIZES[1:])
@pytest.mark.parametrize("kind", ["single", "paired"])
def test_damaged_record_after_unspliced_reads(inputs, off, monkeypatch, kind, batch, block):
    """A record with corrupt aux data right after a run of unspliced fragments: the fragment before it is
    not closed by the rows (its closer is not usable), and the error is the host's, after the same
    fragments and with the same counts."""
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    monkeypatch.setenv("FC2_PARSE_BLOCK", block)
    _, _, bad = inputs[kind]
    ref, _, _ = off(bad)
    assert ref[2][0] == "error" and "corrupted aux data" in ref[2][1], ref[2]
    assert len(ref[0]) > 100
    got, _, grp = G.caller_run(bad, group=2)
    assert got == ref, (got[2], ref[2], got[3], ref[3])
    assert grp[0] > 0


def _cli(tmp_path, monkeypatch, capfd, fa, bam, group, extra, tag):
    monkeypatch.setattr(cli, "_gpu_group", lambda: group)
    monkeypatch.setenv("FC2_CALLER_TIMING", "1")
    out = str(tmp_path / tag)
    capfd.readouterr()
    assert cli.main(["-G", fa, "-o", out, "-n", "test", "-q"] + extra + [bam], evaluator_factory=oracle_evaluator_factory) == 0
    err = capfd.readouterr().err
    m = re.search(r"gpu group: (\d+) fragments closed on the device, (\d+) grouped on the host", err)
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f != "run.log"}
    counts = counters(out)                              # run.log's "find_circ <counter>=<value>" lines
    return files, counts, (int(m.group(1)), int(m.group(2))) if m else None


@pytest.mark.parametrize("extra", [[], ["-B"], ["--noop"]], ids=["plain", "bam_out", "noop"])
def test_command_line_writes_the_same_bytes(inputs, tmp_path, monkeypatch, capfd, extra):
    """Every output file byte for byte, and run.log's counts, with the setting off and at 2; with -B the
    records are written while they are read, on the reader's own thread, and nothing is stepped over."""
    monkeypatch.setenv("FC2_BGZF_BATCH", "3")
    monkeypatch.setenv("FC2_PARSE_BLOCK", "3000")
    fa, bam, _ = inputs["paired"]
    ref_files, ref_counts, ref_grp = _cli(tmp_path, monkeypatch, capfd, fa, bam, 0, extra, "off")
    files, counts, grp = _cli(tmp_path, monkeypatch, capfd, fa, bam, 2, extra, "on")
    assert sorted(files) == sorted(ref_files) and len(files) >= 4
    for f in files:
        assert files[f] == ref_files[f], f
    assert counts == ref_counts and counts["total_mates"] > 2000, (counts, ref_counts)
    assert ref_grp is None
    if extra == ["-B"]:
        assert grp is not None and grp[0] == 0, grp
        assert "spliced_alignments.bam" in files
    else:
        assert grp is not None and grp[0] > 500, grp
    if not extra:
        assert files["lin_splice_sites.bed"].count(b"\n") > 50


def test_fc2_gpu_group_is_opt_in(monkeypatch):
    for v, want in ((None, 0), ("1", 1), ("0", 0), ("2", 0), ("yes", 0), ("", 0)):
        if v is None:
            monkeypatch.delenv("FC2_GPU_GROUP", raising=False)
        else:
            monkeypatch.setenv("FC2_GPU_GROUP", v)
        assert cli._gpu_group() == want


def test_text_hand_back_steps_over_nothing(inputs, monkeypatch):
    """fc2_ingest_next groups on the reader's own thread and wants every record's text: nothing is skipped."""
    from find_circ2_amd.ingest import NativeIngest
    monkeypatch.setenv("FC2_BGZF_BATCH", "3")
    res = []
    for group in (0, 2):
        ing = NativeIngest(inputs["single"][1], True)
        ing.set_gpu_group(group)
        n = 0
        while not ing.eof:
            n += len(ing.next_chunk(13, False, False, 500))
        c = ing.counts
        res.append((n, tuple(getattr(c, f) for f, _ in c._fields_), ing.group_counts()))
        ing.close()
    assert res[0] == res[1] and res[0][0] > 500 and res[0][2][0] == 0
