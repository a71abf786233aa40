"""The parse threads stepping over the fragments of SAM text whose rows say the device closed them
(fc2_ingest_set_gpu_sam_group; csrc/fc2_ingest.cpp sam_split_loop / sam_parse_loop), without a GPU: at the test
setting 2 the host twin fills the slots' rows, so the splitter's slots and the parse-thread logic are the ones a
device's rows drive.  The native read loop and the command line over SAM text shaped like the steady-state
generator's -- 60 % unspliced fragments in runs, unmapped lines and mates, secondaries -- with parse blocks from one
line's length upward, so heads, closers and whole fragments fall on every block edge: the same pairs, read parts,
text, counters and errors as with the setting off, and the same files byte for byte."""
import os
import re

import pytest

import group_inputs as G
import sam_group_helpers as H
from find_circ2_amd import _native as N
from find_circ2_amd import cli
from oracle_engine import oracle_evaluator_factory
from test_ingest import counters

# FC2_PARSE_BLOCK: one byte (every block is one line: nothing can be stepped over -- a placeholder needs a mapped
# line before it and the next fragment's head behind it in its block), about one line, a few lines, many
BLOCKS = ["1", "200", "700", "3000", "20000"]


def _split(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    k = next(i for i, l in enumerate(lines) if not l.startswith("@"))
    return lines[:k], lines[k:-1]


def _write(path, head, body):
    with open(path, "w", newline="") as fh:
        fh.write("\n".join(head + body) + "\n")
    return path


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_group_host")
    out = {}
    for kind, paired in (("single", False), ("paired", True)):
        sam = str(d / (kind + ".sam"))
        out[kind] = (G.group_sam(sam, 1500, 21 + paired, paired), sam)
    fa, sam = out["paired"]
    head, body = _split(sam)
    # line ends and blank lines the host takes in its stride and the rule leaves alone; 3,000 blank lines in a row are
    # more lines than a small block's slot has rows for
    odd = []
    for k, l in enumerate(body):
        odd.append(l + "\r" if k % 37 == 5 else l)
        if k % 53 == 7:
            odd.append("" if k % 2 else " ")
        if k == len(body) // 2:
            odd += [""] * 3000
    out["odd"] = (fa, _write(str(d / "odd.sam"), head, odd))
    name = lambda l: l.split("\t", 1)[0]
    # a CIGAR byte outside the set in the second line of a two-line unspliced fragment past the middle
    k = next(i for i in range(len(body) // 2, len(body) - 1)
             if name(body[i]).startswith("u") and name(body[i + 1]) == name(body[i]) and name(body[i - 1]) != name(body[i]))
    f = body[k + 1].split("\t")
    f[5] = "30M1Q29M"
    out["bad_inside"] = (fa, _write(str(d / "bad_inside.sam"), head, body[:k + 1] + ["\t".join(f)] + body[k + 2:]))
    # nine tabs in the first line after three unspliced fragments in a row
    run, k = 0, len(body) // 2
    while not (run >= 3 and not name(body[k])[0] in "ux" and name(body[k]) != name(body[k - 1])):
        if name(body[k]) != name(body[k - 1]):
            run = run + 1 if name(body[k]).startswith("u") else 0
        k += 1
    out["bad_after"] = (fa, _write(str(d / "bad_after.sam"), head, body[:k] + ["\t".join(body[k].split("\t")[:10])] + body[k + 1:]))
    return out


@pytest.fixture(scope="module")
def off(inputs):
    """The runs with the setting off, one per (input, options), shared by the tests."""
    cache = {}

    def run(path, **opts):
        key = (path, tuple(sorted(opts.items())))
        if key not in cache:
            cache[key] = H.caller_run(path, **opts)
        return cache[key]
    return run


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("kind", ["single", "paired", "odd"])
def test_read_loop_gives_the_same_fragments(inputs, off, monkeypatch, kind, block):
    _, sam = inputs[kind]
    ref, ref_grp = off(sam)                             # (blocks of 4 MiB: the cut of the blocks changes nothing)
    monkeypatch.setenv("FC2_PARSE_BLOCK", block)
    got, grp = H.caller_run(sam, sam_group=2)
    assert got == ref
    n_reads = ref[3][0]
    assert len(ref[0]) > 500 and ref_grp == (0, n_reads) and sum(grp) == n_reads, (ref_grp, grp)
    if block == "1":
        assert grp[0] == 0
    elif int(block) >= 700:                             # a few lines a block: a mapped line, a head and its closer fit now and then
        assert grp[0] > 0


@pytest.mark.parametrize("kind", ["single", "paired", "odd"])
def test_one_block_steps_over_every_fragment_the_rows_close(inputs, off, kind):
    """The whole input in one block: a row with state 1 has a mapped line before it, and the fragment before it ends
    where it begins, so the loop meets every such row at a line start and takes it -- as many as the rule closes."""
    _, sam = inputs[kind]
    ref, _ = off(sam)
    got, grp = H.caller_run(sam, sam_group=2)
    assert got == ref
    body = open(sam, "rb").read()
    while body.startswith(b"@"):
        body = body[body.index(b"\n") + 1:]
    _, _, _, frags = H.group_host(body)                 # (the helpers' table numbers the same names otherwise: equal refIDs stay equal)
    assert grp[0] == int(frags["state"].sum()) > 0.3 * ref[3][0], (grp, ref[3][0])


@pytest.mark.parametrize("opts", [dict(noop=True), dict(chunksize=1), dict(chunksize=7), dict(nolinear=True)],
                         ids=["noop", "max_frags1", "max_frags7", "nolinear"])
def test_options_and_chunk_sizes(inputs, off, monkeypatch, opts):
    _, sam = inputs["paired"]
    ref, _ = off(sam, **opts)
    monkeypatch.setenv("FC2_PARSE_BLOCK", "3000")
    got, grp = H.caller_run(sam, sam_group=2, **opts)
    assert got == ref
    assert grp[0] > 0, grp


@pytest.mark.parametrize("block", BLOCKS[1:])
@pytest.mark.parametrize("kind,message", [("bad_inside", "bad CIGAR"), ("bad_after", "malformed SAM line")])
def test_malformed_line_raises_where_it_does_with_the_setting_off(inputs, off, monkeypatch, kind, message, block):
    """A line the parser refuses inside an unspliced fragment, and one right after a run of unspliced fragments: the
    rows close no fragment over or onto such a line, and the error is the host's, after the same fragments and with
    the same counts."""
    _, sam = inputs[kind]
    ref, _ = off(sam)
    assert ref[2][0] == "error" and message in ref[2][1], ref[2]
    assert len(ref[0]) > 100
    monkeypatch.setenv("FC2_PARSE_BLOCK", block)
    got, grp = H.caller_run(sam, sam_group=2)
    assert got == ref, (got[2], ref[2], got[3], ref[3])
    if int(block) >= 700:
        assert grp[0] > 0


def _cli(tmp_path, monkeypatch, capfd, fa, sam, group, extra, tag):
    monkeypatch.setattr(cli, "_gpu_sam_group", lambda options: group)
    monkeypatch.setenv("FC2_CALLER_TIMING", "1")
    out = str(tmp_path / tag)
    capfd.readouterr()
    assert cli.main(["-G", fa, "-o", out, "-n", "test", "-q"] + extra + [sam], evaluator_factory=oracle_evaluator_factory) == 0
    err = capfd.readouterr().err
    m = re.search(r"gpu sam group: (\d+) fragments closed on the device, (\d+) grouped on the host", err)
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f != "run.log"}
    return files, counters(out), (int(m.group(1)), int(m.group(2))) if m else None


@pytest.mark.parametrize("extra", [[], ["-B"], ["--noop"], ["--python-ingest"]], ids=["plain", "bam_out", "noop", "python_ingest"])
def test_command_line_writes_the_same_bytes(inputs, tmp_path, monkeypatch, capfd, extra):
    """Every output file byte for byte, and run.log's counts, with the setting off and at 2; -B writes the records
    while they are read, on the reader's own thread, and --python-ingest never groups on the parse threads: nothing
    is stepped over there."""
    monkeypatch.setenv("FC2_PARSE_BLOCK", "3000")
    fa, sam = inputs["paired"]
    ref_files, ref_counts, ref_grp = _cli(tmp_path, monkeypatch, capfd, fa, sam, 0, extra, "off")
    files, counts, grp = _cli(tmp_path, monkeypatch, capfd, fa, sam, 2, extra, "on")
    assert sorted(files) == sorted(ref_files) and len(files) >= 4
    for f in files:
        assert files[f] == ref_files[f], f
    assert counts == ref_counts and counts["total_mates"] > 2000, (counts, ref_counts)
    assert ref_grp is None
    if extra == ["-B"]:
        assert grp is not None and grp[0] == 0, grp
        assert "spliced_alignments.bam" in files
    elif extra == ["--python-ingest"]:
        assert grp is None or grp[0] == 0, grp
    else:
        assert grp is not None and grp[0] > 0, grp
    if not extra:
        assert files["lin_splice_sites.bed"].count(b"\n") > 50


def test_fc2_gpu_sam_group_is_opt_in(monkeypatch):
    class Options:
        device = "cuda:0"
    for v, want in ((None, 0), ("1", (1, 0)), ("0", 0), ("2", 0), ("yes", 0), ("", 0)):
        if v is None:
            monkeypatch.delenv("FC2_GPU_SAM_GROUP", raising=False)
        else:
            monkeypatch.setenv("FC2_GPU_SAM_GROUP", v)
        assert cli._gpu_sam_group(Options()) == want
    monkeypatch.setenv("FC2_GPU_GROUP", "1")            # the BAM stage's switch does not turn this one on
    monkeypatch.delenv("FC2_GPU_SAM_GROUP", raising=False)
    assert cli._gpu_sam_group(Options()) == 0


def test_a_bam_input_refuses_the_setting(inputs, tmp_path):
    from find_circ2_amd.ingest import NativeIngest
    _, sam = inputs["single"]
    bam = G.bam_of(sam, str(tmp_path / "single.bam"))
    ing = NativeIngest(bam, True)
    with pytest.raises(N.Fc2Error, match="BAM"):
        ing.set_gpu_sam_group(2)
    assert ing.sam_group_counts()[0] == 0
    ing.close()


def test_text_hand_back_steps_over_nothing(inputs):
    """fc2_ingest_next groups on the reader's own thread and wants every line's text: nothing is skipped."""
    from find_circ2_amd.ingest import NativeIngest
    res = []
    for group in (0, 2):
        ing = NativeIngest(inputs["single"][1], False)
        ing.set_gpu_sam_group(group)
        n = 0
        while not ing.eof:
            n += len(ing.next_chunk(13, False, False, 500))
        c = ing.counts
        res.append((n, tuple(getattr(c, f) for f, _ in c._fields_), ing.sam_group_counts()))
        ing.close()
    assert res[0] == res[1] and res[0][0] > 500 and res[0][2][0] == 0
