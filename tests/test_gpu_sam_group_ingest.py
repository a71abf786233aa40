"""The parse threads stepping over the fragments of SAM text the device closed (fc2_ingest_set_gpu_sam_group;
csrc/fc2_sam_group.hip, csrc/fc2_ingest.cpp sam_split_loop / sam_parse_loop): the native read loop over SAM text from
a file and from a pipe hands out the same pairs, read parts, text, counters and errors with the stage on as with it
off -- at the default parse block and at one so small that heads and closers fall on block edges -- and the command
line, on a file and on a stdin pipe, writes the same bytes and the same run.log counters whatever FC2_GPU_SAM_GROUP
says, with fragments stepped over only at 1 and never with -B."""
import gzip
import os
import re
import subprocess
import sys
import threading

import pytest

import group_inputs as G
import sam_group_helpers as H
from test_ingest import counters

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Single-end and paired SAM text, the paired one also with a CIGAR byte outside the set inside an unspliced
    fragment; with what the loop reads from each with the stage off."""
    d = tmp_path_factory.mktemp("sam_group_gpu")
    out = {}
    for kind, paired in (("single", False), ("paired", True)):
        sam = str(d / (kind + ".sam"))
        fa = G.group_sam(sam, 3000, 41 + paired, paired)
        out[kind] = (fa, sam, H.caller_run(sam)[0])
    fa, sam, _ = out["paired"]
    lines = open(sam).read().split("\n")
    name = lambda l: l.split("\t", 1)[0]
    k = next(i for i in range(len(lines) // 2, len(lines) - 2)
             if name(lines[i]).startswith("u") and name(lines[i + 1]) == name(lines[i]) and name(lines[i - 1]) != name(lines[i]))
    f = lines[k + 1].split("\t")
    f[5] = "30M1Q29M"
    lines[k + 1] = "\t".join(f)
    bad = str(d / "bad.sam")
    open(bad, "w").write("\n".join(lines))
    out["bad"] = (fa, bad, H.caller_run(bad)[0])
    assert out["bad"][2][2][0] == "error" and "bad CIGAR" in out["bad"][2][2][1]
    return out


def from_pipe(sam, run):
    """run('-') with the file's bytes arriving on a pipe at descriptor 0."""
    data = open(sam, "rb").read()
    r, w = os.pipe()
    keep = os.dup(0)
    os.dup2(r, 0)
    os.close(r)

    def feed():
        with os.fdopen(w, "wb") as fh:
            fh.write(data)
    t = threading.Thread(target=feed)
    t.start()
    try:
        return run("-")
    finally:
        os.dup2(keep, 0)
        os.close(keep)
        t.join()


@pytest.mark.parametrize("block", [None, "20000", "700"], ids=["default", "20000", "700"])
@pytest.mark.parametrize("kind", ["single", "paired", "bad"])
def test_device_rows_give_the_same_fragments(inputs, monkeypatch, kind, block):
    if block:
        monkeypatch.setenv("FC2_PARSE_BLOCK", block)
    _, sam, ref = inputs[kind]
    on, grp = H.caller_run(sam, sam_group=(1, 0))
    assert on == ref, (on[2], ref[2], on[3], ref[3])
    assert grp[0] > 0
    if kind != "bad":
        assert sum(grp) == ref[3][0]
    if block is None and kind != "bad":                 # one block: every fragment the rows close (60 % are unspliced)
        assert grp[0] > 0.3 * ref[3][0], (grp, ref[3][0])


@pytest.mark.parametrize("block", [None, "20000"], ids=["default", "20000"])
def test_text_from_a_pipe(inputs, monkeypatch, block):
    if block:
        monkeypatch.setenv("FC2_PARSE_BLOCK", block)
    _, sam, ref = inputs["paired"]
    on, grp = from_pipe(sam, lambda path: H.caller_run(path, sam_group=(1, 0)))
    assert on == ref
    assert grp[0] > 0 and sum(grp) == ref[3][0]


@pytest.mark.parametrize("opts", [dict(noop=True), dict(chunksize=7)], ids=["noop", "max_frags7"])
def test_options(inputs, monkeypatch, opts):
    monkeypatch.setenv("FC2_PARSE_BLOCK", "20000")
    _, sam, _ = inputs["paired"]
    ref = H.caller_run(sam, **opts)[0]
    on, grp = H.caller_run(sam, sam_group=(1, 0), **opts)
    assert on == ref and grp[0] > 0


_CLI = """
import sys
sys.path[:0] = [%r]
from find_circ2_amd import cli
sys.exit(cli.main(sys.argv[1:]))
"""
_CACHE = {}


def _cli(inputs, group, bam_out, pipe, block):
    """One run of the command line: its files, run.log's counters and its "gpu sam group:" counts; cached."""
    fa, sam, _ = inputs["paired"]
    key = (group, bam_out, pipe, block)
    if key not in _CACHE:
        env = dict(os.environ, FC2_CALLER_TIMING="1")
        env.pop("FC2_GPU_SAM_GROUP", None)
        env.pop("FC2_PARSE_BLOCK", None)
        if group is not None:
            env["FC2_GPU_SAM_GROUP"] = group
        if block:
            env["FC2_PARSE_BLOCK"] = block
        o = os.path.join(os.path.dirname(sam), "o_%s_%d_%d_%s" % (group, bam_out, pipe, block))
        script = _CLI % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        cmd = [sys.executable, "-c", script, "-G", fa, "-o", o, "-q"] + (["-B"] if bam_out else [])
        if pipe:
            r = subprocess.run(cmd, env=env, input=open(sam, "rb").read(), capture_output=True, timeout=300)
        else:
            r = subprocess.run(cmd + [sam], env=env, capture_output=True, timeout=300)
        err = r.stderr.decode("latin-1")
        assert r.returncode == 0, err[-3000:]
        m = re.search(r"gpu sam group: (\d+) fragments closed on the device, (\d+) grouped on the host", err)
        files = {f: open(os.path.join(o, f), "rb").read() for f in sorted(os.listdir(o)) if f != "run.log"}
        _CACHE[key] = (files, counters(o), (int(m.group(1)), int(m.group(2))) if m else None)
    return _CACHE[key]


@pytest.mark.parametrize("group,bam_out,pipe,block", [("1", False, False, None), ("1", False, True, None), ("1", False, True, "20000"),
                                                      ("1", True, False, None), ("0", False, False, None), ("2", False, True, None)])
def test_cli_writes_the_same_bytes(inputs, group, bam_out, pipe, block):
    ref_files, ref_counts, ref_grp = _cli(inputs, None, bam_out, False, None)
    files, counts, grp = _cli(inputs, group, bam_out, pipe, block)
    assert sorted(files) == sorted(ref_files) and len(files) >= (5 if bam_out else 4), sorted(files)
    for f in files:
        if block and f.endswith(".gz"):
            # spliced_reads.fastq.gz is one gzip member per range of a chunk, and with small parse blocks a chunk ends
            # where FC2_PIN_MAX blocks are pinned: the members' cut follows the blocks' cut (which a pipe's reads
            # move), the text does not -- test_ingest.same compares this file the same way
            assert gzip.decompress(files[f]) == gzip.decompress(ref_files[f]), f
        else:
            assert files[f] == ref_files[f], f
    assert counts == ref_counts and counts["total_mates"] > 4000
    assert ref_grp is None
    if group == "1" and not bam_out:
        assert grp[0] > 0, grp
    elif group == "1":
        assert grp[0] == 0, grp
    else:
        assert grp is None
    assert files["lin_splice_sites.bed"].count(b"\n") > 100
