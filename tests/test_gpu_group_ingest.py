"""The parse threads stepping over the fragments the device closed (fc2_ingest_set_gpu_group;
csrc/fc2_inflate.hip bam_frag_kernel, csrc/fc2_ingest.cpp sam_parse_loop / group_batch) for the BGZF blocks
the GPU inflates: the native read loop hands out the same pairs, read parts, text and counters with the
fragment rows on, with them off, with them and the digest rows together, and with the CPU inflating -- on
a BAM shaped like the steady-state generator's (60 % unspliced fragments) in 3 kB blocks, at batch sizes
that put chunk and batch edges everywhere, with a corrupt aux field planted after a run of unspliced
fragments (the same error after the same fragments) -- and through the command line, whose files are the
same bytes whatever FC2_GPU_GROUP says."""
import os
import re
import subprocess
import sys

import pytest

import group_inputs as G

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Single-end and paired inputs of over 1,300 blocks each (a batch of 1024 leaves the GPU some), the
    paired one also with a damaged record; with what the CPU inflate reads from each."""
    d = tmp_path_factory.mktemp("group_gpu")
    out = {}
    for kind, paired in (("single", False), ("paired", True)):
        sam = str(d / (kind + ".sam"))
        fa = G.group_sam(sam, 6000, 21 + paired, paired)
        bam = G.bam_of(sam, str(d / (kind + ".bam")))
        assert os.path.getsize(bam + ".raw") > 1300 * 3000
        out[kind] = (fa, bam, G.caller_run(bam)[0])
        if paired:
            bad = G.bam_of(sam, str(d / "bad.bam"), damage=0.5)
            out["bad"] = (fa, bad, G.caller_run(bad)[0])
            assert out["bad"][2][2][0] == "error" and "corrupted aux data" in out["bad"][2][2][1]
    return out


@pytest.mark.parametrize("batch", ["1", "3", "1024"])
@pytest.mark.parametrize("kind", ["single", "paired"])
def test_device_rows_give_the_cpu_inflates_fragments(inputs, monkeypatch, kind, batch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    monkeypatch.setenv("FC2_PARSE_BLOCK", "7000")
    _, bam, cpu = inputs[kind]
    n_reads = cpu[3][0]
    on, on_inf, on_grp = G.caller_run(bam, gpu=True, group=1)
    assert on == cpu
    off, off_inf, off_grp = G.caller_run(bam, gpu=True, group=0)
    assert off == cpu
    both, both_inf, both_grp = G.caller_run(bam, gpu=True, group=1, digest=True)
    assert both == cpu
    assert on_inf == off_inf == both_inf and on_inf[0] > 200 and on_inf[1] == 0, (on_inf, off_inf, both_inf)
    assert off_grp == (0, n_reads) and sum(on_grp) == n_reads and both_grp == on_grp, (off_grp, on_grp, both_grp)
    # 60 % of the fragments are unspliced; rows come with the batches the GPU inflated (the batches read
    # before the device was set are the CPU's: with 1024 blocks a batch, more than half of the file), and a
    # batch of one block is a chunk of 3 kB, where few fragments have their neighbours inside the chunk
    share = on_inf[0] / (os.path.getsize(bam + ".raw") / 3000)
    assert share > 0.3 and on_grp[0] > (0.05 if batch == "1" else 0.3) * share * n_reads, (on_grp, n_reads, share)


@pytest.mark.parametrize("batch", ["3", "1024"])
def test_damaged_record_is_the_hosts_error(inputs, monkeypatch, batch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", batch)
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    _, bad, cpu = inputs["bad"]
    on, _, on_grp = G.caller_run(bad, gpu=True, group=1)
    assert on == cpu, (on[2], cpu[2], on[3], cpu[3])
    assert on_grp[0] > 0


@pytest.mark.parametrize("opts", [dict(noop=True), dict(chunksize=7)], ids=["noop", "max_frags7"])
def test_options(inputs, monkeypatch, opts):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("FC2_BGZF_BATCH", "24")
    monkeypatch.setenv("FC2_GPU_INFLATE", "2")
    monkeypatch.setenv("FC2_PARSE_BLOCK", "20000")
    _, bam, _ = inputs["paired"]
    cpu = G.caller_run(bam, **opts)[0]
    on, _, grp = G.caller_run(bam, gpu=True, group=1, **opts)
    assert on == cpu and grp[0] > 0.3 * cpu[3][0]


_CLI = """
import sys
sys.path[:0] = [%r]
from find_circ2_amd import cli
sys.exit(cli.main(sys.argv[1:]))
"""


def _cli(inputs, cache, group, bam_out, inflate="2"):
    """One run of the command line (small batches and parse blocks): its files, its "gpu group:" counts
    and the blocks the GPU inflated; cached per setting."""
    fa, bam, _ = inputs["paired"]
    key = (group, bam_out, inflate)
    if key not in cache:
        env = dict(os.environ, FC2_CALLER_TIMING="1", FC2_GPU_INFLATE=inflate, FC2_BGZF_BATCH="24", FC2_PARSE_BLOCK="20000")
        env.pop("FC2_GPU_GROUP", None)
        env.pop("FC2_GPU_DIGEST", None)
        if group is not None:
            env["FC2_GPU_GROUP"] = group
        o = os.path.join(os.path.dirname(bam), "o_%s_%d_%s" % (group, bam_out, inflate))
        script = _CLI % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run([sys.executable, "-c", script, "-G", fa, "-o", o, "-q"] + (["-B"] if bam_out else []) + [bam],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        m = re.search(r"gpu group: (\d+) fragments closed on the device, (\d+) grouped on the host", r.stderr)
        g = re.search(r"gpu inflate: \d+ batches \(\d+ pinned\), (\d+) blocks on the GPU, (\d+) on the CPU", r.stderr)
        files = {f: open(os.path.join(o, f), "rb").read() for f in sorted(os.listdir(o)) if f != "run.log"}
        cache[key] = (files, (int(m.group(1)), int(m.group(2))) if m else None, (int(g.group(1)), int(g.group(2))) if g else None)
    return cache[key]


_CACHE = {}


@pytest.mark.parametrize("group,bam_out", [("0", False), ("1", False), ("1", True), ("2", False)])
def test_cli_writes_the_same_bytes(inputs, group, bam_out):
    """FC2_GPU_GROUP unset, 0, 1 and another value: every output file byte for byte the same as with the
    CPU inflating (with -B, spliced_alignments.bam among them); fragments are stepped over only at 1, and
    not with -B, whose records are written while they are read, on the reader's own thread."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cpu_files, _, cpu_inf = _cli(inputs, _CACHE, None, bam_out, inflate="0")
    ref_files, ref_grp, ref_inf = _cli(inputs, _CACHE, None, bam_out)
    files, grp, inf = _cli(inputs, _CACHE, group, bam_out)
    assert sorted(files) == sorted(ref_files) == sorted(cpu_files) and len(files) >= (5 if bam_out else 4), sorted(files)
    for f in files:
        assert files[f] == ref_files[f] == cpu_files[f], f
    assert ("spliced_alignments.bam" in files) == bam_out
    assert cpu_inf is None and inf == ref_inf and inf[0] > 100 and inf[1] == 0, (cpu_inf, inf, ref_inf)
    assert ref_grp is None
    if group == "1" and not bam_out:
        assert grp[0] > 0.3 * sum(grp), grp
    elif group == "1":
        assert grp[0] == 0, grp
    else:
        assert grp is None
    assert files["lin_splice_sites.bed"].count(b"\n") > 100
