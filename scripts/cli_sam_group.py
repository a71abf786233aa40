"""The command line on SAM text from a stdin pipe (the documented `bwa mem ... | cli ...` shape, without -B), with
and without the unspliced fragments closed on the GPU (FC2_GPU_SAM_GROUP; DESIGN.md §5 "Unspliced fragments of SAM
text closed on the device"), on the inputs of scripts/cli_steady.py: for every size and every pool setting (the
default pools; pinned to each of --pinned CPUs) the two cases -- the stage off, the stage on -- are run interleaved,
--reps rounds of one clean run per case, then one FC2_CALLER_TIMING run per case (the per-stage CPU seconds, parse+group among them, the reader's
waits, and the "gpu sam group:" counts).  Every record: loop seconds, process wall, the counts; the first round's
also the SHA-256 of every output file.  The parent commit's figures come from the same script's "off" case run in a
checkout of the parent (it ignores the variable).  One JSON line a run.  Measurement infrastructure (not part of the product).

usage: python scripts/cli_sam_group.py [--sizes 2000000] [--reps 3] [--pinned 4,16]
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def sha_of_outputs(out):
    return {f: hashlib.sha256(open(os.path.join(out, f), "rb").read()).hexdigest()
            for f in sorted(os.listdir(out)) if f != "run.log" and os.path.isfile(os.path.join(out, f))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pinned", default="4,16")
    a = ap.parse_args()
    from cli_steady import log, prepare, run_cli
    sizes = [int(x) for x in a.sizes.split(",")]
    pools = [0] + [int(x) for x in a.pinned.split(",") if x]
    cases = [("off", {}), ("gpu_sam_group", {"FC2_GPU_SAM_GROUP": "1"})]
    d = tempfile.mkdtemp(prefix="fc2_samgrp_", dir="/tmp")
    try:
        fa, bams, sams, info = prepare(d, sizes, keep_sam=True, keep_sam_sizes=sizes)
        print(json.dumps({"prepare": info}), flush=True)
        run_cli(fa, bams[min(sizes)], os.path.join(d, "warm"), 0)       # builds genome.fa.byo_index
        for n in sorted(sizes):
            for threads in pools:
                for r in list(range(a.reps)) + ["timing"]:
                    for name, env in cases:
                        out = os.path.join(d, "o_%d_%s_%d_%s" % (n, name, threads, r))
                        x = run_cli(fa, sams[n], out, threads, timing=(r == "timing"), env_extra=env)
                        err = open(out + ".stderr").read()
                        m = re.search(r"gpu sam group: (\d+) fragments closed on the device, (\d+) grouped on the host", err)
                        rec = {"size": n, "case": name, "cpus": threads or "default", "rep": r, "loop_s": x["loop_s"],
                               "process_wall_s": x["process_wall_s"], "reads": x["reads"], "spans": x["spans"],
                               "stages_s": x["stages_s"], "cpu_s_per_stage": x["cpu_s_per_stage"],
                               "next_phase_ms": x["next_phase_ms"], "upstream_ms": x["upstream_ms"],
                               "sam_group": [int(m.group(1)), int(m.group(2))] if m else None}
                        if r == 0:
                            rec["sha256"] = sha_of_outputs(out)
                        print(json.dumps(rec), flush=True)
                        log(n, name, threads, r, "loop", x["loop_s"], "wall", x["process_wall_s"])
                        shutil.rmtree(out, ignore_errors=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
