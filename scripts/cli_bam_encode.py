"""The command line with -B on SAM text from a stdin pipe (the documented `bwa mem ... | cli ... -B` shape), with
and without spliced_alignments.bam's records encoded on the GPU (FC2_GPU_BAM_ENCODE; DESIGN.md §5 "BAM records
from SAM text on the device"), on the inputs of scripts/cli_steady.py: for every size and every pool setting
(the default pools; pinned to --pinned CPUs) the cases -- the zlib writer, FC2_GPU_BAM=1, FC2_GPU_BAM=1 with
FC2_GPU_BAM_ENCODE=1 -- are run interleaved, --reps rounds of one clean run per case, then one FC2_CALLER_TIMING
run per case (the per-stage CPU seconds, the reading thread's among them).  Every record: loop seconds, process
wall, the batches and pieces run.log counts; the first round's also the SHA-256 of the BAM's inflated stream.
With --bam-input the same cases run on the BAM of the same reads (where the stage does nothing): the figures to
hold against another build's.  One JSON line a run.  Measurement infrastructure (not part of the product).

usage: python scripts/cli_bam_encode.py [--sizes 2000000] [--reps 3] [--pinned 4] [--bam-input]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pinned", type=int, default=4)
    ap.add_argument("--bam-input", action="store_true")
    a = ap.parse_args()
    from cli_bam_tiles import inflated_sha256
    from cli_steady import log, prepare, run_cli
    sizes = [int(x) for x in a.sizes.split(",")]
    cases = [("zlib", {}), ("gpu_bam", {"FC2_GPU_BAM": "1"}),
             ("gpu_bam_encode", {"FC2_GPU_BAM": "1", "FC2_GPU_BAM_ENCODE": "1"})]
    if a.bam_input:
        cases = cases[:2]
    d = tempfile.mkdtemp(prefix="fc2_bamenc_", dir="/tmp")
    try:
        fa, bams, sams, info = prepare(d, sizes, keep_sam=True, keep_sam_sizes=sizes)
        print(json.dumps({"prepare": info}), flush=True)
        inputs = bams if a.bam_input else sams
        run_cli(fa, bams[min(sizes)], os.path.join(d, "warm"), 0)       # builds genome.fa.byo_index
        for n in sorted(sizes):
            for threads in (0, a.pinned):
                for r in list(range(a.reps)) + ["timing"]:
                    for name, env in cases:
                        out = os.path.join(d, "o_%d_%s_%d_%s" % (n, name, threads, r))
                        x = run_cli(fa, inputs[n], out, threads, extra=["-B"], timing=(r == "timing"), env_extra=env)
                        ph = x["phases_s"]
                        rec = {"size": n, "input": "bam" if a.bam_input else "sam", "case": name, "cpus": threads or "default",
                               "rep": r, "loop_s": x["loop_s"], "process_wall_s": x["process_wall_s"],
                               "bam_bytes": x["output_bytes"].get("spliced_alignments.bam"),
                               "bam_enc_gpu_batches": ph.get("bam_enc_gpu_batches"),
                               "bam_enc_host_batches": ph.get("bam_enc_host_batches"),
                               "bam_gpu_pieces": ph.get("bam_gpu_pieces"), "bam_cpu_pieces": ph.get("bam_cpu_pieces"),
                               "stages_s": x["stages_s"], "cpu_s_per_stage": x["cpu_s_per_stage"]}
                        if r == 0:
                            rec["inflated_sha256"] = inflated_sha256(os.path.join(out, "spliced_alignments.bam"))
                        print(json.dumps(rec), flush=True)
                        log(n, name, threads, r, "loop", x["loop_s"], "wall", x["process_wall_s"])
                        shutil.rmtree(out, ignore_errors=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
