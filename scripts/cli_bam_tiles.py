"""The command line with -B and spliced_alignments.bam compressed on the GPU, with and without tiles inside the
blocks (FC2_GPU_BAM_TILE, FC2_GPU_BAM_HISTORY; DESIGN.md §5 "Tiles inside a BGZF block"), on the inputs of
scripts/cli_steady.py: for every size the cases are run interleaved, --reps rounds of one clean run per case,
then one FC2_CALLER_TIMING run per case (the per-stage CPU seconds).  Every record: loop seconds, process wall,
piece counts, tile and history as run.log reports them, the BAM's size; the first round's also the SHA-256 of
the BAM's inflated stream.  One JSON line a run.  Measurement infrastructure (not part of the product).

usage: python scripts/cli_bam_tiles.py [--sizes 2000000,20000000] [--reps 3] [--tile 16320] [--hist 32768]
"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def inflated_sha256(path):
    """SHA-256 of a BGZF file's inflated stream, member after member."""
    h = hashlib.sha256()
    with open(path, "rb") as f:
        z, buf = zlib.decompressobj(31), b""
        while True:
            buf = buf or f.read(1 << 22)
            if not buf:
                break
            h.update(z.decompress(buf))
            buf = z.unused_data if z.eof else b""
            if z.eof:
                z = zlib.decompressobj(31)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000000,20000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tile", type=int, default=16320)
    ap.add_argument("--hist", type=int, default=32768)
    a = ap.parse_args()
    from cli_steady import log, prepare, run_cli
    sizes = [int(x) for x in a.sizes.split(",")]
    tiles = {"FC2_GPU_BAM_TILE": str(a.tile), "FC2_GPU_BAM_HISTORY": str(a.hist)}
    cases = [("level1", {"FC2_GPU_BAM": "1"}), ("level2", {"FC2_GPU_BAM": "1", "FC2_GPU_BAM_LEVEL": "2"}),
             ("level1_tiles", dict({"FC2_GPU_BAM": "1"}, **tiles)),
             ("level2_tiles", dict({"FC2_GPU_BAM": "1", "FC2_GPU_BAM_LEVEL": "2"}, **tiles))]
    d = tempfile.mkdtemp(prefix="fc2_bamtiles_", dir="/tmp")
    try:
        fa, bams, _, info = prepare(d, sizes)
        print(json.dumps({"prepare": info}), flush=True)
        run_cli(fa, bams[min(sizes)], os.path.join(d, "warm"), 0)       # builds genome.fa.byo_index
        for n in sorted(sizes):
            for r in list(range(a.reps)) + ["timing"]:
                for name, env in cases:
                    out = os.path.join(d, "o_%d_%s_%s" % (n, name, r))
                    x = run_cli(fa, bams[n], out, 0, extra=["-B"], timing=(r == "timing"), env_extra=env)
                    rec = {"size": n, "case": name, "rep": r, "loop_s": x["loop_s"], "process_wall_s": x["process_wall_s"],
                           "bam_bytes": x["output_bytes"].get("spliced_alignments.bam"),
                           "bam_gpu_pieces": x["phases_s"].get("bam_gpu_pieces"), "bam_cpu_pieces": x["phases_s"].get("bam_cpu_pieces"),
                           "bam_gpu_level": x["phases_s"].get("bam_gpu_level", 1), "bam_gpu_tile": x["phases_s"].get("bam_gpu_tile"),
                           "bam_gpu_history": x["phases_s"].get("bam_gpu_history"), "stages_s": x["stages_s"],
                           "cpu_s_per_stage": x["cpu_s_per_stage"]}
                    if r == 0:
                        rec["inflated_sha256"] = inflated_sha256(os.path.join(out, "spliced_alignments.bam"))
                    print(json.dumps(rec), flush=True)
                    log(n, name, r, "loop", x["loop_s"], "wall", x["process_wall_s"])
                    shutil.rmtree(out, ignore_errors=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
