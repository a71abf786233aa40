"""The command line with -B and both GPU writers at level 2 over a grid of search efforts (FC2_GPU_BAM_DEPTH / _NICE,
FC2_GPU_GZIP_DEPTH / _NICE; DESIGN.md §5 "Search effort at level 2"), on the inputs of scripts/cli_steady.py.
A grid entry D:N:P adds FC2_GPU_BAM_PASSES / FC2_GPU_GZIP_PASSES (DESIGN.md §5 "Priced passes at level 2"); :D:N left
empty (::P) leaves the search at level 2's own.  Part "sizes": one run per setting, without and with the tiles (FC2_GPU_BAM_TILE, FC2_GPU_BAM_HISTORY,
FC2_GPU_GZIP_HISTORY), each file's size against the CPU writers' of a default run (zlib level 6 for
spliced_alignments.bam, libdeflate level 1 for spliced_reads.fastq.gz) and the SHA-256 of what each file holds
against that run's.  Part "loop": --chosen D:N against level 2 alone, interleaved, --reps clean runs each: loop
seconds and process wall.  --keep DIR: the default run's two compressed files are copied there (inputs of
scripts/deflate_search_bench.py).  One JSON line a run.  Measurement infrastructure (not part of the product).

usage: python scripts/cli_deflate_search.py [--sizes 2000000] [--grid 8:258,16:258,32:258,64:258,128:258,32:32]
                                            [--chosen 32:258] [--reps 3] [--keep DIR] [--parts sizes,loop]
                                            [--writers both|bam]
--writers bam: only spliced_alignments.bam goes to the GPU (the reads file stays with the CPU writer), so the loop
waits for no other kernels than the BAM writer's.
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
    ap.add_argument("--grid", default="8:258,16:258,32:258,64:258,128:258,32:32")
    ap.add_argument("--chosen", default="32:258")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tile", type=int, default=16320)
    ap.add_argument("--hist", type=int, default=32768)
    ap.add_argument("--keep", default="")
    ap.add_argument("--parts", default="sizes,loop")
    ap.add_argument("--writers", default="both", choices=["both", "bam"])
    a = ap.parse_args()
    from cli_bam_tiles import inflated_sha256
    from cli_steady import log, prepare, run_cli
    sizes = [int(x) for x in a.sizes.split(",")]
    parts = a.parts.split(",")
    level2 = {"FC2_GPU_BAM": "1", "FC2_GPU_BAM_LEVEL": "2", "FC2_GPU_GZIP": "1", "FC2_GPU_GZIP_LEVEL": "2"}
    tiles = {"FC2_GPU_BAM_TILE": str(a.tile), "FC2_GPU_BAM_HISTORY": str(a.hist), "FC2_GPU_GZIP_HISTORY": str(a.hist)}
    if a.writers == "bam":                          # (spliced_reads.fastq.gz stays with the CPU writer)
        level2 = {k: v for k, v in level2.items() if "BAM" in k}
        tiles = {k: v for k, v in tiles.items() if "BAM" in k}

    def search(setting):
        d, n, p = (setting.split(":") + [""])[:3]
        both = {"FC2_GPU_BAM_DEPTH": d, "FC2_GPU_BAM_NICE": n, "FC2_GPU_GZIP_DEPTH": d, "FC2_GPU_GZIP_NICE": n,
                "FC2_GPU_BAM_PASSES": p, "FC2_GPU_GZIP_PASSES": p}
        return {k: v for k, v in both.items() if a.writers == "both" or "BAM" in k}

    d = tempfile.mkdtemp(prefix="fc2_search_", dir="/tmp")
    try:
        fa, bams, _, info = prepare(d, sizes)
        print(json.dumps({"prepare": info}), flush=True)
        run_cli(fa, bams[min(sizes)], os.path.join(d, "warm"), 0)       # builds genome.fa.byo_index
        for n in sorted(sizes):
            ref = {}

            def one(name, env, rep, sha):
                out = os.path.join(d, "o_%d_%s_%s" % (n, name, rep))
                x = run_cli(fa, bams[n], out, 0, extra=["-B"], env_extra=env)
                ph = x["phases_s"]
                rec = {"size": n, "case": name, "writers": a.writers, "rep": rep, "loop_s": x["loop_s"], "process_wall_s": x["process_wall_s"],
                       "bam_bytes": x["output_bytes"].get("spliced_alignments.bam"),
                       "gz_bytes": x["output_bytes"].get("spliced_reads.fastq.gz"),
                       "bam_gpu_pieces": ph.get("bam_gpu_pieces"), "bam_cpu_pieces": ph.get("bam_cpu_pieces"),
                       "gzip_gpu_pieces": ph.get("gzip_gpu_pieces"), "gzip_cpu_pieces": ph.get("gzip_cpu_pieces"),
                       "as_run": {k: ph[k] for k in sorted(ph) if k.startswith(("bam_gpu_", "gzip_gpu_")) and "pieces" not in k},
                       "stages_s": x["stages_s"]}
                if sha:
                    rec["holds"] = {f: inflated_sha256(os.path.join(out, f)) for f in ("spliced_alignments.bam", "spliced_reads.fastq.gz")}
                if name == "cpu":
                    ref.update(bam=rec["bam_bytes"], gz=rec["gz_bytes"], holds=rec.get("holds"))
                    if a.keep:
                        os.makedirs(a.keep, exist_ok=True)
                        for f in ("spliced_alignments.bam", "spliced_reads.fastq.gz"):
                            shutil.copy(os.path.join(out, f), os.path.join(a.keep, f))
                elif ref:
                    rec["bam_over_zlib6"] = round(rec["bam_bytes"] / ref["bam"], 4)
                    rec["gz_over_libdeflate1"] = round(rec["gz_bytes"] / ref["gz"], 4)
                    if sha:
                        rec["holds_the_cpu_runs_bytes"] = rec["holds"] == ref["holds"]
                        del rec["holds"]
                print(json.dumps(rec), flush=True)
                log(n, name, rep, "loop", x["loop_s"], "wall", x["process_wall_s"], "bam", rec["bam_bytes"], "gz", rec["gz_bytes"])
                shutil.rmtree(out, ignore_errors=True)

            if "sizes" in parts or a.keep:
                one("cpu", {}, 0, True)
            if "sizes" in parts:
                for tag, extra in (("", {}), ("_tiles", tiles)):
                    one("level2" + tag, dict(level2, **extra), 0, True)
                    for g in a.grid.split(","):
                        one("search_%s%s" % (g.replace(":", "_"), tag), dict(level2, **extra, **search(g)), 0, True)
            if "loop" in parts:
                for r in range(a.reps):
                    for tag, extra in (("", {}), ("_tiles", tiles)):
                        one("level2" + tag, dict(level2, **extra), "loop%d" % r, False)
                        one("search_%s%s" % (a.chosen.replace(":", "_"), tag), dict(level2, **extra, **search(a.chosen)),
                            "loop%d" % r, False)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
