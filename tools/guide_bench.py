"""Guide-tree benchmark (reported, not gated): a run without -t next to the same run with -t on the tree it wrote, on the synthetic families
of bench.py (10 000 x 10 kbp nucleotide, 5 000 x 2 kaa protein; the 100 000-sequence family is over the cap of 16 384 sequences).
Prints one JSON line per family:

  count_ms, pairs_ms, download_ms, upgma_ms, text_ms   the five phases of the tree, as the run's -v line reports them (upload + count kernel,
                                                       all-pairs kernel, download of the matrix, distances + UPGMA on the host, Newick text)
  wall_built_s                                         the whole run without -t (process start to exit)
  wall_given_s                                         the same run with -t on the written tree
  same_output                                          the two alignments are one file, byte for byte

Each run is made once: one run, no repeats.

    python tools/guide_bench.py [--configs rnasim10k,protein5k] [--leaves N] [--length L] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")


def _run(cmd, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return wall, r.stderr


def _md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="rnasim10k,protein5k")
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--limit", type=int, default=600, help="time limit of each run, seconds")
    a = ap.parse_args()
    import bench
    import __graft_entry__ as g

    for name in a.configs.split(","):
        cfg = dict(bench.CONFIGS[name])
        if cfg["kind"] != "family" or (a.leaves or cfg["leaves"]) > 16384:
            raise SystemExit(f"{name}: not a family of at most 16384 sequences")
        cfg["workload"] = "calibrated"
        if a.leaves:
            cfg["leaves"] = a.leaves
        if a.length:
            cfg["length"] = a.length
        with tempfile.TemporaryDirectory(prefix="twl_guide_bench_") as d:
            t0 = time.perf_counter()
            _, fasta = bench.write_family(cfg, d)
            print(f"[guide_bench] {name}: family of {cfg['leaves']} x {cfg['length']} written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            built, given, tree = os.path.join(d, "built.aln"), os.path.join(d, "given.aln"), os.path.join(d, "built.nwk")
            wall_built, err = _run([EXE, "-i", fasta, "-o", built, "--write-tree", tree, "--type", cfg["type"], "-v"], a.limit)
            m = re.search(r"Guide tree of (\d+) sequences \(ms\): upload \+ count ([\d.e+-]+), all pairs ([\d.e+-]+), download ([\d.e+-]+), UPGMA ([\d.e+-]+), text ([\d.e+-]+)", err)
            if not m:
                raise SystemExit("no guide-tree line in the run's -v output:\n" + err[-2000:])
            print(f"[guide_bench] {name}: run without -t {wall_built:.2f} s", file=sys.stderr, flush=True)
            wall_given, _ = _run([EXE, "-t", tree, "-i", fasta, "-o", given, "--type", cfg["type"], "-v"], a.limit)
            line = json.dumps({
                "workload": f"{name}: {cfg['leaves']} sequences x {cfg['length']}, type {cfg['type']}", "runs": "one run, no repeats",
                "sequences": int(m.group(1)), "count_ms": float(m.group(2)), "pairs_ms": float(m.group(3)), "download_ms": float(m.group(4)),
                "upgma_ms": float(m.group(5)), "text_ms": float(m.group(6)),
                "wall_built_s": round(wall_built, 3), "wall_given_s": round(wall_given, 3), "same_output": _md5(built) == _md5(given),
                "tree_bytes": os.path.getsize(tree), "library_sources": g.source_hash()})
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
