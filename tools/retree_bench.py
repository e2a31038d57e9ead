"""Benchmark of --iterations 2 (reported, not gated), on the synthetic families of bench.py (10 000 x 10 kbp nucleotide, 5 000 x 2 kaa protein).
Prints one JSON line per family:

  kept_columns, columns                                          what the mask kept of the first alignment
  upload_ms, gaps_ms, pack_ms, pairs_ms, download_ms,
  upgma_ms, text_ms                                              the phases of the rebuilt tree, as the run's -v line reports them
  wall_iterations_s                                              the whole run with --iterations 2 (process start to exit)
  wall_first_s, wall_second_s                                    the two runs it consists of: the run without --iterations that writes its
                                                                 tree, and -t on the final tree of the iterated run
  same_output                                                    the iterated run's alignment and the second of those are one file

Each run is made once, under its own time limit: one run, no repeats.

    python tools/retree_bench.py [--configs rnasim10k,protein5k] [--leaves N] [--length L] [--out FILE]
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
NUM = r"([\d.e+-]+)"
LINE = (r"Guide tree rebuilt from the alignment of iteration 1: kept (\d+) of (\d+) columns, (\d+) sequences \(ms\): upload " + NUM + ", gaps " + NUM + ", pack " + NUM +
        ", pairs " + NUM + ", download " + NUM + ", UPGMA " + NUM + ", text " + NUM)


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
    ap.add_argument("--limit", type=int, default=300, help="time limit of each run, seconds")
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
        with tempfile.TemporaryDirectory(prefix="twl_retree_bench_") as d:
            t0 = time.perf_counter()
            _, fasta = bench.write_family(cfg, d)
            print(f"[retree_bench] {name}: family of {cfg['leaves']} x {cfg['length']} written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            it, first, second = os.path.join(d, "it.aln"), os.path.join(d, "first.aln"), os.path.join(d, "second.aln")
            tree_it, tree_first = os.path.join(d, "it.nwk"), os.path.join(d, "first.nwk")
            wall_it, err = _run([EXE, "-i", fasta, "-o", it, "--iterations", "2", "--write-tree", tree_it, "--type", cfg["type"], "-v"], a.limit)
            m = re.search(LINE, err)
            if not m:
                raise SystemExit("no rebuilt-tree line in the run's -v output:\n" + err[-2000:])
            print(f"[retree_bench] {name}: --iterations 2 {wall_it:.2f} s", file=sys.stderr, flush=True)
            wall_first, _ = _run([EXE, "-i", fasta, "-o", first, "--write-tree", tree_first, "--type", cfg["type"]], a.limit)
            print(f"[retree_bench] {name}: run without --iterations {wall_first:.2f} s", file=sys.stderr, flush=True)
            wall_second, _ = _run([EXE, "-t", tree_it, "-i", fasta, "-o", second, "--type", cfg["type"]], a.limit)
            v = [float(x) for x in m.groups()[3:]]
            line = json.dumps({
                "workload": f"{name}: {cfg['leaves']} sequences x {cfg['length']}, type {cfg['type']}, --iterations 2", "runs": "one run, no repeats",
                "sequences": int(m.group(3)), "kept_columns": int(m.group(1)), "columns": int(m.group(2)),
                "upload_ms": v[0], "gaps_ms": v[1], "pack_ms": v[2], "pairs_ms": v[3], "download_ms": v[4], "upgma_ms": v[5], "text_ms": v[6],
                "wall_iterations_s": round(wall_it, 3), "wall_first_s": round(wall_first, 3), "wall_second_s": round(wall_second, 3),
                "same_output": _md5(it) == _md5(second), "library_sources": g.source_hash()})
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
