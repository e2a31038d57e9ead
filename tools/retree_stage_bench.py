"""Benchmark of --iterations 2 --retree-seeds S (reported, not gated), on the synthetic families of bench.py.  Two cases, one JSON line each:

  rnasim100k   100 000 x 1.6 kbp: --tree-seeds 632 --iterations 2 --retree-seeds 632, next to the same run without --iterations
  rnasim10k    10 000 x 10 kbp:   --iterations 2 --retree-seeds 200, next to --iterations 2 alone (the one-stage rebuilt tree)

  kept_columns, columns                                  what the mask kept of the first alignment
  upload_ms, gaps_ms, pack_ms, assign_ms, groups_ms,
  download_ms, upgma_ms, text_ms, clusters               the phases of the rebuilt tree and the smallest, median and largest cluster, as the
                                                         run's -v line reports them
  assign_pair_columns_per_s                              N * S * columns / assign_ms: what the assign kernel compares per second
  wall_staged_s                                          the whole run with --retree-seeds (process start to exit)
  wall_other_s, other                                    the run it stands next to, and which one that is
  one_stage                                              rnasim10k: the phases of the one-stage tree of that other run

Each run is made once, under its own time limit, and a run that fails ends the script: one run, no repeats.

    python tools/retree_stage_bench.py [--cases rnasim100k,rnasim10k] [--leaves N] [--length L] [--out FILE]
"""
import argparse
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
STAGED = (r"Guide tree rebuilt in two stages from the alignment of iteration 1: kept (\d+) of (\d+) columns, (\d+) sequences, (\d+) seeds \(ms\): upload " + NUM + ", gaps " + NUM +
          ", pack " + NUM + ", assign " + NUM + ", groups " + NUM + ", download " + NUM + ", UPGMA " + NUM + ", text " + NUM + r"; clusters: smallest (\d+), median (\d+), largest (\d+)")
ONE = (r"Guide tree rebuilt from the alignment of iteration 1: kept (\d+) of (\d+) columns, (\d+) sequences \(ms\): upload " + NUM + ", gaps " + NUM + ", pack " + NUM +
       ", pairs " + NUM + ", download " + NUM + ", UPGMA " + NUM + ", text " + NUM)
CASES = {"rnasim100k": dict(seeds=632, first=("--tree-seeds", "632"), other="the same run without --iterations", other_iterations=False),
         "rnasim10k": dict(seeds=200, first=(), other="--iterations 2 alone", other_iterations=True)}


def _run(cmd, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return wall, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="rnasim100k,rnasim10k")
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--seeds", type=int, default=0, help="override S (development)")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--limit", type=int, default=300, help="time limit of each run, seconds")
    a = ap.parse_args()
    import bench
    import __graft_entry__ as g

    for name in a.cases.split(","):
        case = CASES[name]
        cfg = dict(bench.CONFIGS[name])
        cfg["workload"] = "calibrated"
        if a.leaves:
            cfg["leaves"] = a.leaves
        if a.length:
            cfg["length"] = a.length
        s = a.seeds or case["seeds"]
        first = ("--tree-seeds", str(s)) if case["first"] else ()
        with tempfile.TemporaryDirectory(prefix="twl_retree_stage_bench_") as d:
            t0 = time.perf_counter()
            _, fasta = bench.write_family(cfg, d)
            print(f"[retree_stage_bench] {name}: family of {cfg['leaves']} x {cfg['length']} written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            staged, other = os.path.join(d, "staged.aln"), os.path.join(d, "other.aln")
            wall_staged, err = _run([EXE, "-i", fasta, "-o", staged, "--iterations", "2", "--retree-seeds", str(s), "--type", cfg["type"], "-v", *first], a.limit)
            m = re.search(STAGED, err)
            if not m:
                raise SystemExit("no two-stage line in the run's -v output:\n" + err[-2000:])
            print(f"[retree_stage_bench] {name}: --iterations 2 --retree-seeds {s} {wall_staged:.2f} s", file=sys.stderr, flush=True)
            wall_other, err_other = _run([EXE, "-i", fasta, "-o", other, "--type", cfg["type"], "-v", *first, *(("--iterations", "2") if case["other_iterations"] else ())], a.limit)
            print(f"[retree_stage_bench] {name}: {case['other']} {wall_other:.2f} s", file=sys.stderr, flush=True)
            kept, columns, n, seeds = (int(x) for x in m.groups()[:4])
            v = [float(x) for x in m.groups()[4:12]]
            rec = {"workload": f"{name}: {cfg['leaves']} sequences x {cfg['length']}, type {cfg['type']}, --iterations 2 --retree-seeds {s}" + (f" --tree-seeds {s}" if first else ""),
                   "runs": "one run, no repeats", "sequences": n, "seeds": seeds, "kept_columns": kept, "columns": columns,
                   "upload_ms": v[0], "gaps_ms": v[1], "pack_ms": v[2], "assign_ms": v[3], "groups_ms": v[4], "download_ms": v[5], "upgma_ms": v[6], "text_ms": v[7],
                   "clusters": [int(x) for x in m.groups()[12:15]], "assign_pair_columns_per_s": n * seeds * columns / (v[3] / 1e3),
                   "wall_staged_s": round(wall_staged, 3), "wall_other_s": round(wall_other, 3), "other": case["other"], "library_sources": g.source_hash()}
            if case["other_iterations"]:
                o = re.search(ONE, err_other)
                if not o:
                    raise SystemExit("no rebuilt-tree line in the other run's -v output:\n" + err_other[-2000:])
                w = [float(x) for x in o.groups()[3:]]
                rec["one_stage"] = {"kept_columns": int(o.group(1)), "columns": int(o.group(2)), "upload_ms": w[0], "gaps_ms": w[1], "pack_ms": w[2], "pairs_ms": w[3],
                                    "download_ms": w[4], "upgma_ms": w[5], "text_ms": w[6]}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
