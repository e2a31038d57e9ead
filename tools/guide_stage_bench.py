"""Two-stage guide-tree benchmark (reported, not gated): a run with --tree-seeds S next to the same run with -t on the tree it wrote, on the
synthetic families of bench.py.  Prints one JSON line per case (family, S):

  count_ms, assign_ms, groups_ms, download_ms   the device phases of the tree, as the run's -v line reports them from twl_guide_set_timing
                                                (upload + count kernel, assign kernel, group kernels of the clusters and of the seeds, downloads)
  upgma_ms, text_ms                             distances + UPGMA of all clusters and of the seeds on the host, the grafted Newick text
  clusters                                      smallest, median and largest cluster
  assign_bins_per_s                             N * S * padded bins / assign_ms: what the assign kernel compares per second
  wall_built_s / wall_given_s                   the whole run with --tree-seeds (process start to exit) / the same run with -t on the written tree
  same_output                                   the two alignments are one file, byte for byte
  width, band_cells                             of the final alignment, as the run reports them (information, no quality claim)

With --one-stage (families of at most 16 384 sequences) the run without the flag is made as well, in the same session, and reported as
"one_stage": its phases, width and band cells, and pairs_bins_per_s = N (N + 1) / 2 * padded bins / pairs_ms of the all-pairs kernel.
Each run is made once: one run, no repeats.

    python tools/guide_stage_bench.py --config rnasim100k --seeds 632,2528 [--one-stage] [--leaves N] [--length L] [--out FILE]
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


def _result(err):
    m = re.search(r"\(length (\d+)\).*?level kernel: (\d+) pairs, (\d+) band cells", err)
    return {"width": int(m.group(1)), "band_cells": int(m.group(3))} if m else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="rnasim100k")
    ap.add_argument("--seeds", default="632,2528", help="values of S, comma-separated")
    ap.add_argument("--one-stage", action="store_true", help="also the run without --tree-seeds (at most 16384 sequences)")
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--limit", type=int, default=600, help="time limit of each run, seconds")
    a = ap.parse_args()
    import bench
    import __graft_entry__ as g

    cfg = dict(bench.CONFIGS[a.config])
    if cfg["kind"] != "family":
        raise SystemExit(f"{a.config}: not a family")
    cfg["workload"] = "calibrated"
    if a.leaves:
        cfg["leaves"] = a.leaves
    if a.length:
        cfg["length"] = a.length
    bins_pad = 4096 if cfg["type"] == "n" else 7808
    lines = []
    with tempfile.TemporaryDirectory(prefix="twl_guide_stage_bench_") as d:
        t0 = time.perf_counter()
        _, fasta = bench.write_family(cfg, d)
        print(f"[guide_stage_bench] {a.config}: family of {cfg['leaves']} x {cfg['length']} written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        built, given, tree = os.path.join(d, "built.aln"), os.path.join(d, "given.aln"), os.path.join(d, "built.nwk")
        one = None
        if a.one_stage:
            wall_built, err = _run([EXE, "-i", fasta, "-o", built, "--write-tree", tree, "--type", cfg["type"], "-v"], a.limit)
            m = re.search(rf"Guide tree of (\d+) sequences \(ms\): upload \+ count {NUM}, all pairs {NUM}, download {NUM}, UPGMA {NUM}, text {NUM}", err)
            if not m:
                raise SystemExit("no guide-tree line in the run's -v output:\n" + err[-2000:])
            wall_given, _ = _run([EXE, "-t", tree, "-i", fasta, "-o", given, "--type", cfg["type"], "-v"], a.limit)
            n = int(m.group(1))
            one = {"count_ms": float(m.group(2)), "pairs_ms": float(m.group(3)), "download_ms": float(m.group(4)), "upgma_ms": float(m.group(5)), "text_ms": float(m.group(6)),
                   "pairs_bins_per_s": n * (n + 1) / 2 * bins_pad / (float(m.group(3)) / 1e3), "wall_built_s": round(wall_built, 3), "wall_given_s": round(wall_given, 3),
                   "same_output": _md5(built) == _md5(given), **_result(err)}
        for s in [int(x) for x in a.seeds.split(",")]:
            wall_built, err = _run([EXE, "-i", fasta, "-o", built, "--write-tree", tree, "--tree-seeds", str(s), "--type", cfg["type"], "-v"], a.limit)
            m = re.search(rf"Guide tree of (\d+) sequences in two stages, (\d+) seeds \(ms\): upload \+ count {NUM}, assign {NUM}, groups {NUM}, download {NUM}, UPGMA {NUM}, text {NUM}; "
                          r"clusters: smallest (\d+), median (\d+), largest (\d+)", err)
            if not m:
                raise SystemExit("no two-stage line in the run's -v output:\n" + err[-2000:])
            print(f"[guide_stage_bench] {a.config}, S = {s}: run with --tree-seeds {wall_built:.2f} s", file=sys.stderr, flush=True)
            wall_given, _ = _run([EXE, "-t", tree, "-i", fasta, "-o", given, "--type", cfg["type"], "-v"], a.limit)
            n = int(m.group(1))
            rec = {"workload": f"{a.config}: {cfg['leaves']} sequences x {cfg['length']}, type {cfg['type']}", "runs": "one run, no repeats", "sequences": n, "seeds": s,
                   "count_ms": float(m.group(3)), "assign_ms": float(m.group(4)), "groups_ms": float(m.group(5)), "download_ms": float(m.group(6)),
                   "upgma_ms": float(m.group(7)), "text_ms": float(m.group(8)), "clusters": [int(m.group(9)), int(m.group(10)), int(m.group(11))],
                   "assign_bins_per_s": n * s * bins_pad / (float(m.group(4)) / 1e3), "wall_built_s": round(wall_built, 3), "wall_given_s": round(wall_given, 3),
                   "same_output": _md5(built) == _md5(given), "tree_bytes": os.path.getsize(tree), **_result(err), "library_sources": g.source_hash()}
            if one:
                rec["one_stage"] = one
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("".join(l + "\n" for l in lines))


if __name__ == "__main__":
    main()
