"""--adjust-direction benchmark (reported, not gated): the family of bench.py's default configuration, 10 000 sequences x 10 kbp, with every
record i with i % 3 == 1 reverse-complemented, aligned with --adjust-direction next to the same binary without the flag on the unreversed
file; both with -t on the family's own tree.  Prints one JSON line:

  count_ms, seed_groups_ms, permute_ms, opposite_ms, assign_ms, download_ms   the device phases of the decision, as the run's -v line reports them
                                                                              (twl_guide_set_timing and twl_guide_set_strand_timing)
  prim_ms                                       the spanning tree over the seeds, on the host
  assign_bins_per_s                             N * S * 2 strands * bins / assign_ms: what the two-strand tile body compares per second
  reversed, wrong                               records the run turned; records whose direction is not the planted one
  wall_flag_s / wall_plain_s                    the whole run with the flag on the planted file / without it on the original file (process start to exit)
  same_output                                   the two alignments are one file apart from the _R_ names
Each run is made once: one run, no repeats.

    python tools/strand_bench.py [--leaves N] [--length L] [--seeds S] [--out FILE]
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
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _run(cmd, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return wall, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--seeds", type=int, default=0, help="--direction-seeds (default: the run's own default)")
    ap.add_argument("--out", default="", help="append the JSON line to this file as well")
    ap.add_argument("--limit", type=int, default=600, help="time limit of each run, seconds")
    a = ap.parse_args()
    import bench
    import __graft_entry__ as g

    cfg = dict(bench.CONFIGS["rnasim10k"])
    cfg["workload"] = "calibrated"
    if a.leaves:
        cfg["leaves"] = a.leaves
    if a.length:
        cfg["length"] = a.length
    with tempfile.TemporaryDirectory(prefix="twl_strand_bench_") as d:
        t0 = time.perf_counter()
        tree, fasta = bench.write_family(cfg, d)
        planted, names, plant = os.path.join(d, "planted.fa"), [], []
        with open(fasta, "rb") as f, open(planted, "wb") as out:
            recs = f.read().split(b">")[1:]
            for i, rec in enumerate(recs):
                name, seq = rec.split(b"\n")[:2]
                names.append(name.decode())
                plant.append("-" if i % 3 == 1 else "+")
                out.write(b">" + name + b"\n" + (seq.translate(COMP)[::-1] if i % 3 == 1 else seq) + b"\n")
        print(f"[strand_bench] family of {cfg['leaves']} x {cfg['length']} written and planted in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        flag, plain, dirs = os.path.join(d, "flag.aln"), os.path.join(d, "plain.aln"), os.path.join(d, "dirs.tsv")
        seeds = ["--direction-seeds", str(a.seeds)] if a.seeds else []
        wall_flag, err = _run([EXE, "-t", tree, "-i", planted, "-o", flag, "--type", "n", "-v", "--adjust-direction", "--write-directions", dirs, *seeds], a.limit)
        wall_plain, _ = _run([EXE, "-t", tree, "-i", fasta, "-o", plain, "--type", "n", "-v"], a.limit)
        m = re.search(rf"Directions of (\d+) sequences \(ms\): upload \+ count {NUM}, seeds' shared counts {NUM}, permute {NUM}, opposite {NUM}, assign {NUM}, download {NUM}, "
                      rf"spanning tree {NUM}", err)
        s = re.search(r"Directions: (\d+) of \d+ sequences lie reversed and are reverse-complemented \((\d+) seeds", err)
        if not m or not s:
            raise SystemExit("no directions line in the run's -v output:\n" + err[-2000:])
        got = dict(l.split("\t") for l in open(dirs).read().splitlines())
        n, S = int(m.group(1)), int(s.group(2))
        same = open(flag, "rb").read().replace(b">_R_", b">") == open(plain, "rb").read()
        rec = {"workload": f"rnasim10k: {cfg['leaves']} sequences x {cfg['length']}, type n, every third record reversed", "runs": "one run, no repeats", "sequences": n, "seeds": S,
               "count_ms": float(m.group(2)), "seed_groups_ms": float(m.group(3)), "permute_ms": float(m.group(4)), "opposite_ms": float(m.group(5)), "assign_ms": float(m.group(6)),
               "download_ms": float(m.group(7)), "prim_ms": float(m.group(8)), "assign_bins_per_s": n * S * 2 * 4096 / (float(m.group(6)) / 1e3), "reversed": int(s.group(1)),
               "wrong": sum(1 for nm, p in zip(names, plant) if got.get(nm) != p), "wall_flag_s": round(wall_flag, 3), "wall_plain_s": round(wall_plain, 3), "same_output": same,
               "library_sources": g.source_hash()}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
