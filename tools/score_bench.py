"""--score benchmark (reported, not gated): a family of tools/true_family.py aligned with -t, the same command without --score and with it,
alternated, `--reps` times each.  Prints one JSON line per run:

  flag                      whether the run carried --score -v
  wall_s                    process start to exit
  pack_ms, columns_ms, pairs_ms   the three kernel phases of the score (HIP-event times, the run's -v line "Score kernels (ms)")
  score_all_ms              the whole scoring step on the host's clock: the upload of the rows into a store, the kernels, the read-back
  rows, columns, score      of the run's "score:" line
and per shape one summary line: the medians of both walls, their difference (what the flag adds) and the spread of each.

    python tools/score_bench.py [--config nuc10k|prot5k|both] [--leaves N] [--length L] [--reps 3] [--out FILE]

The shapes: nuc10k = 10 000 x 10 kbp, type n; prot5k = 5 000 x 2 kaa, type p.  tools/true_family.py evolves four letters; the protein family is that
family written in the amino acids A, L, G, K: the aligner and the score run their protein paths (21 classes, 231 products), on a composition
that no real protein has."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
SHAPES = {"nuc10k": (10000, 10000, "n"), "prot5k": (5000, 2000, "p")}


def _run(cmd, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return wall, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["nuc10k", "prot5k", "both"])
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--limit", type=int, default=600, help="time limit of each run, seconds")
    a = ap.parse_args()
    import __graft_entry__ as g
    import true_family as TF

    def emit(rec):
        line = json.dumps({**rec, "library_sources": g.source_hash()})
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for name in (["nuc10k", "prot5k"] if a.config == "both" else [a.config]):
        leaves, length, seq_type = SHAPES[name]
        leaves, length = a.leaves or leaves, a.length or length
        with tempfile.TemporaryDirectory(prefix="twl_score_bench_") as d:
            t0 = time.perf_counter()
            newick, seqs, _ = TF.make_true_family(leaves, length, seed=1, with_truth=False)
            if seq_type == "p":
                seqs = [(nm, s.translate(str.maketrans("ACGT", "ALGK"))) for nm, s in seqs]
            fam = os.path.join(d, "fam")
            TF.write_family(fam, newick, seqs, [])
            print(f"[score_bench] family of {leaves} x {length} written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            workload = f"{name}: {leaves} sequences x {length}, type {seq_type}, family of tools/true_family.py seed 1, -t"
            out = os.path.join(d, "out.aln")
            base = [EXE, "-t", os.path.join(fam, "t.nwk"), "-i", os.path.join(fam, "s.fa"), "-o", out, "--type", seq_type]
            walls = {False: [], True: []}
            kernels = []
            for rep in range(a.reps):
                for flag in (False, True):
                    wall, err = _run(base + (["--score", "-v"] if flag else []), a.limit)
                    rec = {"workload": workload, "rep": rep, "flag": flag, "wall_s": round(wall, 3)}
                    if flag:
                        line = re.search(r"score: rows (\d+) columns (\d+) pairs (\d+) letters (\d+) gapcols (\d+) runs (\d+) terminal (\d+)/(\d+) score (\S+) per_pair (\S+)", err)
                        ph = re.search(r"Score kernels \(ms\): pack ([\d.]+), columns ([\d.]+), pairs ([\d.]+); all with the upload of the rows ([\d.]+)", err)
                        if not line or not ph:
                            raise SystemExit("a line is missing in the run's output:\n" + err[-3000:])
                        rec.update(rows=int(line.group(1)), columns=int(line.group(2)), runs=int(line.group(6)), score=float(line.group(9)), per_pair=float(line.group(10)),
                                   pack_ms=float(ph.group(1)), columns_ms=float(ph.group(2)), pairs_ms=float(ph.group(3)), score_all_ms=float(ph.group(4)))
                        kernels.append(rec)
                    walls[flag].append(wall)
                    emit(rec)
                    os.remove(out)
            med = {f: statistics.median(w) for f, w in walls.items()}
            emit({"workload": workload, "summary": True, "reps": a.reps, "wall_s_median": round(med[False], 3), "wall_score_s_median": round(med[True], 3),
                  "added_s": round(med[True] - med[False], 3), "wall_s_range": [round(min(walls[False]), 3), round(max(walls[False]), 3)],
                  "wall_score_s_range": [round(min(walls[True]), 3), round(max(walls[True]), 3)],
                  **{k + "_median": round(statistics.median(r[k] for r in kernels), 3) for k in ("pack_ms", "columns_ms", "pairs_ms", "score_all_ms")}})


if __name__ == "__main__":
    main()
