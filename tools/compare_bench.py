"""--compare benchmark (reported, not gated): a family of tools/true_family.py with its true alignment, aligned by the modes that compute different
alignments from the same sequences (-t, -t -m 1000, -t --iterations 2, no tree), each run once without --compare and once with it against the
truth.  Prints one JSON line per mode:

  SP, modeler, TC          as the run's "compare:" line reports them (TC as recovered / reference columns)
  upload_ms .. download_ms the four phases of the comparison (the run's -v line "Compare phases (ms)"; the two kernel phases are HIP-event times)
  keys_mb                  the residue keys on the device
  wall_s, wall_compare_s   process start to exit without and with --compare
and, for context only, one line with the time of the per-column numpy oracle (tests/compare_oracle.py) on the first 1 000 rows of the -t output.

    python tools/compare_bench.py [--config rnasim10k|rnasim100k|both] [--leaves N] [--length L] [--modes tree,subtrees,iterations,no_tree]
                                  [--reference truth|tree] [--out FILE]

The shapes: rnasim10k = 10 000 x 10 kbp, rnasim100k = 100 000 x 1.6 kbp (without a tree: --tree-seeds 632).  The true alignment has a column for
every site any branch inserted: 307 896 columns for rnasim10k (a 3 GB file), and far more rows times columns than any machine holds for
rnasim100k.  `--reference tree` therefore compares every mode with the output of the -t run of the same family instead of the truth (no true.aln
is made): what it measures is the comparison's phases at that size and how far the modes' alignments lie from each other, not their quality.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
SHAPES = {"rnasim10k": (10000, 10000), "rnasim100k": (100000, 1600)}


def _run(cmd, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return wall, r.stderr


def mode_args(mode, fam, leaves):
    tree = ["-t", os.path.join(fam, "t.nwk")]
    return {"tree": tree, "subtrees": tree + ["-m", "1000"], "iterations": tree + ["--iterations", "2"] + (["--retree-seeds", "632"] if leaves > 16384 else []),
            "no_tree": ["--tree-seeds", "632"] if leaves > 16384 else []}[mode]


def one_mode(mode, fam, leaves, out, limit, ref):
    base = [EXE, *mode_args(mode, fam, leaves), "-i", os.path.join(fam, "s.fa"), "-o", out, "--type", "n", "-v"]
    wall, _ = _run(base, limit)
    wall_c, err = _run(base + ["--compare", ref], limit)
    line = re.search(r"compare: rows (\d+) .* pairs_out (\d+) pairs_ref (\d+) shared (\d+) SP (\S+) modeler (\S+) TC (\d+)/(\d+) columns (\d+)/(\d+)", err)
    ph = re.search(r"Compare phases \(ms\): upload ([\d.]+), key kernels ([\d.]+), column kernel ([\d.]+), download ([\d.]+), all with reading the reference ([\d.]+); residue keys ([\d.]+) MB", err)
    if not line or not ph:
        raise SystemExit("a line is missing in the run's output:\n" + err[-3000:])
    return {"mode": mode, "rows": int(line.group(1)), "pairs_out": int(line.group(2)), "pairs_ref": int(line.group(3)), "shared": int(line.group(4)), "SP": float(line.group(5)),
            "modeler": float(line.group(6)), "TC": f"{line.group(7)}/{line.group(8)}", "columns": int(line.group(9)), "true_columns": int(line.group(10)),
            "upload_ms": float(ph.group(1)), "keys_ms": float(ph.group(2)), "columns_ms": float(ph.group(3)), "download_ms": float(ph.group(4)), "compare_all_ms": float(ph.group(5)),
            "keys_mb": float(ph.group(6)), "wall_s": round(wall, 3), "wall_compare_s": round(wall_c, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["rnasim10k", "rnasim100k", "both"])
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--modes", default="tree,subtrees,iterations,no_tree")
    ap.add_argument("--reference", default="truth", choices=["truth", "tree"], help="what every mode is compared with: the true alignment, or the -t output")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--limit", type=int, default=900, help="time limit of each run, seconds")
    a = ap.parse_args()
    import __graft_entry__ as g
    import compare_oracle as CO
    import true_family as TF

    def emit(rec):
        line = json.dumps({**rec, "library_sources": g.source_hash()})
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for name in (["rnasim10k", "rnasim100k"] if a.config == "both" else [a.config]):
        leaves, length = SHAPES[name]
        leaves, length = a.leaves or leaves, a.length or length
        with tempfile.TemporaryDirectory(prefix="twl_compare_bench_") as d:
            t0 = time.perf_counter()
            fam = os.path.join(d, "fam")
            TF.write_family(fam, *TF.make_true_family(leaves, length, seed=1, with_truth=a.reference == "truth"))
            print(f"[compare_bench] family of {leaves} x {length} written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            workload = f"{name}: {leaves} sequences x {length}, type n, family of tools/true_family.py seed 1, reference: " + \
                       ("its true alignment" if a.reference == "truth" else "the output of the -t run")
            ref = os.path.join(fam, "true.aln") if a.reference == "truth" else os.path.join(d, "tree_reference.aln")
            if a.reference == "tree":
                _run([EXE, *mode_args("tree", fam, leaves), "-i", os.path.join(fam, "s.fa"), "-o", ref, "--type", "n"], a.limit)
            for mode in a.modes.split(","):
                out = os.path.join(d, mode + ".aln")
                emit({"workload": workload, **one_mode(mode, fam, leaves, out, a.limit, ref)})
                if mode == "tree" and a.reference == "truth":
                    names, rows = CO.read_alignment(out, limit=1000)
                    _, truth = CO.read_alignment(ref, limit=1000)      # (both files list the leaves in one order)
                    sub = [n for n in names if n in truth]
                    t0 = time.perf_counter()
                    cols = CO.per_column_np([rows[n] for n in sub], [truth[n] for n in sub])
                    emit({"workload": workload, "mode": "tree", "context": f"numpy per-column oracle on the first {len(sub)} rows", "oracle_s": round(time.perf_counter() - t0, 3),
                          "oracle_line": CO.report(cols, len(sub), 0, 0)})
                os.remove(out)


if __name__ == "__main__":
    main()
