"""Placement benchmark (reported, not gated): N_NEW mutated sequences placed into an N_BB-row backbone (`twilight-mi355x -a`), the backbone
aligned by the product's default mode (-t) from a synthetic family (twilight_amd/synth.py).  Prints one JSON line: the per-phase times of
the placement as its -v report gives them (count, prepare + DP, restore, collect, finish, read-back, write) and the cells/s of its DP launches.

    python tools/place_bench.py [--new 20000] [--backbone 1000] [--length 10000] [--dir DIR]

With --keep-length the same input is placed twice in one session, without the flag and with `--keep-length --write-insertions`, and one JSON
line is printed for each (and appended to --out FILE): per phase the finish (the HIP-event time of the rows kernel with the bytes it reads
and writes and the share of the 8 TB/s HBM peak they amount to), the runs step, the read-back, the write and the wall clock.  The two runs
compute different files: there is no pass/fail number.

    python tools/place_bench.py --keep-length [--out profiles/keep_length/bench.jsonl] [...]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")


def write_inputs(d, n_bb, n_new, length, seed=20261016):
    from twilight_amd import synth

    sys.setrecursionlimit(1000000)
    nwk, leaves = synth.make_family(n_bb, length, seed=seed)
    tree, fasta, new = os.path.join(d, "bb.nwk"), os.path.join(d, "bb.fa"), os.path.join(d, "new.fa")
    open(tree, "w").write(nwk + "\n")
    with open(fasta, "w") as f:
        for name, s in leaves:
            f.write(f">{name}\n{s}\n")
    # the new sequences: leaves of the family mutated once more (substitutions and short indels)
    rng = np.random.default_rng(seed + 1)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = [np.frombuffer(s.encode(), dtype=np.uint8) for _, s in leaves]
    inv = np.zeros(256, dtype=np.int8)
    inv[lut] = np.arange(4, dtype=np.int8)
    with open(new, "wb") as f:
        for k in range(n_new):
            src = inv[codes[int(rng.integers(0, n_bb))]]
            m = synth._mutate(src, rng, 4, 0.01, 0.001, None)
            f.write(b">q%d\n" % k + lut[m].tobytes() + b"\n")
    return tree, fasta, new


def run(cmd, timeout):
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{cmd[0]} exited with {r.returncode}")
    return r, time.perf_counter() - t0


HBM_PEAK = 8.0e12      # bytes/s, the MI355X's specified peak


def keep_line(a, d, bb, new, t_bb, t_inputs):
    """The run with --keep-length --write-insertions: its JSON record."""
    out, ins = os.path.join(d, "kept.aln"), os.path.join(d, "kept_insertions.tsv")
    r, t_place = run([EXE, "-a", bb, "-i", new, "-o", out, "--keep-length", "--write-insertions", ins, "-v"], 1800)
    m = re.search(r"Placement phases \(ms\): count ([\d.]+), prepare\+DP ([\d.]+), restore ([\d.]+), collect ([\d.]+), keep-finish ([\d.]+), runs ([\d.]+), "
                  r"read-back ([\d.]+), write ([\d.]+); DP kernel ([\d.]+) ms, (\d+) band cells; restored on the host \d+; keep kernels: rows ([\d.]+) ms, runs ([\d.]+) ms", r.stderr)
    k = re.search(r"Kept the backbone's length (\d+): (\d+) insertion run\(s\), (\d+) letter\(s\) of (\d+) sequence\(s\) left out \(merged they would make (\d+) columns\)", r.stderr)
    w = re.search(r"Placed (\d+) sequences into (\d+) backbone rows", r.stderr)
    if not m or not k or not w:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("no phase report in the output of the run with --keep-length")
    count, dp, restore, collect, finish, runs, read, write, kern = (float(x) for x in m.groups()[:9])
    rows_ms, runs_ms = float(m.group(11)), float(m.group(12))
    L, n_runs, letters, n_seq, merged = (int(x) for x in k.groups())
    M, B = int(w.group(1)), int(w.group(2))
    total_letters = sum(len(l.strip()) for l in open(new) if not l.startswith(">"))
    # the rows kernel reads every final path (L codes and one per dropped letter) and every sequence, and writes M rows of L columns and two counts each
    read_b, written_b = M * L + letters + total_letters, M * L + 8 * M
    return {
        "workload": f"place {a.new} x {a.length} bp into {a.backbone} rows, --keep-length --write-insertions",
        "backbone_columns": L, "final_columns": L, "merged_columns_would_be": merged, "placed": M, "backbone_rows": B,
        "dropped_runs": n_runs, "dropped_letters": letters, "sequences_with_runs": n_seq,
        "phases_ms": {"count": count, "prepare_dp": dp, "restore": restore, "collect": collect, "keep_finish": finish, "runs": runs, "read_back": read, "write": write},
        "keep_rows_kernel_ms": rows_ms, "keep_runs_kernel_ms": runs_ms,
        "keep_rows_kernel_bytes": {"read": read_b, "written": written_b},
        "keep_rows_kernel_share_of_hbm_peak": (read_b + written_b) / (rows_ms / 1e3) / HBM_PEAK if rows_ms > 0 else None,
        "rows_read_back_bytes": M * L, "output_bytes": os.path.getsize(out), "insertions_bytes": os.path.getsize(ins),
        "dp_kernel_ms": kern, "band_cells": int(m.group(10)),
        "placement_wall_s": round(t_place, 3), "backbone_wall_s": round(t_bb, 3), "inputs_s": round(t_inputs, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=20000)
    ap.add_argument("--backbone", type=int, default=1000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--keep-length", action="store_true", help="place the same input a second time with --keep-length --write-insertions; one JSON line per run")
    ap.add_argument("--out", default=None, help="with --keep-length: a file the two JSON lines are appended to")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="place_bench_")
    os.makedirs(d, exist_ok=True)
    t0 = time.perf_counter()
    tree, fasta, new = write_inputs(d, a.backbone, a.new, a.length)
    t_inputs = time.perf_counter() - t0
    bb = os.path.join(d, "bb.aln")
    _, t_bb = run([EXE, "-t", tree, "-i", fasta, "-o", bb], 1200)
    out = os.path.join(d, "out.aln")
    r, t_place = run([EXE, "-a", bb, "-i", new, "-o", out, "-v"], 1800)
    m = re.search(r"Placement phases \(ms\): count ([\d.]+), prepare\+DP ([\d.]+), restore ([\d.]+), collect ([\d.]+), finish ([\d.]+), "
                  r"read-back ([\d.]+), write ([\d.]+); DP kernel ([\d.]+) ms, (\d+) band cells", r.stderr)
    w = re.search(r"final alignment length (\d+) \(backbone (\d+)\), (\d+) chunk", r.stderr)
    if not m or not w:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("no phase report in the placement's output")
    count, dp, restore, collect, finish, read, write, kern = (float(x) for x in m.groups()[:8])
    cells = int(m.group(9))
    rec = {
        "workload": f"place {a.new} x {a.length} bp into {a.backbone} rows",
        "backbone_columns": int(w.group(2)), "final_columns": int(w.group(1)), "chunks": int(w.group(3)),
        "phases_ms": {"count": count, "prepare_dp": dp, "restore": restore, "collect": collect, "finish": finish, "read_back": read, "write": write},
        "dp_kernel_ms": kern, "band_cells": cells, "dp_cells_per_s": cells / (kern / 1e3) if kern > 0 else None,
        "dp_cells_per_s_incl_prepare": cells / (dp / 1e3) if dp > 0 else None,
        "count_collect_finish_over_dp": (count + collect + finish) / dp if dp > 0 else None,
        "placement_wall_s": round(t_place, 3), "backbone_wall_s": round(t_bb, 3), "inputs_s": round(t_inputs, 3)}
    if a.keep_length:
        B = sum(1 for l in open(bb) if l.startswith(">"))
        rec["rows_read_back_bytes"] = (B + a.new) * int(w.group(1))
        rec["output_bytes"] = os.path.getsize(out)
    lines = [json.dumps(rec)]
    print(lines[0], flush=True)
    if a.keep_length:
        lines.append(json.dumps(keep_line(a, d, bb, new, t_bb, t_inputs)))
        print(lines[1], flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
