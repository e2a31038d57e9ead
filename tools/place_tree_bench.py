"""Benchmark of placement along a tree (reported, not gated), on the 10 000 x 10 kbp family of bench.py: the backbone is the product's own
alignment of 9 000 of its sequences, the other 1 000 (every tenth) are placed, the tree is the family's.  Prints one JSON line:

  groups, rows, columns_before, columns_after        what the squeeze saw: columns summed over the groups
  read_s, upload_ms, squeeze_kernel_ms,              the phases of the run as its -v lines report them (upload: the store's creation without
  squeeze_call_ms, levels, align_s, write_s          the squeeze call; align: upload, squeeze and all levels)
  squeeze_bytes_read / _written, squeeze_gb_s,       the row bytes the three kernels move, their rate over the HIP-event time and its share of
  squeeze_share_of_hbm_peak                          the MI355X's 8 TB/s
  warm                                               the same three kernels through the binding on synthetic rows (4 000 x 50 000, groups of two, four
                                                     columns of five all-gap), two calls in one process: the first pays the kernels' first launch
                                                     as the CLI's one call does, the second does not
  host_loop_16_threads_s                             for context: the reference's host loop restated (tools/micro/squeeze_host.cpp) on the same rows
  wall_place_s, wall_backbone_s, wall_all_s          wall clock: the placement; the run that made the backbone; -t on all 10 000 (another alignment:
                                                     context, not a target)

Each run is made once, under its own time limit: one run, no repeats.

    python tools/place_tree_bench.py [--leaves N] [--length L] [--every 10] [--out profiles/place_tree/bench.jsonl]
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
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
NUM = r"([\d.e+-]+)"
LINE = (r"Placement-on-tree phases: groups (\d+), rows (\d+), columns (\d+) -> (\d+), squeeze kernels " + NUM + r" ms \(call " + NUM + r" ms, row bytes read (\d+), written (\d+)\), levels (\d+); "
        r"read " + NUM + " ms, align " + NUM + " ms, write " + NUM + " ms")
HBM_PEAK = 8.0e12


def _run(cmd, limit, env=None):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return wall, r


def _split(fasta, every, bb_fa, new_fa):
    n = -1
    with open(fasta) as f, open(bb_fa, "w") as b, open(new_fa, "w") as w:
        out = b
        for line in f:
            if line.startswith(">"):
                n += 1
                out = w if n % every == every - 1 else b
            out.write(line)
    return n + 1


def warm_calls(rows=4000, length=50000):
    """Two calls of twl_store_squeeze_groups in one process, each on half of the rows: HIP-event ms of each and the row bytes each moves."""
    import numpy as np
    import twilight_amd as twl
    from twilight_amd import backbone, level

    twl.init([0])
    rng = np.random.default_rng(1)
    out = []
    block = np.full((rows, length), ord("A"), dtype=np.uint8)
    block[rng.random((rows, length)) < 0.5] = 0x2D
    for k in range(0, rows, 2):
        block[k: k + 2, rng.random(length) < 0.8] = 0x2D
    st = level.Store([block[k].tobytes() for k in range(rows)], "n")
    try:
        for half in (0, 1):
            groups = [[k, k + 1] for k in range(half * rows // 2, (half + 1) * rows // 2, 2)]
            kept = backbone.squeeze_groups(st, groups)
            ms = backbone.squeeze_ms(st)
            moved = 2 * (rows // 2) * length + 2 * sum(kept)
            out.append({"kernel_ms": round(ms, 4), "row_bytes": moved, "gb_s": round(moved / (ms / 1e3) / 1e9, 1), "share_of_hbm_peak": round(moved / (ms / 1e3) / HBM_PEAK, 4)})
    finally:
        st.close()
        twl.shutdown()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--every", type=int, default=10, help="every n-th sequence is new")
    ap.add_argument("--out", default="", help="append the JSON line to this file as well")
    ap.add_argument("--limit", type=int, default=300, help="time limit of each run, seconds")
    a = ap.parse_args()
    import bench
    import __graft_entry__ as g
    import place_tree_oracle as PO

    cfg = dict(bench.CONFIGS["rnasim10k"])
    cfg["workload"] = "calibrated"
    if a.leaves:
        cfg["leaves"] = a.leaves
    if a.length:
        cfg["length"] = a.length
    with tempfile.TemporaryDirectory(prefix="twl_place_tree_bench_") as d:
        tree, fasta = bench.write_family(cfg, d)
        bb_fa, new_fa, bb_aln, out, all_aln = (os.path.join(d, f) for f in ("bb.fa", "new.fa", "bb.aln", "out.aln", "all.aln"))
        total = _split(fasta, a.every, bb_fa, new_fa)
        print(f"[place_tree_bench] family of {total} x {cfg['length']} written", file=sys.stderr, flush=True)
        wall_bb, _ = _run([EXE, "-t", tree, "-i", bb_fa, "-o", bb_aln, "--type", cfg["type"]], a.limit)
        print(f"[place_tree_bench] backbone aligned in {wall_bb:.2f} s", file=sys.stderr, flush=True)
        wall_place, r = _run([EXE, "-t", tree, "-a", bb_aln, "-i", new_fa, "-o", out, "--type", cfg["type"], "--place-on-tree", "-v"], a.limit)
        m = re.search(LINE, r.stderr)
        up = re.search(r"Sequences resident on \d+ device replica\(s\) in " + NUM + " ms", r.stderr)
        if not m or not up:
            raise SystemExit("no phase line in the run's -v output:\n" + r.stderr[-3000:])
        print(f"[place_tree_bench] placement {wall_place:.2f} s", file=sys.stderr, flush=True)
        wall_all, _ = _run([EXE, "-t", tree, "-i", fasta, "-o", all_aln, "--type", cfg["type"]], a.limit)
        # context: the host loop on the same rows and groups, 16 threads
        exe = PO.build_dump(d)
        env = dict(os.environ, TWL_DUMP_NO_ROWS="1")
        _, dr = _run([exe, "-t", tree, "-a", bb_aln, "-i", new_fa, "-o", "x", "--type", cfg["type"], "--place-on-tree"], a.limit, env=env)
        doc = [json.loads(line) for line in dr.stdout.splitlines() if line.startswith("{")][0]
        groups_txt = os.path.join(d, "groups.txt")
        with open(groups_txt, "w") as f:
            for v in doc["groups"].values():
                f.write(" ".join(str(i) for i in v["ids"]) + "\n")
        host = os.path.join(d, "squeeze_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-o", host, os.path.join(ROOT, "tools", "micro", "squeeze_host.cpp")])
        _, hr = _run([host, bb_aln, groups_txt], a.limit, env=dict(os.environ, OMP_NUM_THREADS="16"))
        hm = re.search(r"groups (\d+) threads (\d+) columns (\d+) -> (\d+) seconds " + NUM, hr.stdout)
        kernel_ms, call_ms = float(m.group(5)), float(m.group(6))
        rd, wr = int(m.group(7)), int(m.group(8))
        rate = (rd + wr) / (kernel_ms / 1e3) if kernel_ms > 0 else None
        line = json.dumps({
            "workload": f"place {total // a.every} of {total} x {cfg['length']} along the family's tree into the product's alignment of the other {total - total // a.every}",
            "runs": "one run, no repeats", "groups": int(m.group(1)), "rows": int(m.group(2)), "columns_before": int(m.group(3)), "columns_after": int(m.group(4)),
            "backbone_columns": doc["backbone_len"], "levels": int(m.group(9)),
            "read_s": round(float(m.group(10)) / 1e3, 3), "upload_ms": round(float(up.group(1)) - call_ms, 3), "squeeze_kernel_ms": kernel_ms, "squeeze_call_ms": call_ms,
            "align_s": round(float(m.group(11)) / 1e3, 3), "write_s": round(float(m.group(12)) / 1e3, 3),
            "squeeze_bytes_read": rd, "squeeze_bytes_written": wr, "squeeze_gb_s": round(rate / 1e9, 1) if rate else None,
            "squeeze_share_of_hbm_peak": round(rate / HBM_PEAK, 4) if rate else None,
            "warm": warm_calls(),
            "host_loop_16_threads_s": float(hm.group(5)) if hm else None, "host_loop_same_columns": bool(hm) and (int(hm.group(3)), int(hm.group(4))) == (int(m.group(3)), int(m.group(4))),
            "wall_place_s": round(wall_place, 3), "wall_backbone_s": round(wall_bb, 3), "wall_all_s": round(wall_all, 3), "library_sources": g.source_hash()})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
