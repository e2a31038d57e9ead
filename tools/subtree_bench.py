"""Subtree-mode benchmark (reported, not gated): the product's command line with -m on the synthetic families of bench.py.  Prints one JSON line.

  rnasim10k    10 000 x 10 kbp at -m 1000
  rnasim100k   100 000 x 1.6 kbp at -m 10000

Per case, from the -v output of `twilight-mi355x -t T -i S -o O -m N -v`: the wall-clock of the run, phase A (the subtrees, one after the
other), the subtree profiles, phase B (the merge along the tree of subtrees: prepare + DP, restore, apply, commit) and the final row
rewrite; per subtree whose profile was summed on the device, the time of twl_store_weighted_columns with the row bytes it read, and from
their totals its bytes per second as a share of the HBM peak; for information, the wall-clock of the same binary without -m (a different
alignment: context, not a yardstick).  There is no threshold: the mode has no earlier time to be held to.

    python tools/subtree_bench.py [--cases rnasim10k,rnasim100k] [--leaves N --length L --max-subtree M] [--keep DIR] [--no-plain]
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
CASES = {"rnasim10k": 1000, "rnasim100k": 10000}
HBM_PEAK_BYTES_PER_S = 8.0e12


def run_cli(args):
    t0 = time.perf_counter()
    r = subprocess.run([EXE] + args, capture_output=True, text=True)
    secs = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("twilight-mi355x failed:\n" + r.stderr[-3000:])
    return secs, r.stderr


def parse_verbose(err):
    out = {}
    m = re.search(r"Aligned (\d+) subtrees \((\d+) rows\) and merged them: subtrees (\d+) pairs, (\d+) band cells; merge (\d+) band cells, (\d+) retried", err)
    out["subtrees"], out["rows"], out["subtree_pairs"], out["band_cells_subtrees"], out["band_cells_merge"], out["merge_retries"] = [int(x) for x in m.groups()]
    m = re.search(r"Subtree phases \(ms\): subtrees ([\d.]+), profiles ([\d.]+) \((\d+) row bytes\), merge ([\d.]+) \(prepare\+DP ([\d.]+), restore ([\d.]+), apply ([\d.]+), "
                  r"commit ([\d.]+)\), finish ([\d.]+), read-back ([\d.]+), write ([\d.]+)", err)
    keys = ("phase_a_ms", "profiles_ms", "profile_row_bytes", "phase_b_ms", "merge_dp_ms", "merge_restore_ms", "merge_apply_ms", "merge_commit_ms", "finish_ms", "read_back_ms", "write_ms")
    out.update({k: (int(v) if k == "profile_row_bytes" else float(v)) for k, v in zip(keys, m.groups())})
    out["width"] = int(re.search(r"Final Alignment Length: (\d+)", err).group(1))
    out["merge_pairs_per_level"] = [int(x) for x in re.findall(r"Subtree merge level \d+: (\d+) pairs? in one", err)]
    groups = [{"subtree": int(k), "rows": int(n), "columns": int(c), "ms": float(ms), "row_bytes": int(b)}
              for k, n, c, ms, b in re.findall(r"Subtree (\d+) profile: weighted columns over (\d+) rows x (\d+) columns \(([\d.]+) ms, (\d+) row bytes read", err)]
    out["weighted_columns"] = groups
    out["cached_profiles"] = len(re.findall(r"profile: cached msaFreq", err))
    ms, nbytes = sum(g["ms"] for g in groups), sum(g["row_bytes"] for g in groups)
    out["weighted_columns_ms"], out["weighted_columns_bytes_per_s"] = round(ms, 3), (nbytes / (ms / 1e3) if ms > 0 else None)
    out["weighted_columns_share_of_hbm_peak"] = (nbytes / (ms / 1e3) / HBM_PEAK_BYTES_PER_S if ms > 0 else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--max-subtree", type=int, default=0, help="override -m (development)")
    ap.add_argument("--keep", default="", help="directory for the generated families (kept)")
    ap.add_argument("--no-plain", action="store_true", help="skip the run without -m")
    a = ap.parse_args()
    import bench

    result = {"cases": {}}
    for name in [c for c in a.cases.split(",") if c]:
        cfg = dict(bench.CONFIGS[name])
        cfg["workload"] = "calibrated"
        if a.leaves:
            cfg["leaves"] = a.leaves
        if a.length:
            cfg["length"] = a.length
        m = a.max_subtree or CASES[name]
        with tempfile.TemporaryDirectory() as tmp:
            d = os.path.join(a.keep, name) if a.keep else tmp
            os.makedirs(d, exist_ok=True)
            tree, fasta = bench.write_family(cfg, d)
            common = ["-t", tree, "-i", fasta, "--type", cfg["type"]]
            secs, err = run_cli(common + ["-o", os.path.join(d, "subtrees.aln"), "-m", str(m), "-v"])
            rec = {"workload": f"{cfg['leaves']} x {cfg['length']} ({cfg['type']}) at -m {m}", "wall_s": round(secs, 3)}
            rec.update(parse_verbose(err))
            if not a.no_plain:
                secs, err = run_cli(common + ["-o", os.path.join(d, "plain.aln")])
                rec["plain_wall_s"] = round(secs, 3)
                rec["plain_width"] = int(re.search(r"\(length (\d+)\)", err).group(1))
            result["cases"][name] = rec
    import twilight_amd as twl

    result["library"] = twl.version()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
