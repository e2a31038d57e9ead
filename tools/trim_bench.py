"""--trim-gappy benchmark (reported, not gated): the families of bench.py's configurations rnasim10k (10 000 x 10 kbp) and rnasim100k
(100 000 x 1.6 kbp), aligned with -t on the family's own tree, the same command without the flag and with `--trim-gappy 0.95`, three runs
each, alternated (plain, trimmed, plain, trimmed, ...) so that both see the same machine.  Prints one JSON line per run:

  read_back_ms        the last download of the rows (the run's -v line "Rows back on the host in ... ms"; with the flag it holds the trim)
  write_s             the driver's write phase (its -v line "Driver phases (s)")
  trim_kernels_ms     twl_store_trim_timing as the run's -v line reports it (null without the flag); where: resident rows or an uploaded copy
  width, kept         columns of the alignment before and after the trim
  bytes_written       size of the output file
  command_to_file_s   process start to exit
The counts pass reads N x W row bytes once, the compaction reads them again and writes N x kept: trim_bytes / trim_kernels_ms is set against
the HBM peak as share_of_hbm_peak.

    python tools/trim_bench.py [--config rnasim10k|rnasim100k|both] [--leaves N] [--length L] [--runs 3] [--threshold 0.95] [--out FILE]
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
HBM_PEAK = 8.0e12      # bytes per second, MI355X


def _run(cmd, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return wall, r.stderr


def one_run(tree, fasta, out, threshold, limit):
    flags = ["--trim-gappy", str(threshold)] if threshold is not None else []
    wall, err = _run([EXE, "-t", tree, "-i", fasta, "-o", out, "--type", "n", "-v", *flags], limit)
    back = re.findall(r"Rows back on the host in ([\d.e+-]+) ms", err)
    phases = re.search(r"Driver phases \(s\): tree ([\d.e+-]+), read ([\d.e+-]+), align ([\d.e+-]+), write ([\d.e+-]+)", err)
    trimmed = re.search(r"Trimmed the alignment: (\d+) of (\d+) columns kept", err)
    kern = re.search(r"Trim kernels ([\d.e+-]+) ms on (the resident rows|an uploaded copy of the final rows)", err)
    length = re.search(r"Alignment \(length: (\d+)\)", err)
    if not back or not phases or not length or (threshold is not None and not (trimmed and kern)):
        raise SystemExit("a -v line is missing in the run's output:\n" + err[-3000:])
    rec = {"flag": f"--trim-gappy {threshold}" if threshold is not None else None, "read_back_ms": float(back[-1]), "write_s": float(phases.group(4)),
           "align_s": float(phases.group(3)), "width": int(length.group(1)), "kept": int(trimmed.group(1)) if trimmed else None,
           "trim_kernels_ms": float(kern.group(1)) if kern else None, "where": kern.group(2) if kern else None,
           "bytes_written": os.path.getsize(out), "command_to_file_s": round(wall, 3)}
    os.remove(out)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["rnasim10k", "rnasim100k", "both"])
    ap.add_argument("--leaves", type=int, default=0, help="override the family size (development)")
    ap.add_argument("--length", type=int, default=0, help="override the sequence length (development)")
    ap.add_argument("--runs", type=int, default=3, help="runs of each of the two commands, alternated")
    ap.add_argument("--threshold", type=float, default=0.95)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--limit", type=int, default=900, help="time limit of each run, seconds")
    a = ap.parse_args()
    import bench
    import __graft_entry__ as g

    for name in (["rnasim10k", "rnasim100k"] if a.config == "both" else [a.config]):
        cfg = dict(bench.CONFIGS[name])
        cfg["workload"] = "calibrated"
        if a.leaves:
            cfg["leaves"] = a.leaves
        if a.length:
            cfg["length"] = a.length
        with tempfile.TemporaryDirectory(prefix="twl_trim_bench_") as d:
            t0 = time.perf_counter()
            tree, fasta = bench.write_family(cfg, d)
            print(f"[trim_bench] family of {cfg['leaves']} x {cfg['length']} written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            for k in range(a.runs):
                for threshold in (None, a.threshold):
                    rec = one_run(tree, fasta, os.path.join(d, "out.aln"), threshold, a.limit)
                    n = cfg["leaves"]
                    if rec["trim_kernels_ms"]:
                        rec["trim_bytes"] = {"read": 2 * n * rec["width"], "written": n * rec["kept"]}
                        rec["share_of_hbm_peak"] = (2 * n * rec["width"] + n * rec["kept"]) / (rec["trim_kernels_ms"] / 1e3) / HBM_PEAK
                    rec = {"workload": f"{name}: {n} sequences x {cfg['length']}, type n, -t", "run": k + 1, "of": a.runs, **rec, "library_sources": g.source_hash()}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if a.out:
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "a") as f:
                            f.write(line + "\n")


if __name__ == "__main__":
    main()
