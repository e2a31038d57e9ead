"""Merge benchmark (reported, not gated): FILES alignments of ROWS rows x COLS columns merged as a star, the paths given (no DP: what is
timed is what the merge mode adds to the level API).  Prints one JSON line.

  (a) maps     twl_merge_apply per merge + twl_merge_finish: the column maps composed per merge, every row rewritten once
               (HIP-event time of their kernels, twl_merge_timing)
  (b) commits  the same merges done the only way the level API alone allows: every row listed as a member of its side and rewritten
               by twl_level_commit at every merge (HIP-event time of the commits' kernels, twl_level_timing)
  copy         a device-to-device copy that moves as many bytes as the row rewrite of (a) reads and writes (rows * (COLS + W)), in
               the same process (torch's copy_, timed with its events)

Both ways run once at a small size first (code objects loaded; their final rows are compared there), then REPEATS times each at the full
size, alternating, each on a store of its own; the medians are reported.  The rows' letters do not matter to any kernel timed here: every
file repeats one random row.

    python tools/merge_bench.py [--files 32] [--rows 2000] [--cols 10000] [--match 0.98] [--repeats 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_case(files, rows, cols, match, seed=20261017):
    """(rows of every file, merge steps [(groups under the root, child, path)], final width): a star rooted at file 0, the last child first."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT-", dtype=np.uint8)
    data = [[letters[rng.integers(0, 5, cols)].tobytes()] * rows for _ in range(files)]
    steps, under, w = [], [0], cols
    for ch in range(files - 1, 0, -1):
        n0 = int(cols * match)
        p = np.array([0] * n0 + [1] * (cols - n0) + [2] * (w - n0), dtype=np.int8)
        rng.shuffle(p)
        steps.append((list(under), ch, p))
        under.append(ch)
        w = len(p)
    return data, steps, w


def run_maps(level, merge, data, steps):
    ids, at = [], 0
    for f in data:
        ids.append(list(range(at, at + len(f))))
        at += len(f)
    st = level.Store([r for f in data for r in f], "n")
    mg = merge.Merge(st, ids)
    for under, ch, p in steps:
        mg.apply_host([under], [[ch]], [p])
    W = mg.finish()
    apply_ms, finish_ms, rewrite_ms = mg.timing()
    return st, mg, W, apply_ms, finish_ms, rewrite_ms


def run_commits(twl, level, data, steps):
    from twilight_amd import synth

    ids, at = [], 0
    for f in data:
        ids.append(list(range(at, at + len(f))))
        at += len(f)
    st = level.Store([r for f in data for r in f], "n")
    prm = twl.make_params(synth.nucleotide_matrix())
    lib = level._lib()
    total, w = 0.0, len(data[0][0])
    for under, ch, p in steps:
        ref = [q for g in under for q in ids[g]]
        qry = ids[ch]
        st.prepare(prm, [[level.Side(ref, [1.0] * len(ref), w, len(ref), float(len(ref))),
                          level.Side(qry, [1.0] * len(qry), len(data[ch][0]), len(qry), float(len(qry)))]], seq_len=max(w, len(data[ch][0])))
        st.commit([p])
        pm, cm = C.c_double(0), C.c_double(0)
        level.api._check(lib.twl_level_timing(st._h, C.byref(pm), C.byref(cm)))
        total += cm.value
        w = len(p)
    return st, w, total


def copy_ms(n_bytes, repeats):
    import torch

    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda").fill_(45)
    dst = torch.empty_like(src)
    out = []
    for k in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--cols", type=int, default=10000)
    ap.add_argument("--match", type=float, default=0.98)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import twilight_amd as twl
    from twilight_amd import level, merge

    twl.init([0])
    # small first: code objects loaded, and the two ways must end in the same rows
    data, steps, W = make_case(4, 40, 1500, a.match, seed=1)
    st, mg, w1, *_ = run_maps(level, merge, data, steps)
    st2, w2, _ = run_commits(twl, level, data, steps)
    assert w1 == w2 == W and st.rows() == st2.rows(), "the two ways disagree"
    mg.close(); st.close(); st2.close()

    data, steps, W = make_case(a.files, a.rows, a.cols, a.match)
    S = a.files * a.rows
    maps, rewrites, applies, commits = [], [], [], []
    for _ in range(a.repeats):
        st, mg, w1, apply_ms, finish_ms, rewrite_ms = run_maps(level, merge, data, steps)
        assert w1 == W
        maps.append(apply_ms + finish_ms); applies.append(apply_ms); rewrites.append(rewrite_ms)
        mg.close(); st.close()
        st, w2, commit_ms = run_commits(twl, level, data, steps)
        assert w2 == W
        commits.append(commit_ms)
        st.close()
    moved = S * (a.cols + W)
    t_copy = copy_ms(moved // 2, a.repeats)
    t_rw = statistics.median(rewrites)
    print(json.dumps({
        "workload": f"merge {a.files} files x {a.rows} rows x {a.cols} columns, {a.files - 1} merges, final width {W}",
        "repeats": a.repeats,
        "maps_ms": round(statistics.median(maps), 3), "maps_ms_all": [round(x, 3) for x in maps],
        "maps_apply_ms": round(statistics.median(applies), 3), "rewrite_ms": round(t_rw, 3),
        "commits_ms": round(statistics.median(commits), 3), "commits_ms_all": [round(x, 3) for x in commits],
        "commits_over_maps": round(statistics.median(commits) / statistics.median(maps), 2),
        "rewrite_bytes": moved, "rewrite_bytes_per_s": moved / (t_rw / 1e3) if t_rw > 0 else None,
        "copy_ms": round(t_copy, 3), "copy_bytes_per_s": moved / (t_copy / 1e3) if t_copy > 0 else None,
        "rewrite_over_copy": round(t_rw / t_copy, 2) if t_copy > 0 else None,
        "library": twl.version()}))
    twl.shutdown()


if __name__ == "__main__":
    main()
