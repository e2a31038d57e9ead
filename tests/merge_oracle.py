"""tests/merge_oracle.py -- CPU restatement of the merge of existing alignments (the reference's MERGE_MSA mode, `twilight -f DIR -o OUT`).

TEST INFRASTRUCTURE ONLY.  Built from oracle/level_oracle.py (profile_from_cache, prepare_side, add_gappy_columns_back, update_frequency)
and the DP checker (tests/oracle_lib.py: talco_oracle.c), following what the reference does in that mode:
  1. files: every regular file under the directory, recursively, sorted by path (readAlignments_and_buildTree, io.cpp:246-261)
  2. per file a node: profile = counts of letterIdx(type, toupper(c)) per column over its rows, alnNum = rows, alnWeight = float(rows)
     (readAlignment, io.cpp:200-238), and a column map that starts as the identity (subtreeAln, io.cpp:270)
  3. a star: nodes sorted by row count, descending (stable here; the reference's std::sort leaves ties open), the first one the root,
     the others its children in that order (io.cpp:279-290)
  4. schedule, mode 1 (progressive.cpp:81-95): collectPostOrder (node.cpp:58-71) pushes the root, then the children first to last, so the
     stack's top is the LAST child; every node popped is paired with its parent at the next level: the last child is merged first, then
     the one before it, ... one pair per level, the root always the reference side
  5. per pair (alignment-cpu.cpp:50-175, currentTask 2): both profiles = msaFreq / alnWeight * alnNum, gappy columns removed at -r, PSGP,
     gapCharScore 0, a failed DP retried until errorType 0 (1: xdrop doubles; 2: the band limit grows), gappy columns back
  6. updateFrequency (alignment-helper.cpp:506-539) with the two alnWeights; updateAlignment's subtreeAln branch (:402-423, :449-470): the
     map of every file under the reference side goes through the path's codes != 1, the query's through the codes != 2; then
     alnNum, alnWeight add up and alnLen = the path's length (:474-476)
  7. output (io.cpp:355-449): every row of every file through its file's map, '-' in the other columns; files in sorted order, rows in
     file order

The reference keeps a map as a code string of the merged width (0 where the file has a column); here it is kept as the int array of the
columns the file's own columns sit in -- the same thing, and what include/twl_merge.h keeps on the device.  The three numpy functions
below (path_ranks, compose, expand_rows) are what tests hold merge_kernels.hip.h to, byte for byte.
"""
from __future__ import annotations

import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import level_oracle as LO  # noqa: E402
import oracle_lib as O  # noqa: E402
import place_oracle as PO  # noqa: E402

F = np.float32


# ---- the numpy versions of the device kernels ----

def path_ranks(path):
    """(rpos, qpos): rpos[r] = position of the r-th code != 1, qpos[q] = position of the q-th code != 2."""
    p = np.asarray(path, dtype=np.int8)
    return np.flatnonzero(p != 1).astype(np.int32), np.flatnonzero(p != 2).astype(np.int32)


def compose(pos, table):
    """pos[c] = table[pos[c]]."""
    return np.asarray(table, dtype=np.int32)[np.asarray(pos, dtype=np.int64)]


def expand_rows(rows, pos, W):
    """out[pos[c]] = row[c], '-' elsewhere, for every row of a group."""
    out = []
    idx = np.asarray(pos, dtype=np.int64)
    for r in rows:
        o = np.full(W, ord("-"), dtype=np.uint8)
        o[idx] = np.frombuffer(r, dtype=np.uint8)
        out.append(o.tobytes())
    return out


def path_ok(path, wr, wq):
    p = np.asarray(path, dtype=np.int8)
    return bool(np.all((p >= 0) & (p <= 2)) and np.count_nonzero(p != 1) == wr and np.count_nonzero(p != 2) == wq)


class Maps:
    """The maps of a merge, as include/twl_merge.h keeps them: apply() per level, rows() at the end."""

    def __init__(self, lengths):
        self.pos = [np.arange(L, dtype=np.int32) for L in lengths]
        self.width = list(lengths)

    def apply(self, ref_groups, qry_groups, paths):
        for rg, qg, p in zip(ref_groups, qry_groups, paths):
            if len(p) == 0:
                continue
            assert path_ok(p, self.width[rg[0]], self.width[qg[0]])
            rpos, qpos = path_ranks(p)
            for g in rg:
                self.pos[g] = compose(self.pos[g], rpos)
            for g in qg:
                self.pos[g] = compose(self.pos[g], qpos)
            for g in list(rg) + list(qg):
                self.width[g] = len(p)

    def rows(self, groups_rows):
        W = self.width[0]
        assert all(w == W for w in self.width)
        return [expand_rows(rows, pos, W) for rows, pos in zip(groups_rows, self.pos)], W


# ---- the mode ----

def list_files(directory):
    out = []
    for base, _, names in os.walk(directory):
        out += [os.path.join(base, n) for n in names if os.path.isfile(os.path.join(base, n))]
    return sorted(out)


def schedule(row_counts):
    """(root, children in the order they are merged): items 3 and 4."""
    order = sorted(range(len(row_counts)), key=lambda k: -row_counts[k])      # (sorted() is stable)
    return order[0], order[1:][::-1]


def merge_pair(fr, num_r, w_r, fq, num_q, w_q, seq_type, matrix, *, gap_open=-50.0, gap_extend=-5.0, thr=0.95, log=None):
    """Item 5: the final path of one pair of cached profiles."""
    P = fr.shape[1]
    rp = LO.profile_from_cache(fr, w_r, num_r)
    qp = LO.profile_from_cache(fq, w_q, num_q)
    cr, ir, runs_r = LO.prepare_side(rp, num_r, thr, gap_open, gap_extend, seq_type)
    cq, iq, runs_q = LO.prepare_side(qp, num_q, thr, gap_open, gap_extend, seq_type)
    prm = O.make_params(matrix, gap_open=gap_open, gap_extend=gap_extend, gap_char=0.0)
    min_len = min(cr.shape[0], cq.shape[0])
    while True:
        path, err, _ = O.align_pair(prm, cr[:, :P], cq[:, :P], cr[:, P], cr[:, P + 1], cq[:, P], cq[:, P + 1], num_r, num_q)
        if err == 0:
            break
        assert err != 3, "errorType 3"
        if err == 2:
            prm.flen = min(int(prm.flen * 1.2) << 1, min_len)
        else:
            prm.xdrop = int(prm.xdrop * 2)
            prm.flen = min(int(prm.xdrop * 4) << 1, min_len)
        if log is not None:
            log(prm.xdrop, prm.flen)
    return LO.add_gappy_columns_back(path, runs_r if thr != 1.0 else [], runs_q if thr != 1.0 else [], (ir & 0x7F).astype(np.int64),
                                     (iq & 0x7F).astype(np.int64), matrix, gap_open, gap_extend)


def merge(files, seq_type="n", *, matrix=None, gap_open=-50.0, gap_extend=-5.0, thr=0.95, log=None):
    """files: [[(name, row), ...], ...] in sorted file order.  Returns (records [(name, row)], W, maps, paths in merge order)."""
    from twilight_amd import synth

    if matrix is None:
        matrix = synth.nucleotide_matrix() if seq_type == "n" else synth.protein_matrix()
    for recs in files:
        assert recs and all(len(r) == len(recs[0][1]) for _, r in recs), "rows of unequal length"
    rows = [[r for _, r in recs] for recs in files]
    if len(files) == 1:
        return list(files[0]), len(rows[0][0]), Maps([len(rows[0][0])]), []
    freq = [PO.backbone_profile(r, seq_type) for r in rows]
    root, children = schedule([len(r) for r in rows])
    maps = Maps([len(r[0]) for r in rows])
    num, weight, under, paths = len(rows[root]), F(len(rows[root])), [root], []
    for ch in children:
        qn, qw = len(rows[ch]), F(len(rows[ch]))
        path = merge_pair(freq[root], num, weight, freq[ch], qn, qw, seq_type, matrix, gap_open=gap_open, gap_extend=gap_extend, thr=thr, log=log)
        freq[root] = LO.update_frequency(freq[root], freq[ch], path, weight, qw)
        maps.apply([under], [[ch]], [path])
        num, weight = num + qn, F(weight + qw)
        under.append(ch)
        paths.append(path)
    out_rows, W = maps.rows(rows)
    records = [(n, r) for recs, rr in zip(files, out_rows) for (n, _), r in zip(recs, rr)]
    return records, W, maps, paths


def merge_dir(directory, seq_type="n", **kw):
    return merge([PO.read_fasta(f) for f in list_files(directory)], seq_type, **kw)


to_bytes = PO.to_bytes
