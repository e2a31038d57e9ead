#!/usr/bin/env python3
"""A synthetic nucleotide family WITH its true alignment.

make_true_family evolves a root sequence down a random binary tree by the model of twilight_amd.synth.make_family (substitutions with transitions
twice as likely as each transversion, indel events of geometric length with mean 3, Yule-like splits, per-branch rates sub x U(0.5, 1.5)), but
every site carries an id: a substitution keeps the id, a deletion drops it, an insertion makes new ones.  Two letters are homologous iff they
carry one id, so the leaves come with the alignment that is true by construction.  The ids are kept in one linked order: new ids go right behind
the id that precedes them in the sequence they are inserted into, which is consistent with the order of every sequence that ever holds them.

It does not reproduce make_family's sequences for a seed (the random numbers are drawn in another order); it is deterministic for its own seed.

  python tools/true_family.py OUTDIR [--leaves 200] [--length 1000] [--seed 1] [--sub 0.015] [--indel 0.001]     writes t.nwk, s.fa, true.aln
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ALPHABET = np.frombuffer(b"ACGT", dtype=np.uint8)


class _Order:
    """The linked order of all site ids; id 0 is the head in front of every site."""

    def __init__(self, n_root: int):
        self.next = list(range(1, n_root + 1)) + [-1]          # 0 -> 1 -> ... -> n_root -> end

    def insert_after(self, pred: int, count: int) -> np.ndarray:
        first = len(self.next)
        self.next.extend(range(first + 1, first + count))
        self.next.append(self.next[pred])
        self.next[pred] = first
        return np.arange(first, first + count, dtype=np.int64)

    def ranks(self) -> np.ndarray:
        rank = np.full(len(self.next), -1, dtype=np.int64)
        at, r = self.next[0], 0
        while at != -1:
            rank[at] = r
            r += 1
            at = self.next[at]
        return rank


def _mutate(seq, ids, rng, sub, indel, order):
    s = seq.copy()
    hit = rng.random(s.size) < sub
    r = rng.random(s.size)
    new = np.where(r < 0.5, (s + 2) % 4, np.where(r < 0.75, (s + 1) % 4, (s + 3) % 4))
    s = np.where(hit, new, s).astype(np.int8)
    if indel <= 0:
        return s, ids
    out_s, out_i = [], []
    pos = 0
    for e in np.flatnonzero(rng.random(s.size) < indel):
        if e < pos:
            continue
        out_s.append(s[pos:e]); out_i.append(ids[pos:e])
        length = int(rng.geometric(1.0 / 3.0))
        if rng.random() < 0.5:                                  # deletion
            pos = min(s.size, e + length)
        else:                                                   # insertion in front of site e: behind the site that precedes it here
            pred = 0
            for part in reversed(out_i):
                if part.size:
                    pred = int(part[-1])
                    break
            out_s.append(rng.integers(0, 4, size=length).astype(np.int8)); out_i.append(order.insert_after(pred, length))
            pos = e
    out_s.append(s[pos:]); out_i.append(ids[pos:])
    return np.concatenate(out_s), np.concatenate(out_i)


def make_true_family(n_leaves: int, length: int, *, seed: int = 1, sub: float = 0.015, indel: float = 0.001, with_truth: bool = True):
    """(newick, [(name, sequence)], [(name, aligned row)]): leaves s0 .. s{n-1} in file order; the rows all have one width, no column is all gaps,
    and a row without its gaps is the leaf's sequence.  The truth has a column for every inserted site of every branch, so its width grows with the
    number of leaves (10 000 x 10 kbp: 307 896 columns; 100 000 x 1.6 kbp: several hundred thousand, tens of GB of rows): with_truth = False
    returns no rows."""
    rng = np.random.default_rng(seed)
    order = _Order(length)
    root = rng.integers(0, 4, size=length).astype(np.int8)
    leaves = []
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n_leaves + 1000))

    def grow(seq, ids, n):
        if n == 1:
            name = f"s{len(leaves)}"
            leaves.append((name, seq, ids))
            return name
        left = int(rng.integers(1, n))
        parts = []
        for k in (left, n - left):
            b = float(rng.uniform(0.5, 1.5) * sub)
            s2, i2 = _mutate(seq, ids, rng, b, indel, order)
            parts.append(f"{grow(s2, i2, k)}:{b:.6f}")
        return "(" + ",".join(parts) + ")"

    newick = grow(root, np.arange(1, length + 1, dtype=np.int64), n_leaves) + ";"
    if not with_truth:
        return newick, [(name, ALPHABET[seq].tobytes().decode()) for name, seq, _ in leaves], []
    rank = order.ranks()
    used = np.zeros(len(rank), dtype=bool)
    for _, _, ids in leaves:
        used[rank[ids]] = True
    col = np.cumsum(used) - 1                                   # the column of every rank that some leaf holds
    W = int(used.sum())
    seqs, rows = [], []
    for name, seq, ids in leaves:
        letters = ALPHABET[seq]
        row = np.full(W, 0x2D, dtype=np.uint8)
        row[col[rank[ids]]] = letters
        seqs.append((name, letters.tobytes().decode()))
        rows.append((name, row.tobytes().decode()))
    return newick, seqs, rows


def write_family(outdir: str, newick, seqs, rows) -> None:
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "t.nwk"), "w") as f:
        f.write(newick + "\n")
    for path, recs in (("s.fa", seqs), ("true.aln", rows)):
        if not recs:
            continue
        with open(os.path.join(outdir, path), "w") as f:
            for name, s in recs:
                f.write(f">{name}\n{s}\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("outdir")
    ap.add_argument("--leaves", type=int, default=200)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sub", type=float, default=0.015)
    ap.add_argument("--indel", type=float, default=0.001)
    a = ap.parse_args()
    nwk, seqs, rows = make_true_family(a.leaves, a.length, seed=a.seed, sub=a.sub, indel=a.indel)
    write_family(a.outdir, nwk, seqs, rows)
    print(f"{len(seqs)} leaves, true alignment of {len(rows[0][1])} columns -> {a.outdir}")
