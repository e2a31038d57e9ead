"""The guide tree rebuilt from an alignment (--iterations), restated in numpy from its definition: the column mask, the
letters, the pair counts, the distances; the tree and its text go through guide_oracle.upgma_newick (section 4f).  Independent of the C++:
tests compare the library, the host code and the command line with it."""
import math

import numpy as np

import guide_oracle

_LETTERS = {"n": ["A", "C", "G", "TU"], "p": list("ACDEFGHIKLMNPQRSTVWY")}


def letter_table(type_):
    """256 entries: the letter's code, -1 for a byte that is no letter; either case."""
    t = np.full(256, -1, dtype=np.int64)
    for v, letters in enumerate(_LETTERS[type_]):
        for ch in letters:
            t[ord(ch)] = v
            t[ord(ch.lower())] = v
    return t


def matrix(rows):
    """uint8 [n][width] of rows given as bytes, all of one width >= 1."""
    a = np.stack([np.frombuffer(bytes(r), dtype=np.uint8) for r in rows])
    assert a.ndim == 2 and a.shape[1] >= 1
    return a


def column_gaps(rows):
    """gaps[c]: rows whose byte at column c is '-'."""
    return (matrix(rows) == ord("-")).sum(axis=0).astype(np.uint32)


def max_gaps(T, n):
    return math.floor(float(T) * n)


def kept_columns(rows, mg):
    return column_gaps(rows) <= mg


def pair_counts(rows, type_, mg):
    """(match, both, kept): uint32 [n][n] each over the kept columns, and their number."""
    a = matrix(rows)
    keep = kept_columns(rows, mg)
    code = letter_table(type_)[a][:, keep]
    n = len(a)
    match = np.zeros((n, n), dtype=np.int64)
    both = np.zeros((n, n), dtype=np.int64)
    valid = code >= 0
    for i in range(n):
        b = valid[i][None, :] & valid
        both[i] = b.sum(axis=1)
        match[i] = (b & (code == code[i][None, :])).sum(axis=1)
    return match.astype(np.uint32), both.astype(np.uint32), int(keep.sum())


def distances(match, both):
    """d = 1 - match / both in double, 1 where both is 0, 0 on the diagonal."""
    m, b = match.astype(np.float64), both.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(both == 0, 1.0, 1.0 - m / b)
    np.fill_diagonal(d, 0.0)
    return d


def tree_of(names, rows, type_, T=0.95):
    match, both, _ = pair_counts(rows, type_, max_gaps(T, len(rows)))
    return guide_oracle.upgma_newick(names, distances(match, both))
