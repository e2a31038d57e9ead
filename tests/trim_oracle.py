"""tests/trim_oracle.py -- CPU restatement of the column trim of finished rows (include/twl_trim.h; `--trim-gappy`, `--trim-to`, `--write-columns`).
TEST INFRASTRUCTURE.

Stated twice and held to itself (agree): once on a 2-D byte array with boolean indexing, once row by row on Python bytes.  Only the byte
0x2D ('-') is a gap; '.' is not; every other byte is kept as it is.
"""
import math

import numpy as np

GAP = 0x2D
MAX_GAPS, TO_ROW = 0, 1


def block(rows):
    """n rows of one length as an (n, W) uint8 array."""
    W = len(rows[0]) if rows else 0
    assert all(len(r) == W for r in rows), "rows of one length"
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), W)


def gap_counts(rows):
    return (block(rows) == GAP).sum(axis=0).astype(np.uint32)


def max_gaps(T, n):
    """floor(T * N), the product taken in double (retree_max_gaps of twl_retree_plan.inc.hip)."""
    return int(math.floor(float(T) * float(n)))


def keep_mask(rows, rule, arg):
    """rule MAX_GAPS: arg = the gap limit; rule TO_ROW: arg = the index in rows of the reference row."""
    if rule == MAX_GAPS:
        return gap_counts(rows) <= arg
    assert rule == TO_ROW
    return block(rows)[arg] != GAP


def trimmed_rows(rows, mask):
    b = block(rows)[:, mask]
    return [b[k].tobytes() for k in range(len(rows))]


def kept_columns(mask):
    return np.flatnonzero(mask).astype(np.int32)


def column_text(rows, mask):
    """The --write-columns file: new<TAB>old<TAB>gaps per kept column."""
    g = gap_counts(rows)
    return "".join(f"{new}\t{old}\t{int(g[old])}\n" for new, old in enumerate(kept_columns(mask)))


# ---- the same, row by row on bytes ----
def gap_counts_by_rows(rows):
    W = len(rows[0]) if rows else 0
    return [sum(1 for r in rows if r[c] == GAP) for c in range(W)]


def keep_list_by_rows(rows, rule, arg):
    if rule == MAX_GAPS:
        return [g <= arg for g in gap_counts_by_rows(rows)]
    return [b != GAP for b in rows[arg]]


def trimmed_rows_by_rows(rows, keep):
    return [bytes(b for b, k in zip(r, keep) if k) for r in rows]


def agree(rows, rule, arg):
    """Both statements on one input; returns (mask, trimmed rows)."""
    mask = keep_mask(rows, rule, arg)
    keep = keep_list_by_rows(rows, rule, arg)
    assert list(mask) == keep
    assert list(gap_counts(rows)) == gap_counts_by_rows(rows)
    out = trimmed_rows(rows, mask)
    assert out == trimmed_rows_by_rows(rows, keep)
    assert all(len(r) == int(mask.sum()) for r in out)
    return mask, out


# ---- FASTA as the tool writes it: one line per row ----
def read_fasta(path):
    names, rows = [], []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\n")
            if line.startswith(b">"):
                names.append(line[1:].decode())
                rows.append(b"")
            elif names:
                rows[-1] += line
    return names, rows
