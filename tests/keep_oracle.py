"""tests/keep_oracle.py -- CPU restatement of the placement finish that keeps the backbone's length (include/twl_keep.h, `-a --keep-length`).

TEST INFRASTRUCTURE ONLY, plain numpy, no GPU.  Two independent statements of the same result:
  1. keep_row / runs / counts: from (sequence, path, L) directly -- the row of L columns, the dropped runs as (col, qpos, len) records
     and their number and letters;
  2. strip / strip_row / records_of_merged: from the merged output of tests/place_oracle.py (every row at the width W = L + sum(longest))
     by deleting the insertion columns, the columns of the blocks longest[k].
tests/test_keep_oracle_cpu.py proves that the two agree on every directed input."""
from __future__ import annotations

import numpy as np


def keep_row(seq: bytes, path, L: int) -> bytes:
    """The row of L columns: the letter under code 0, '-' under code 2, letters under code 1 left out."""
    out = bytearray()
    q = 0
    for v in path:
        if v == 0:
            out.append(seq[q])
            q += 1
        elif v == 2:
            out.append(ord("-"))
        else:
            q += 1
    assert len(out) == L and q == len(seq), (len(out), L, q, len(seq))
    return bytes(out)


def runs(path):
    """[(col, qpos, len)] of every maximal run of code 1, in path order: col backbone columns in front, qpos index of its first letter."""
    out = []
    c = q = 0
    start = None
    for v in list(path) + [0]:
        if v == 1:
            if start is None:
                start = q
            q += 1
            continue
        if start is not None:
            out.append((c, start, q - start))
            start = None
        if v != 1:
            c += 1
        if v == 0:
            q += 1
    return out


def counts(path):
    """(dropped runs, dropped letters)."""
    r = runs(path)
    return len(r), sum(n for _, _, n in r)


def insertion_lines(name: bytes, seq: bytes, path) -> bytes:
    """The sequence's lines of the --write-insertions file: name<TAB>k<TAB>letters per run."""
    return b"".join(name + b"\t%d\t" % c + seq[q: q + n] + b"\n" for c, q, n in runs(path))


def rebuild(row: bytes, records) -> bytes:
    """The sequence back from its kept row and its records [(col, letters)]: the letters re-inserted in front of backbone column col, gaps dropped."""
    at = {}
    for c, letters in records:
        assert c not in at, "two runs in one slot"
        at[c] = letters
    out = bytearray()
    for c, ch in enumerate(row):
        out += at.get(c, b"")
        if ch != ord("-"):
            out.append(ch)
    out += at.get(len(row), b"")
    return bytes(out)


# ---- the same from the merged output ----

def insertion_mask(longest) -> np.ndarray:
    """bool[W]: True in the columns of the blocks longest[k] (block k lies in front of backbone column k, block L behind the last)."""
    longest = np.asarray(longest, dtype=np.int64)
    L = len(longest) - 1
    mask = np.zeros(L + int(longest.sum()), dtype=bool)
    at = 0
    for k in range(L + 1):
        mask[at: at + longest[k]] = True
        at += int(longest[k]) + 1
    return mask


def strip_row(row: bytes, longest) -> bytes:
    keep = ~insertion_mask(longest)
    assert len(row) == len(keep)
    return np.frombuffer(row, dtype=np.uint8)[keep].tobytes()


def strip(records, longest):
    """records [(name, row)] at the merged width -> the same records with every insertion column deleted."""
    return [(n, strip_row(r, longest)) for n, r in records]


def records_of_merged(row: bytes, longest):
    """[(col, letters)] of a placed row at the merged width: what it holds in the insertion blocks (left-aligned letters, '.' behind them)."""
    out = []
    at = 0
    for k in range(len(longest)):
        letters = row[at: at + int(longest[k])].replace(b".", b"")
        if letters:
            out.append((k, letters))
        at += int(longest[k]) + 1
    return out
