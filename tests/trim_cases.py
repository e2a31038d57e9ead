"""tests/trim_cases.py -- directed inputs of twl_store_trim_columns (include/twl_trim.h), each listed with the branch of trim_kernels.hip.h
it is for.  TEST INFRASTRUCTURE.  The shapes sit on the kernels' constants (twl_trim_describe): T columns of a column tile, R rows of a
counts row slice, C columns of a scan round, F rows per flush of the packed byte counters; a thread owns 16 columns, a keep word 32."""
import numpy as np

import trim_oracle as TO

GAP = TO.GAP
LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)


def random_rows(rng, n, W, p_gap=0.4, letters=LETTERS):
    b = rng.choice(letters, size=(n, W))
    b[rng.random((n, W)) < p_gap] = GAP
    return b


def _rows(b):
    return [b[k].tobytes() for k in range(b.shape[0])]


class Case:
    def __init__(self, name, branch, rows, rule, arg):
        self.name, self.branch, self.rows, self.rule, self.arg = name, branch, rows, rule, arg      # arg of TO_ROW: the index of the reference row

    def __repr__(self):
        return self.name


def width_cases(T, C):
    """Three rows, at most one gap kept: every width at which a kernel takes another path."""
    rng = np.random.default_rng(20261021)
    out = []
    for W, branch in ((1, "one column: a thread's 16-byte word mostly behind the row, one keep word of one bit"),
                      (15, "one below a thread's 16 columns"), (16, "a thread's 16 columns"), (17, "one above: a second thread with one column"),
                      (31, "one below a keep word"), (32, "a keep word"), (33, "one above a keep word: the ballot's second half writes one bit"),
                      (63, "one below a wave's two keep words"), (65, "one above"),
                      (T - 1, "one below a column tile"), (T, "a column tile"), (T + 1, "one above: a second tile of one column"),
                      (C - 1, "one below a scan round"), (C, "a scan round"), (C + 1, "one above: a second round with one word")):
        out.append(Case(f"W={W}", branch, _rows(random_rows(rng, 3, W)), TO.MAX_GAPS, 1))
    return out


def row_count_cases(R, F):
    """37 columns; column 5 is '-' in every row (a packed byte counter would wrap at 256 without its flush), column 6 in every row but the last."""
    rng = np.random.default_rng(20261022)
    out = []
    for n, branch in ((1, "one row: the row loop's single-row tail only"), (3, "three rows: no group of four"), (4, "one group of four"), (5, "a group of four and a tail"),
                      (F - 1, "one below a flush period"), (F, "a flush period"), (F + 1, "one above: a second flush with one row"),
                      (R - 1, "one below a row slice"), (R, "a row slice"), (R + 1, "one above: a second workgroup with one row, atomics from two slices")):
        b = random_rows(rng, n, 37, p_gap=0.5)
        b[:, 5] = GAP
        b[:, 6] = GAP
        b[n - 1, 6] = ord("A")
        out.append(Case(f"n={n}", branch, _rows(b), TO.MAX_GAPS, n - 1))
    return out


def content_cases(T, C):
    rng = np.random.default_rng(20261023)
    out = []
    # nine rows, 70 columns, column c with c % 10 gaps: the limit between two columns
    b = rng.choice(LETTERS, size=(9, 70))
    for c in range(70):
        b[: c % 10, c] = GAP
    rows = _rows(b)
    out.append(Case("limit 4 between columns of 4 and 5 gaps", "gaps[c] <= arg: a column with exactly max_gaps gaps beside one with max_gaps + 1", rows, TO.MAX_GAPS, 4))
    out.append(Case("max_gaps = 0", "only gap-free columns", rows, TO.MAX_GAPS, 0))
    out.append(Case("max_gaps = n", "every column, all-gap ones too: kept == W", rows, TO.MAX_GAPS, 9))
    b2 = b.copy()
    b2[0, :] = GAP
    out.append(Case("kept = 0", "no column without a gap: every tile of the compaction ends at once", _rows(b2), TO.MAX_GAPS, 0))
    out.append(Case("kept = W, no gap at all", "nothing to count, every byte moves", _rows(rng.choice(LETTERS, size=(4, T + 40))), TO.MAX_GAPS, 0))
    # kept runs that start and end inside a 32-column word, across words, threads, a tile edge
    W = T + 100
    b = np.full((3, W), GAP, dtype=np.uint8)
    b[1:, :] = rng.choice(LETTERS, size=(2, W))
    for lo, hi in ((5, 9), (14, 18), (30, 34), (37, 61), (70, 71), (95, 97), (T - 3, T + 3), (W - 1, W)):
        b[0, lo:hi] = ord("C")
    out.append(Case("kept runs inside words", "runs that start and end inside a 32-column word, across two threads' 16 columns, two words and a tile edge; the last column kept",
                    _rows(b), TO.MAX_GAPS, 0))
    # three scan rounds, the only kept column in the last word
    W = 2 * C + 40
    b = random_rows(rng, 2, W, p_gap=0.3)
    b[0, :] = GAP
    b[:, W - 2] = ord("G")
    out.append(Case("three scan rounds, one kept column in the last word", "the scan's carry over rounds that keep nothing; compaction tiles without a kept byte", _rows(b), TO.MAX_GAPS, 0))
    b = random_rows(rng, 3, W, p_gap=0.5)
    out.append(Case("three scan rounds, random", "the scan's carry over three rounds", _rows(b), TO.MAX_GAPS, 1))
    # '.', lower case, bytes >= 0x80
    b = rng.choice(np.frombuffer(b"acgtn.", dtype=np.uint8), size=(5, 200))
    b[:, 3::7] = ord(".")
    b[:, 4::7] = GAP
    b[2, 0] = 0xAD                                   # ('-' with its top bit set is a letter)
    out.append(Case("'.' and lower case", "only 0x2D counts; columns of '.' stay; bytes are not folded", _rows(b), TO.MAX_GAPS, 0))
    b = rng.integers(0x80, 0x100, size=(4, 90)).astype(np.uint8)
    b[1, 1::3] = GAP
    out.append(Case("bytes >= 0x80", "the zero-byte test of the packed counters with top bits set", _rows(b), TO.MAX_GAPS, 0))
    # rule 1: the reference row first and last
    b = random_rows(rng, 6, T + 77, p_gap=0.6)
    out.append(Case("to the first row", "TWL_TRIM_TO_ROW, the reference row first in ids", _rows(b), TO.TO_ROW, 0))
    out.append(Case("to the last row", "TWL_TRIM_TO_ROW, the reference row last in ids", _rows(b), TO.TO_ROW, 5))
    b3 = b.copy()
    b3[2, :] = GAP
    out.append(Case("to an all-gap row", "TWL_TRIM_TO_ROW with kept == 0", _rows(b3), TO.TO_ROW, 2))
    return out


def all_cases(T, R, C, F):
    return width_cases(T, C) + row_count_cases(R, F) + content_cases(T, C)
