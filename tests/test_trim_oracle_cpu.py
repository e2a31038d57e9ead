"""The trim's CPU restatement (tests/trim_oracle.py) against tiny alignments trimmed by hand, its two statements against each other on the
directed cases (tests/trim_cases.py), and floor(T * N) where the product lies next to an integer.  No GPU needed."""
import math
from fractions import Fraction

import numpy as np
import pytest

import trim_cases as TC
import trim_oracle as TO

# 4 x 8, by hand.  gaps per column: 0 1 1 2 4 0 1 2 (the '.' of column 6 is no gap)
HAND = [b"AC-T-G.A",
        b"ACG--Gc-",
        b"A-G--G-A",
        b"ACGT-GT-"]
HAND_GAPS = [0, 1, 1, 2, 4, 0, 1, 2]


def test_gap_counts_by_hand():
    assert TO.gap_counts(HAND).tolist() == HAND_GAPS
    assert TO.gap_counts_by_rows(HAND) == HAND_GAPS


@pytest.mark.parametrize("limit, cols, rows", [
    (0, [0, 5], [b"AG", b"AG", b"AG", b"AG"]),
    (1, [0, 1, 2, 5, 6], [b"AC-G.", b"ACGGc", b"A-GG-", b"ACGGT"]),
    (2, [0, 1, 2, 3, 5, 6, 7], [b"AC-TG.A", b"ACG-Gc-", b"A-G-G-A", b"ACGTGT-"]),
    (3, [0, 1, 2, 3, 5, 6, 7], [b"AC-TG.A", b"ACG-Gc-", b"A-G-G-A", b"ACGTGT-"]),
    (4, list(range(8)), HAND),
])
def test_max_gaps_by_hand(limit, cols, rows):
    mask, out = TO.agree(HAND, TO.MAX_GAPS, limit)
    assert TO.kept_columns(mask).tolist() == cols
    assert out == rows


@pytest.mark.parametrize("ref, cols, rows", [
    (0, [0, 1, 3, 5, 6, 7], [b"ACTG.A", b"AC-Gc-", b"A--G-A", b"ACTGT-"]),      # '.' is not a gap: column 6 stays
    (2, [0, 2, 5, 7], [b"A-GA", b"AGG-", b"AGGA", b"AGG-"]),
])
def test_to_row_by_hand(ref, cols, rows):
    mask, out = TO.agree(HAND, TO.TO_ROW, ref)
    assert TO.kept_columns(mask).tolist() == cols
    assert out == rows
    assert GAPLESS(out[ref]) and out[ref] == HAND[ref].replace(b"-", b"")


def GAPLESS(row):
    return b"-" not in row


def test_column_text_by_hand():
    mask = TO.keep_mask(HAND, TO.MAX_GAPS, 1)
    assert TO.column_text(HAND, mask) == "0\t0\t0\n1\t1\t1\n2\t2\t1\n3\t5\t0\n4\t6\t1\n"
    assert TO.column_text(HAND, TO.keep_mask(HAND, TO.MAX_GAPS, 0)) == "0\t0\t0\n1\t5\t0\n"
    assert TO.column_text([b"--", b"--"], TO.keep_mask([b"--", b"--"], TO.MAX_GAPS, 1)) == ""


def test_an_all_gap_row_is_still_a_row():
    rows = [b"A-C", b"---", b"AGC"]
    mask, out = TO.agree(rows, TO.MAX_GAPS, 1)
    assert out == [b"AC", b"--", b"AC"]


def test_no_rows_and_no_columns():
    assert TO.gap_counts([b"", b""]).tolist() == []
    mask, out = TO.agree([b"", b""], TO.MAX_GAPS, 0)
    assert out == [b"", b""] and mask.size == 0


def test_both_statements_agree_on_the_directed_cases():
    cases = TC.all_cases(256, 24, 512, 8)      # (small constants: the cases scale with them; the GPU tests take the kernels' own)
    assert len(cases) >= 35
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.branch
        mask, out = TO.agree(c.rows, c.rule, c.arg)
        if c.name.startswith("kept = 0") or c.name == "to an all-gap row":
            assert mask.sum() == 0
        if c.name.startswith(("kept = W", "max_gaps = n")):
            assert mask.all() and out == c.rows
        if c.name == "three scan rounds, one kept column in the last word":
            assert TO.kept_columns(mask).tolist() == [len(c.rows[0]) - 2]


def test_floor_next_to_an_integer():
    """floor(T * N) with the product taken in double: where the exact product lies within an ulp of an integer the rounded product decides.
    The values are those tests/retree_plan_kats.cpp and test_retree_plan_cpu.py pin for retree_max_gaps, which the command line calls."""
    pinned = {(1.0, 7): 7, (1.0, 16384): 16384, (0.5, 4): 2, (0.25, 3): 0, (0.95, 20): 19, (0.95, 200): 190, (0.1, 10): 1, (0.1, 30): 3, (0.7, 10): 7, (0.3, 10): 3,
              (0.29, 100): 28, (0.57, 100): 56, (float(np.nextafter(0.5, 0.0)), 4): 1, (float(np.nextafter(0.5, 1.0)), 4): 2, (float(np.nextafter(1.0, 0.0)), 16384): 16383,
              (0.0, 5): 0, (1e-9, 5): 0}
    for (T, n), want in pinned.items():
        assert TO.max_gaps(T, n) == want, (T, n)
        # the same from exact arithmetic: the exact product, rounded once to double, then floored
        assert math.floor(float(Fraction(T) * n)) == want, (T, n)
    # 0.95 * 20 is 19 only after rounding: the exact product of the double 0.95 with 20 lies below 19
    assert Fraction(0.95) * 20 < 19 and math.floor(Fraction(0.95) * 20) == 18
    assert Fraction(0.29) * 100 < 29 and float(Fraction(0.29) * 100) < 29.0
