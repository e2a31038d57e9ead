"""The numpy restatement of the rebuilt guide tree (tests/retree_oracle.py) pinned on alignments whose masks, counts and trees were derived by
hand (tests/retree_cases.py): a column exactly at max_gaps and one above it, lower case, U against T, N against N, a pair with both = 0,
the protein letters.  No GPU needed."""
import numpy as np
import pytest

import retree_cases as K
import retree_oracle as R


@pytest.mark.parametrize("name", sorted(K.HAND))
def test_hand_derived_alignment(name):
    c = K.HAND[name]
    n = len(c["rows"])
    assert R.max_gaps(c["T"], n) == c["max_gaps"]
    assert R.column_gaps(c["rows"]).tolist() == c["gaps"]
    assert R.kept_columns(c["rows"], c["max_gaps"]).astype(int).tolist() == c["kept"]
    match, both, kept = R.pair_counts(c["rows"], c["type"], c["max_gaps"])
    assert both.tolist() == c["both"] and match.tolist() == c["match"] and kept == sum(c["kept"])
    assert match.dtype == both.dtype == np.uint32
    assert (match == match.T).all() and (both == both.T).all() and (np.diag(match) == np.diag(both)).all()
    assert R.tree_of(c["names"], c["rows"], c["type"], c["T"]) == c["tree"]


def test_the_edges_of_the_mask_and_the_letters():
    c = K.HAND["n_mask"]
    g = R.column_gaps(c["rows"])
    assert g[2] == c["max_gaps"] and c["kept"][2] == 1, "a column exactly at max_gaps is kept"
    assert g[4] == c["max_gaps"] + 1 and c["kept"][4] == 0, "a column one above it is not"
    match, both, _ = R.pair_counts(c["rows"], "n", c["max_gaps"])
    # rows 0 and 1: T against U in column 3 is a match, a against C in column 6 is none, N against N in column 7 is not even in both
    assert both[0, 1] == 5 and match[0, 1] == 4
    t = R.letter_table("n")
    assert t[ord("U")] == t[ord("t")] == 3 and t[ord("N")] == t[ord("-")] == t[ord(".")] == t[ord("X")] == -1
    p = R.letter_table("p")
    assert [p[ord(ch)] for ch in "ACDEFGHIKLMNPQRSTVWY"] == list(range(20)) and p[ord("y")] == 19
    assert all(p[ord(ch)] == -1 for ch in "BZXJOU*-.")


def test_distances():
    match = np.array([[4, 3, 0], [3, 5, 0], [0, 0, 0]], dtype=np.uint32)
    both = np.array([[4, 4, 0], [4, 5, 0], [0, 0, 0]], dtype=np.uint32)
    d = R.distances(match, both)
    assert d[0, 1] == 1.0 - 3.0 / 4.0 and d[0, 2] == 1.0 and d[1, 2] == 1.0 and (np.diag(d) == 0).all(), "both = 0 gives 1, the diagonal is 0 even there"


def test_max_gaps_known_values():
    assert R.max_gaps(1.0, 7) == 7 and R.max_gaps(0.5, 4) == 2 and R.max_gaps(0.25, 3) == 0 and R.max_gaps(0.95, 20) == 19 and R.max_gaps(0.95, 200) == 190


def test_the_directed_rows_are_what_they_are_listed_for():
    rows, facts = K.directed_rows(600, 512, seed=5)
    K.check_directed(rows, facts, 512)
    K.masked_match_rows(10, 40, seed=6)
