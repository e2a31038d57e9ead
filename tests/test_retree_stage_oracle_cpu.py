"""The restatement of the two-stage rebuilt guide tree (tests/retree_stage_oracle.py) against what can be known without it: as many seeds as
rows give the one-stage tree of tests/retree_oracle.py byte for byte, a 6-row alignment whose assignment, clusters and text are derived by
hand below, and the near tie that single precision cannot order.  No GPU needed."""
import numpy as np
import pytest

import retree_cases as cases
import retree_oracle as R
import retree_stage_oracle as RS
from retree_stage_cases import near_tie_rows

# ---- hand-derived: 'n', 6 x 8, T = 1 (max_gaps = 6: every column is kept), S = 2: the seeds are rows floor(0 * 6 / 2) = 0 and floor(1 * 6 / 2) = 3
#
#            01234567        with r0: match / both     with r3: match / both     goes to
#   r0       AAAAAAAA        seed 0                                              0 (itself), counts 8, 8
#   r1       AAAAAACC        6 / 8                     2 / 8                     0
#   r2       AAACCCCC        3 / 8                     5 / 8                     1
#   r3       CCCCCCCC                                  seed 1                    1 (itself), counts 8, 8
#   r4       CCCCCCAA        2 / 8                     6 / 8                     1
#   r5       ACACAC--        3 / 6                     3 / 6                     0: equal ratios go to the smaller t
#
# K_0 = [r0, r1, r5]: d(r0, r1) = 1 - 6/8 = 0.25, d(r0, r5) = 1 - 3/6 = 0.5, d(r1, r5) = 1 - 3/6 = 0.5 (r1 holds A in columns 0 .. 5).
#   (r0, r1) at 0.125; d(r0r1, r5) = (0.5 + 0.5) / 2 = 0.5: root at 0.25.       ((r0:0.125,r1:0.125):0.125,r5:0.25), height 0.25
# K_1 = [r2, r3, r4]: d(r2, r3) = 1 - 5/8 = 0.375, d(r2, r4) = 1 - 3/8 = 0.625 (equal in columns 3 .. 5 only), d(r3, r4) = 1 - 6/8 = 0.25.
#   (r3, r4) at 0.125; d(r2, r3r4) = (0.375 + 0.625) / 2 = 0.5: root at 0.25.   (r2:0.25,(r3:0.125,r4:0.125):0.125), height 0.25
# seeds [r0, r3]: d = 1 - 0/8 = 1: root at 0.5, both grafted roots stand at 0.25: two branches of 0.25.
HAND = {
    "names": ["r0", "r1", "r2", "r3", "r4", "r5"],
    "rows": [b"AAAAAAAA", b"AAAAAACC", b"AAACCCCC", b"CCCCCCCC", b"CCCCCCAA", b"ACACAC--"],
    "seed_of": [0, 0, 1, 1, 1, 0],
    "match": [8, 6, 5, 8, 6, 3],
    "both": [8, 8, 8, 8, 8, 6],
    "clusters": [[0, 1, 5], [2, 3, 4]],
    "tree": "(((r0:0.125000,r1:0.125000):0.125000,r5:0.250000):0.250000,(r2:0.250000,(r3:0.125000,r4:0.125000):0.125000):0.250000);\n",
}


def test_the_hand_derived_alignment():
    seed_of, match, both = RS.assign(HAND["rows"], "n", 6, [0, 3])
    assert seed_of.tolist() == HAND["seed_of"] and match.tolist() == HAND["match"] and both.tolist() == HAND["both"]
    text, k = RS.tree_of(HAND["names"], HAND["rows"], "n", 2, T=1.0)
    assert k == HAND["clusters"]
    assert text == HAND["tree"]


def test_seeds_out_of_order_are_positions():
    seed_of, match, both = RS.assign(HAND["rows"], "n", 6, [3, 0])
    assert seed_of.tolist() == [1, 1, 0, 0, 0, 0]      # r5's tie goes to the smaller t, which is now row 3
    assert match.tolist() == HAND["match"] and both.tolist() == HAND["both"]


def test_the_mask_is_taken_over_all_rows():
    """max_gaps = 0 drops columns 6 and 7 (r5 holds '-' there) for every pair, also for pairs of rows that hold letters there."""
    seed_of, match, both = RS.assign(HAND["rows"], "n", 0, [0, 3])
    assert both.tolist() == [6] * 6 and match.tolist() == [6, 6, 3, 6, 6, 3]
    assert seed_of.tolist() == [0, 0, 0, 1, 1, 0]      # r2 now has 3 / 6 with both seeds: the smaller t


@pytest.mark.parametrize("case", ["hand_n_mask", "seeded_n", "seeded_p"])
def test_as_many_seeds_as_rows_is_the_one_stage_tree(case):
    if case == "hand_n_mask":
        h = cases.HAND["n_mask"]
        names, rows, type_, T = h["names"], h["rows"], h["type"], h["T"]
    else:
        type_ = case[-1]
        rows = cases.seeded_rows(type_, 13, 70, 11)
        names, T = ["s%d" % i for i in range(13)], 0.95
    text, k = RS.tree_of(names, rows, type_, len(rows), T=T)
    assert k == [[i] for i in range(len(rows))]
    assert text == R.tree_of(names, rows, type_, T)
    if case == "hand_n_mask":
        assert text == h["tree"]


def test_the_near_tie_goes_to_the_larger_t():
    rows, seeds, i = near_tie_rows()
    m, b, _ = R.pair_counts(rows, "n", len(rows))
    assert (m[i, 0], b[i, 0], m[i, 1], b[i, 1]) == (8191, 8192, 8192, 8193)
    assert np.float32(8191) / np.float32(8192) == np.float32(8192) / np.float32(8193), "single precision cannot order the two ratios"
    seed_of, match, both = RS.assign(rows, "n", len(rows), seeds)
    assert seed_of[i] == 1 and (match[i], both[i]) == (8192, 8193)
    # and with the two seeds exchanged the same seed row wins, now at t = 0
    seed_of, match, both = RS.assign(rows, "n", len(rows), [1, 0])
    assert seed_of[i] == 0 and (match[i], both[i]) == (8192, 8193)


def test_rows_without_letters():
    """A row with no letter in a kept column goes to seed 0 with counts 0, 0; a seed without letters keeps itself."""
    rows = [b"ACGT", b"----", b"NNNN", b"ACGA", b"----"]
    seed_of, match, both = RS.assign(rows, "n", 5, [3, 4, 0])
    assert seed_of.tolist() == [2, 0, 0, 0, 1]
    assert match.tolist() == [4, 0, 0, 4, 0] and both.tolist() == [4, 0, 0, 4, 0]
