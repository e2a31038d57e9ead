"""The comparison's oracle (tests/compare_oracle.py): its statements held to each other -- per column with a dictionary of keys, a brute force
over all row pairs, and the numpy form the larger GPU cases use -- on the known answer of include/twl_compare.h's definitions and on seeded small
families; the rule of the refusal; the report line.  No GPU needed."""
import numpy as np
import pytest

import compare_cases as CC
import compare_oracle as CO

KEYS = ("shared", "letters", "distinct", "recovered", "ref_letters")


def _three_ways(E, R):
    a = CO.agree(E, R)
    b = CO.per_column_np(E, R)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    return a


def test_known_answer():
    E, R = CC.known_answer()
    cols = _three_ways(E, R)
    assert cols["shared"].tolist() == [1, 1, 0, 1, 3]
    assert [int(n) * (int(n) - 1) // 2 for n in cols["letters"]] == [1, 3, 1, 1, 3]
    assert cols["recovered"].tolist() == [0, 0, 0, 0, 1]
    t = CO.totals(cols)
    assert t == {"shared": 6, "pairs_out": 9, "pairs_ref": 10, "recovered": 1, "ref_columns": 4}
    assert CO.report(cols, 3, 0, 0) == ("compare: rows 3 (0 only in the output, 0 only in the reference) pairs_out 9 pairs_ref 10 shared 6 SP 0.600000 modeler 0.666667 "
                                        "TC 1/4 columns 5/5")


def test_known_answer_by_hand_over_row_pairs():
    """The 6 shared pairs, spelled out: residue pairs of E columns that R also puts into one column."""
    E, R = CC.known_answer()
    pe, pr = [CO.positions(e) for e in E], [CO.positions(r) for r in R]
    pairs = 0
    for i in range(3):
        for j in range(i + 1, 3):
            for a, c in enumerate(pe[i]):
                if c in pe[j] and pr[i][a] == pr[j][pe[j].index(c)]:
                    pairs += 1
    assert pairs == 6


@pytest.mark.parametrize("seed", range(12))
def test_seeded_small_families(seed):
    rng = np.random.default_rng(seed)
    n, We, Wr = int(rng.integers(2, 9)), int(rng.integers(1, 30)), int(rng.integers(1, 30))
    E, R = CC.random_pair(rng, n, We, Wr, empty_rows=0.15, full_rows=0.15)
    cols = _three_ways(E, R)
    t = CO.totals(cols)
    assert t["shared"] <= min(t["pairs_out"], t["pairs_ref"]) and t["recovered"] <= t["ref_columns"]
    assert int(cols["letters"].sum()) == int(cols["ref_letters"].sum())


def test_an_alignment_against_itself():
    rng = np.random.default_rng(3)
    E, _ = CC.random_pair(rng, 6, 25, 25)
    cols = _three_ways(E, E)
    t = CO.totals(cols)
    assert t["shared"] == t["pairs_out"] == t["pairs_ref"] and t["recovered"] == t["ref_columns"]
    assert np.array_equal(cols["recovered"], (cols["letters"] >= 2).astype(np.uint8))


def test_ratios_over_zero_print_nan():
    E, R = [b"A-", b"-C"], [b"-A", b"C-"]
    cols = _three_ways(E, R)
    assert CO.report(cols, 2, 1, 2).endswith("pairs_out 0 pairs_ref 0 shared 0 SP nan modeler nan TC 0/0 columns 2/2")


def test_the_rule_of_the_refusal():
    assert CO.check_rows([b"AC-", b"a-c"], [b"A-C", b"AC-"]) is None
    assert CO.check_rows([b"AC-", b"A-G"], [b"A-C", b"AC-"]) == (1, "letters")
    assert CO.check_rows([b"ACG", b"A-G", b"A--"], [b"A-C", b"AG-", b"AC-"]) == (0, "count")
    assert CO.check_rows([b"A.C"], [b"AC-"]) == (0, "count"), "'.' is a letter"


def test_the_files_reader(tmp_path):
    import gzip

    p = tmp_path / "a.aln.gz"
    with gzip.open(p, "wb") as f:
        f.write(b">x first\nAC\n-G\n>y\nA--T\n>x\nTTTT\n")
    names, rows = CO.read_alignment(p)
    assert names == ["x", "y"] and rows == {"x": b"AC-G", "y": b"A--T"}
