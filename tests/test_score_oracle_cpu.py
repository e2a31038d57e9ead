"""tests/score_oracle.py held to itself: the walk over projection strings (a) against the big-integer carry (b) and the column formulas, on
every directed case of tests/score_cases.py and on seeded random rows; every claim of the directed cases; the independence of (b) from the
number of pad bits; the score's formula on a case worked by hand.  No GPU needed."""
import numpy as np
import pytest

import score_cases as SC
import score_oracle as SO

S, T, R, F = 16, 64, 512, 252      # the constants of the kernels (test_score_plan_cpu.py holds twl_score_describe to them)
CASES = SC.all_cases(S, T, R, F)
WALK_BUDGET = 20000                # ordered pairs the walk takes per case; above it a seeded sample of the pairs


def _pairs(n, seed):
    if n * (n - 1) <= WALK_BUDGET:
        return None
    rng = np.random.default_rng(seed)
    got = {(0, n - 1), (n - 1, 0)}
    while len(got) < 4000:
        i, j = (int(x) for x in rng.integers(0, n, size=2))
        if i != j:
            got.add((i, j))
    return sorted(got)


def test_the_cases_cover_what_the_issue_lists():
    names = {c.name for c in CASES}
    for must in ("closing bit in the next word", "closing bit three words up", "bit 63 and bit 0", "run to the last column", "a row without letters", "two identical rows",
                 "terminal runs at one end only", "every nucleotide class", "every protein class"):
        assert must in names
    assert {len(c.rows[0]) for c in SC.width_cases(S)} == {1, 63, 64, 65, S * 64 - 1, S * 64, S * 64 + 1}
    assert {len(c.rows) for c in SC.row_count_cases(T)} == {2, 63, 64, 65, 129}
    assert {len(c.rows) for c in SC.counter_cases(R, F)} == {F - 1, F, F + 1, R - 1, R, R + 1}
    assert len(names) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_claims_and_both_statements(case):
    assert len({len(r) for r in case.rows}) == 1
    if case.claim:
        case.claim(SO, case)
    pairs = _pairs(len(case.rows), 5)
    runs_a, tot_a = SO.walk_all(case.rows, pairs)
    assert runs_a == SO.carry_runs_row(case.rows, pairs=pairs)
    W = len(case.rows[0])
    assert runs_a == SO.carry_runs_row(case.rows, bits=(W + S * 64 - 1) // (S * 64) * (S * 64), pairs=pairs), "pad bits change nothing"
    if pairs is None:
        tot_b = SO.column_totals(case.rows)
        assert {k: tot_a[k] for k in ("G", "RT", "GT")} == {k: tot_b[k] for k in ("G", "RT", "GT")}
        assert tot_b["letters"] == sum(1 for r in case.rows for b in r if b != SO.GAP)


@pytest.mark.parametrize("seed,n,W,p_gap", [(1, 7, 130, 0.5), (2, 12, 70, 0.9), (3, 9, 200, 0.1), (4, 20, 33, 0.7)])
def test_random_rows_both_statements(seed, n, W, p_gap):
    rng = np.random.default_rng(seed)
    rows = SC.random_rows(rng, n, W, p_gap)
    rows[0] = b"-" * W                                     # a row without letters among them
    rows[1] = rows[2]                                       # and two identical rows
    runs_a, tot_a = SO.walk_all(rows)
    sub, runs_b, tot_b = SO.expected(rows, "n")
    assert runs_a == runs_b and tot_a == {k: tot_b[k] for k in ("R", "G", "RT", "GT")}
    assert tot_b["RT"] <= tot_b["R"] and tot_b["GT"] <= tot_b["G"] and tot_b["R"] - tot_b["RT"] <= tot_b["G"] - tot_b["GT"]
    # sub against pairs of rows counted one by one
    K = 4
    naive = np.zeros((K + 1, K + 1), dtype=object)
    for i in range(n):
        for j in range(i + 1, n):
            for x, y in zip(rows[i], rows[j]):
                a, b = SO.class_of(x, "n"), SO.class_of(y, "n")
                if a is not None and b is not None:
                    naive[min(a, b), max(a, b)] += 1
    assert (naive == sub).all()


def test_the_score_by_hand():
    """Two rows AC-GT / A--GT: columns A/A, G/G, T/T match (3 x 18), C against '-' is an inner run of row 1 against row 0 (1 column): open."""
    rows = [b"AC-GT", b"A--GT"]
    sub, runs, tot = SO.expected(rows, "n")
    assert runs == [0, 1] and tot == dict(R=1, G=1, RT=0, GT=0, letters=7)
    assert SO.score(sub, tot, SO.nucleotide_matrix(), -50.0, -5.0, -5.0, 4) == 3 * 18 - 50
    # a terminal run of two columns costs 2 x ends; an inner run of three costs open + 2 x extend
    rows = [b"ACGTACGTA", b"--GT---TA"]
    sub, runs, tot = SO.expected(rows, "n")
    assert tot == dict(R=2, G=5, RT=1, GT=2, letters=13)
    assert SO.score(sub, tot, SO.nucleotide_matrix(), -50.0, -5.0, -1.0, 4) == 4 * 18 + (-50 + 2 * -5) + 2 * -1


def test_classes():
    assert [SO.class_of(b, "n") for b in b"ACGTUacgtu"] == [0, 1, 2, 3, 3] * 2
    assert [SO.class_of(b, "n") for b in b"N.*\x80R"] == [4] * 5 and SO.class_of(0x2D, "n") is None
    assert [SO.class_of(b, "p") for b in SO.PROT] == list(range(20)) == [SO.class_of(b, "p") for b in SO.PROT.lower()]
    assert [SO.class_of(b, "p") for b in b"BJOUXZ*."] == [20] * 8
