"""twl_compare_create / twl_compare_columns (include/twl_compare.h; compare_kernels.hip.h, twl_compare.inc.hip) through the binding, against
tests/compare_oracle.py, exactly: all five arrays, where the kernels switch (tests/compare_cases.py on the constants of twl_compare_describe),
with poisoned guard words behind every array, and with everything the calls refuse."""
import numpy as np
import pytest

import compare_cases as CC
import compare_oracle as CO

pytestmark = pytest.mark.gpu
KEYS = ("shared", "letters", "distinct", "recovered", "ref_letters")


@pytest.fixture(scope="module")
def consts(gpu):
    from twilight_amd import compare

    T, TILE, STEP, CHUNK = compare.describe()
    assert T >= 64 and TILE >= 16 and STEP >= 2 and CHUNK >= TILE
    return T, TILE, STEP, CHUNK


def _hold(E, R, what, oracle=CO.per_column):
    from twilight_amd import compare

    want = oracle(E, R)
    with compare.Compare(E, R) as c:
        got = c.columns(guard_words=3)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{what}: {k}"
    return got


def _run(cases):
    for c in cases:
        _hold(c.est, c.ref, f"{c.name} ({c.branch})")


def test_known_answer(gpu):
    got = _hold(*CC.known_answer(), "the known answer")
    assert got["shared"].tolist() == [1, 1, 0, 1, 3] and got["recovered"].tolist() == [0, 0, 0, 0, 1]


def test_key_spans(gpu, consts):
    """A column whose keys span T - 1 .. 2T + 1 reference columns; equal counts on both sides of a window boundary."""
    _run(CC.span_cases(consts[0]))


def test_row_counts(gpu, consts):
    """n = 2, 63 .. 257 and around the rows per step; all keys equal, all keys distinct."""
    cases = CC.row_count_cases(consts[2])
    _run(cases)
    from twilight_amd import compare

    n = 257
    E, R = CC.build([[(0, 0)] for _ in range(n)], 1, 1)
    with compare.Compare(E, R) as c:
        got = c.columns()
    assert int(got["shared"][0]) == n * (n - 1) // 2 and int(got["recovered"][0]) == 1


def test_widths(gpu, consts):
    """We and Wr at 1, 63, 64, 65, around the column tile and the scan round; widths that are no multiple of 16."""
    _run(CC.width_cases(consts[1], consts[3]))


def test_scan_rounds_and_gaps(gpu, consts):
    """Letters across a scan round, a round of gaps, a tile of gaps, rows without letters, rows of letters only, a against A."""
    _run(CC.scan_cases(consts[1], consts[3]))


def test_one_cell_holds_every_row(gpu):
    """65 537 and 92 700 rows in one cell: a 32-bit product or sum would be wrong."""
    for c in CC.big_cell_cases():
        n = len(c.est)
        got = _hold(c.est, c.ref, c.name, oracle=CO.per_column_np)
        assert int(got["shared"].astype(object).sum()) == n * (n - 1) // 2 > (1 << 31)


def test_refusals_leave_nothing_behind(gpu):
    """A letter that differs at the last residue of the last row; a count off by one in one row and in two: bad_row is the smaller; a create after
    a refusal succeeds; the arguments the plan refuses."""
    import torch

    from twilight_amd import api, compare

    rng = np.random.default_rng(5)
    rows = CC.random_rows(rng, 8, 70, 75) + [[(c, c + 5) for c in range(0, 70, 3)]]
    E, R = CC.build(rows, 70, 75)
    E[8] = E[8][:69] + b"A"; R[8] = R[8][:74] + b"C"          # the last residue of the last row
    assert CO.check_rows(E, R) == (8, "letters")
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(compare.BadRow, match="letters differ") as ei:
        compare.Compare(E, R)
    assert ei.value.row == 8
    good_E, good_R = CC.random_pair(rng, 9, 70, 75)
    for rows_off in ((6,), (6, 3)):
        E2 = list(good_E)
        for j in rows_off:
            E2[j] = E2[j].replace(b"-", b"A", 1) if b"-" in E2[j] else b"-" + E2[j][1:]
        assert CO.check_rows(E2, good_R) == (min(rows_off), "count")
        with pytest.raises(compare.BadRow, match="letter count differs") as ei:
            compare.Compare(E2, good_R)
        assert ei.value.row == min(rows_off)
    assert torch.cuda.mem_get_info()[0] >= free0, "a refused create left device memory allocated"
    _hold(good_E, good_R, "a create after a refusal")
    for args, why in (((1, 3, [b"A-C"], 3, [b"AC-"]), "at least 2 rows"), ((2, -1, [b"", b""], 3, [b"AC-"] * 2), "negative width"),
                      ((2, 3, None, 3, [b"AC-"] * 2), "bad argument"), ((2, 3, [b"A-C"] * 2, 3, None), "bad argument"), (((1 << 20) + 1, 0, [], 0, []), "too many rows")):
        with pytest.raises(api.TwlError, match=why):
            compare.create_raw(*args)
    with pytest.raises(api.TwlError, match="bad argument"):
        compare.create_raw(2, 3, [b"A-C"] * 2, 3, [b"AC-"] * 2, want_cmp=False)
    with pytest.raises(api.TwlError, match="bad argument"):
        compare.create_raw(2, 3, [b"A-C"] * 2, 3, [b"AC-"] * 2, want_bad=False)


def test_repeatable_and_two_objects(gpu):
    """Two calls of twl_compare_columns in a row give one answer; two objects alive at once keep their own; any output pointer may be NULL."""
    from twilight_amd import compare

    rng = np.random.default_rng(6)
    E1, R1 = CC.random_pair(rng, 40, 300, 280)
    E2, R2 = CC.random_pair(rng, 7, 90, 130)
    w1, w2 = CO.per_column_np(E1, R1), CO.per_column_np(E2, R2)
    with compare.Compare(E1, R1) as a, compare.Compare(E2, R2) as b:
        g1, g2, g1b = a.columns(guard_words=2), b.columns(guard_words=2), a.columns(guard_words=2)
        a.columns_raw()
        b.columns_raw(shared=True, ref_letters=True)
        up, keys, cols, down = a.timing()
        assert keys > 0 and cols > 0 and up >= 0 and down >= 0
    for k in KEYS:
        assert np.array_equal(g1[k], w1[k]) and np.array_equal(g1b[k], w1[k]) and np.array_equal(g2[k], w2[k]), k


def test_zero_width(gpu):
    """We = 0 and Wr = 0: every row is without letters."""
    from twilight_amd import compare

    with compare.Compare([b"", b""], [b"", b""]) as c:
        got = c.columns(guard_words=1)
    assert all(len(got[k]) == 0 for k in KEYS)


@pytest.fixture(scope="module")
def families():
    return [CC.moved_gaps_family(s) for s in range(40)]


def test_moved_gaps_families(gpu, families):
    """40 seeded families (n <= 300, W <= 3000 + a quarter) whose estimate is the reference with its gaps moved at random."""
    assert max(len(E) for E, _ in families) > 100 and max(len(R[0]) for _, R in families) > 1000
    for s, (E, R) in enumerate(families):
        _hold(E, R, f"family {s}: {len(E)} x {len(E[0])} against {len(R[0])}", oracle=CO.per_column_np)
