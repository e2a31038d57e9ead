"""The directed inputs of the comparison (tests/compare_cases.py) do what their names say, proved with the oracle on the constants of
twl_compare_describe: the key span of the column, the window every key falls in, the scan round a carry crosses, the counts that pass 32 bits.
No GPU needed."""
import numpy as np
import pytest

import compare_cases as CC
import compare_oracle as CO


@pytest.fixture(scope="module")
def consts(built):
    from twilight_amd import compare

    return compare.describe()


def _keys_of_column(E, R, c):
    """The R columns of the residues of E column c."""
    out = []
    for e, r in zip(E, R):
        pe, pr = CO.positions(e), CO.positions(r)
        if c in pe:
            out.append(pr[pe.index(c)])
    return out


def test_span_cases_put_keys_into_the_windows_they_name(consts):
    T = consts[0]
    cases = CC.span_cases(T)
    spans = {}
    for case in cases[:-1]:
        keys = _keys_of_column(case.est, case.ref, 1)
        lo, hi = min(keys), max(keys)
        windows = sorted({(k - lo) // T for k in keys})
        spans[hi - lo] = windows
        assert keys.count(lo) >= 2 and keys.count(hi) >= 2, "duplicates at both ends: the first and the last window both add pairs"
        assert len(case.ref[0]) > 2 * T
        cols = CO.agree(case.est, case.ref)
        assert int(cols["shared"][1]) == 1 + 3 and int(cols["distinct"][1]) == len(set(keys))
    assert set(spans) >= {T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1}      # largest - smallest: T - 1 is the last one-window span
    assert spans[T - 1] == [0] and spans[T][-1] == 1 and spans[2 * T - 1][-1] == 1 and spans[2 * T][-1] == 2 and spans[2 * T + 1][-1] == 2
    case = cases[-1]
    keys = _keys_of_column(case.est, case.ref, 0)
    lo = min(keys)
    assert keys.count(lo + T - 1) == keys.count(lo + T) == 3, "the last counter of window 0 and the first of window 1 hold the same count"
    assert int(CO.agree(case.est, case.ref)["shared"][0]) == 6


def test_row_count_cases(consts):
    STEP = consts[2]
    cases = CC.row_count_cases(STEP)
    assert {len(c.est) for c in cases} >= {2, 63, 64, 65, 255, 256, 257, STEP - 1, STEP, STEP + 1}
    for c in cases:
        n = len(c.est)
        cols = CO.per_column(c.est, c.ref)
        if "equal" in c.name:
            assert int(cols["shared"][0]) == n * (n - 1) // 2 and int(cols["recovered"][0]) == 1
        else:
            assert int(cols["shared"][0]) == 0 and int(cols["distinct"][0]) == n and int(cols["recovered"][0]) == 0


def test_width_cases(consts):
    T, TILE, STEP, CHUNK = consts
    cases = CC.width_cases(TILE, CHUNK)
    we = {len(c.est[0]) for c in cases}
    wr = {len(c.ref[0]) for c in cases}
    for must in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1):
        assert must in we and must in wr, must
    assert any(w % 16 for w in we) and any(w % 16 for w in wr)
    for c in cases:
        assert CO.check_rows(c.est, c.ref) is None


def test_scan_cases(consts):
    T, TILE, STEP, CHUNK = consts
    cases = {c.name: c for c in CC.scan_cases(TILE, CHUNK)}
    c = cases["letters straddle a scan round; gaps fill a whole round"]
    pe, pr = CO.positions(c.est[0]), CO.positions(c.ref[0])
    assert pe[0] // CHUNK == 0 and pe[-1] // CHUNK == 1 and pr[0] // CHUNK == 1 and pr[-1] // CHUNK == 2, "the row's letters lie on both sides of a round boundary"
    pe, pr = CO.positions(c.est[1]), CO.positions(c.ref[1])
    assert {p // CHUNK for p in pe} == {0, 2} and {p // CHUNK for p in pr} == {1, 2}, "a whole round of gaps between letters: the carry crosses it unchanged"
    c = cases["a whole tile of gaps, columns of gaps, rows without letters"]
    cols = CO.agree(c.est, c.ref)
    assert not cols["letters"][TILE:2 * TILE].any() and cols["letters"][:TILE].any() and cols["letters"][2 * TILE:].any()
    assert any(not CO.positions(e) for e in c.est)
    c = cases["rows of letters only beside a row without letters"]
    assert b"-" not in c.est[0] and not CO.positions(c.est[3])
    c = cases["a against A"]
    assert c.est != c.ref and [e.replace(b"-", b"").upper() for e in c.est] == [r.replace(b"-", b"").upper() for r in c.ref]
    assert any(e.replace(b"-", b"") != r.replace(b"-", b"") for e, r in zip(c.est, c.ref)) and CO.check_rows(c.est, c.ref) is None


def test_big_cells_pass_32_bits():
    (a, b) = CC.big_cell_cases()
    na, nb = len(a.est), len(b.est)
    assert na == 65537 and na * (na - 1) >= 1 << 32 > (na - 1) * (na - 2), "the first n whose product n (n - 1) needs 33 bits"
    assert nb == 92700 and nb * (nb - 1) // 2 >= 1 << 32, "C(n, 2) needs 33 bits"
    for c in (a, b):
        n = len(c.est)
        cols = CO.per_column_np(c.est, c.ref)
        assert int(cols["shared"][1]) == n * (n - 1) // 2 and 2 <= len(c.est[0]) <= 4 and 2 <= len(c.ref[0]) <= 4


def test_moved_gaps_families_are_legal_and_varied():
    fams = [CC.moved_gaps_family(s) for s in range(40)]
    assert all(2 <= len(E) <= 300 and len(R[0]) <= 3000 for E, R in fams)
    assert max(len(E) for E, _ in fams) > 100 and max(len(R[0]) for _, R in fams) > 1000
    for E, R in fams[:6]:
        assert CO.check_rows(E, R) is None
    E, R = fams[1]
    a, b = CO.per_column(E, R), CO.per_column_np(E, R)
    for k in a:
        assert np.array_equal(a[k], b[k])
