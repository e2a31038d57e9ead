"""The directed inputs of tests/test_gpu_div_edges.py are what each of them claims.  No GPU.

Score cases (div_cases.SCORE_CASES): in plain numpy float32, in the oracle's order of operations (div_cases.numerators, held to
twlo_column_score here), every planned cell has exactly the numerator it names (2^-73, 0, the maximum ...), every entry, score and
denominator passes the three guards as the code states them, every mode's cases reach every corner, and -- by the oracle's trace -- the
band is the whole matrix, so the dump of the DP kernel holds every cell.

Guard cases (div_cases.GUARD_CASES): the changed entry's row or column lies inside the band on some diagonal, exactly one value of
the pool differs, and the spans of the changed pool are the committed ones of dp_cases.py (the pool is still a margin pool of its
window, or still just over it).  Nothing is skipped or filtered: a case that does not reach its class fails here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import div_cases as V  # noqa: E402
import dp_cases as D  # noqa: E402
import oracle_lib as O  # noqa: E402

F = np.float32


def matrix_mode(mat):
    """plan_nucleotide's matrix mode (twl_policy.inc.hip): 2 match / transition / transversion with a zero N row and column, 1 zero N row and column, 0 anything."""
    nz = all(mat[4, t] == 0 and mat[t, 4] == 0 for t in range(5))
    st3 = all(mat[l, m] == (mat[0, 0] if l == m else (mat[0, 2] if (l ^ m) == 2 else mat[0, 1])) for l in range(4) for m in range(4))
    return (2 if st3 else 1) if nz else 0


@pytest.mark.parametrize("case", V.SCORE_CASES, ids=lambda c: c.name)
def test_score_case_is_what_it_claims(case):
    n = case.numer()
    d = case.denom
    # the three guards
    assert all(V.entry_ok(x) for x in case.ref.ravel()) and all(V.entry_ok(x) for x in case.qry.ravel())
    assert all(V.score_ok(x) for x in case.matrix.ravel()) and V.score_ok(case.gap_char) and case.gap_char != 0
    assert V.denom_ok(case.nums)
    # the mode the launch policy gives the matrix
    if case.P == 6:
        assert matrix_mode(case.matrix) == {"nuc2": 2, "nuc2_leaf": 2, "nuc5": 2, "nuc1": 1, "nuc0": 0}[case.mode]
    if case.onehot_query:
        assert all(np.count_nonzero(r) == 1 and r[4] == 0 and r[5] == 0 for r in case.qry)
    if case.mode == "nuc2_leaf":
        assert case.nums == (1, 1)
    # the numerators' range: what fast_div's comment names
    nz = n[n != 0]
    assert np.abs(nz).min() >= F(2.0 ** -73) and np.abs(nz).max() <= F(2.0 ** 80), (np.abs(nz).min(), np.abs(nz).max())
    # the planned cells
    for i, j, corner, want in case.planned:
        if want is not None:
            assert n[i, j] == want, (corner, n[i, j], want)
        if corner == "gap_char_on_limit":
            assert abs(case.gap_char) in (V.SCORE_LO, V.SCORE_HI)
        if corner == "score_hi":
            assert V.SCORE_HI in np.abs(case.matrix) and V.ENTRY_HI in case.ref[j] and V.ENTRY_HI in case.qry[i]
        if corner == "score_lo":
            assert V.SCORE_LO in np.abs(case.matrix) and V.ENTRY_LO in case.ref[j] and V.ENTRY_LO in case.qry[i]
        if corner.startswith("denom_"):
            want_d = {"denom_1": F(1), "denom_2p40": F(2.0 ** 40), "denom_2p40_rounded": F(2.0 ** 40), "denom_2p40_below": V.down(2.0 ** 40)}.get(corner)
            assert want_d is None or d == want_d, (corner, d)
            if corner == "denom_2p40_rounded":
                assert case.nums[0] * case.nums[1] == (1 << 40) - 1
            if corner == "denom_odd":
                assert (case.nums[0] * case.nums[1]) % 2 == 1 and 3 <= d <= 21
        if corner == "max_numerator":      # every term that exists is -(2^30 * 2^10 * 2^30)
            r, q, M = case.ref[j], case.qry[i], case.matrix
            assert set(r[r != 0]) == {V.ENTRY_HI} and set(q[q != 0]) == {V.ENTRY_HI} and case.gap_char == -V.SCORE_HI
            assert all(M[l, m] in (-V.SCORE_HI, 0) for l in range(case.P - 1) for m in range(case.P - 1) if r[l] != 0 and q[m] != 0)
    # the DP can use the scores: nothing large and positive, a start cell of ordinary size (see div_cases)
    s = n / d
    assert s.max() <= 2.0 ** 21 and abs(s[0, 0]) <= 2.0 ** 10, (s.max(), s[0, 0])


@pytest.mark.parametrize("case", V.SCORE_CASES[::7], ids=lambda c: c.name)
def test_numpy_numerators_are_the_oracles(case):
    """div_cases.numerators against twlo_column_score itself (denominator 1: the quotient is the numerator), every cell of a sample of the cases."""
    op = O.make_params(case.matrix, **case.params())
    n = case.numer()
    got = np.array([[O.column_score(op, case.ref[j], case.qry[i], 1.0) for j in range(case.ref.shape[0])] for i in range(case.qry.shape[0])], dtype=F)
    assert np.array_equal(got, n)


@pytest.mark.parametrize("case", V.SCORE_CASES, ids=lambda c: c.name)
def test_band_of_a_score_case_is_the_whole_matrix(case):
    b = case.batch()
    R, Q = int(b.len[0, 0]), int(b.len[0, 1])
    rec = []
    _, err, st = O.align_pair(O.make_params(case.matrix, **case.params()), b.freq[0, 0, :R], b.freq[0, 1, :Q], b.gap_open[0, 0, :R], b.gap_extend[0, 0, :R],
                              b.gap_open[0, 1, :Q], b.gap_extend[0, 1, :Q], case.nums[0], case.nums[1], trace=lambda _u, tile, k, L, U, _s: rec.append((tile, k, L, U)))
    assert err == 0 and st.tiles == 1 and len(rec) == R + Q - 1
    for _t, k, L, U in rec:
        assert (L, U) == (max(0, k - R + 1), min(k, Q - 1)), (k, L, U)
    assert st.cells == R * Q


def test_every_mode_reaches_every_corner():
    for mode in V.MODES:
        have = set().union(*(c.corners() for c in V.SCORE_CASES if c.mode == mode))
        want = V.LEAF_CORNERS if mode == "nuc2_leaf" else V.CORNERS
        assert have >= set(want), (mode, sorted(set(want) - have))
        # the smallest numerator against d = 1 and d = 2^40; the largest one too
        for corner in ("min_numerator", "max_numerator"):
            ds = {float(c.denom) for c in V.SCORE_CASES if c.mode == mode and corner in c.corners()}
            assert 1.0 in ds and (mode == "nuc2_leaf" or 2.0 ** 40 in ds), (mode, corner, ds)
    assert {"nuc2", "nuc2_leaf", "nuc5", "nuc1", "nuc0", "prot3"} == set(V.MODES)
    # the denominators: 2^40 - 1 as integers rounds to 2^40, the pair below it is the largest float under 2^40, the random ones spread over the range
    assert V.denom_of(V.DENOMS["d2p40_rounded"]) == F(2.0 ** 40) and V.denom_of(V.DENOMS["d2p40_below"]) == np.nextafter(F(2.0 ** 40), F(0))
    logs = sorted(np.log2(float(V.denom_of(v))) for k, v in V.DENOMS.items() if k.startswith("r_"))
    assert logs[0] < 15 and logs[-1] > 30 and all(b - a < 10 for a, b in zip(logs, logs[1:]))


def test_random_fill_covers_the_entry_range():
    """Entries of the random fill reach both ends of [2^-20, 2^30] (within a binade or two) on each side; the matrices of the fill have both signs."""
    for mode in V.MODES:
        cs = [c for c in V.SCORE_CASES if c.mode == mode]
        for side in ("ref", "qry"):
            e = np.concatenate([getattr(c, side).ravel() for c in cs])
            e = e[e != 0]
            assert e.min() == V.ENTRY_LO and e.max() == V.ENTRY_HI
            h, _ = np.histogram(np.log2(e), bins=10, range=(-20, 30))
            assert h.min() > 0, (mode, side, h)
        assert any((c.matrix > 0).any() and (c.matrix < 0).any() for c in cs)


# ---- guard cases ----
_BASE = {}


def _base(pool):
    if pool not in _BASE:
        _BASE[pool] = V.pool_of(pool).batch()
    return _BASE[pool]


@pytest.mark.parametrize("case", V.GUARD_CASES, ids=lambda c: c.name)
def test_guard_case_is_what_it_claims(case):
    base = _base(case.pool)
    b = case.batch(base)
    mat = D.matrix_of(case.P)
    changes = case.changes(base)
    # ONE changed entry per carrying pair (or its member counts), nothing else
    diff = np.argwhere(b.freq != base.freq)
    assert sorted(map(tuple, diff.tolist())) == sorted(changes) and len(changes) == (len(case.carriers) if case.value else 0)
    for n, side, i, t in changes:
        x = b.freq[n, side, i, t]
        assert base.freq[n, side, i, t] == 0 and x == V.VALUES[case.value]
        assert V.entry_ok(x) == (case.value in ("lo", "hi"))
        assert x in (V.ENTRY_LO, np.nextafter(V.ENTRY_LO, F(0)), V.ENTRY_HI, np.nextafter(V.ENTRY_HI, F(np.inf)))
        if case.where == "gap_letter":
            assert t == case.P - 1
        if case.where == "last_ref_col":
            assert side == 0 and i == int(b.len[n, 0]) - 1
        if case.where == "last_query_row":
            assert side == 1 and i == int(b.len[n, 1]) - 1
        if case.where == "first_tile":
            assert side == 1 and i < 64
        if case.where == "tile_boundary":      # the path's match step in that column lies on an anti-diagonal a tile can begin on
            ks = V.path_diagonals(b, n, side, i, mat, **case.params())
            assert ks and all(any((case.marker - 1) * t <= k <= case.marker * t for t in range(1, 40)) for k in ks), ks
        # inside the band: the optimal path takes a match step through that row / column
        assert V.on_path(b, n, side, i, mat, **case.params()), (case.name, n, side, i)
    nums_changed = {n for n in range(b.n_pairs) if tuple(b.num[n]) != tuple(base.num[n])}
    assert nums_changed == {n for n, _ab in case.nums}
    # what the lean kernels must hand back: an entry outside the range with a denominator other than 1, or a denominator above 2^40
    want = set()
    for n in range(b.n_pairs):
        d = V.denom_of(tuple(int(v) for v in b.num[n]))
        entries_ok = all(V.entry_ok(x) for x in b.freq[n].ravel()[np.flatnonzero(b.freq[n].ravel() != base.freq[n].ravel())])
        if not V.denom_ok(b.num[n]) or (not entries_ok and d != 1):
            want.add(n)
    assert want == set(case.rerun), (case.name, want, case.rerun)
    # the spans are the committed ones: the pool is still in its class
    traces = pool_traces(case, b)
    assert tuple(t.err for t in traces) == (0,) * b.n_pairs
    assert tuple(t.span for t in traces) == case.expected_spans(), (case.name, [t.span for t in traces])
    if case.pool in V.TILE_SPANS and case.marker == 1024:      # (the walk of the ladder runs at the default marker)
        assert tuple(tuple(t.tile_span) for t in traces) == V.TILE_SPANS[case.pool], (case.name, [t.tile_span for t in traces])
    pool = V.pool_of(case.pool)
    if pool.kind == "margin":
        assert all(pool.nv - 2 <= s <= pool.nv - 1 for s in case.expected_spans())
    elif pool.kind == "over":
        assert any(s == pool.nv for s in case.expected_spans())
    else:
        assert max(case.expected_spans()) < 8      # a short pool fits every window there is


def pool_traces(case, b):
    return V.pool_of(case.pool).__class__.traces(_Params(case), b)


class _Params:
    """What DpCase.traces needs of a case: the alphabet and the oracle's parameters (the guard case's own: its marker may differ)."""
    def __init__(self, case):
        self.P = case.P
        self._pk = case.params()

    def params(self):
        return self._pk


def test_guard_cases_cover_positions_values_and_twins():
    names = set(V.GUARD_BY_NAME)
    assert len(names) == len(V.GUARD_CASES)
    # every below / above case has its on-the-limit twin (the guard-plus-window cases, named after the carrying pair, are held to the walk of the ladder instead)
    for c in V.GUARD_CASES:
        if c.value in ("below_lo", "above_hi") and c.rerun and "_p0-" not in c.name and "_p1-" not in c.name:
            twin = c.name.rsplit("-", 1)[0] + ("-lo" if c.value == "below_lo" else "-hi")
            assert twin in names, c.name
    wheres = {c.where for c in V.GUARD_CASES if c.value}
    assert {"first_tile", "last_ref_col", "last_query_row", "gap_letter", "mid", "near_end"} <= wheres
    assert any(c.marker == 128 and c.where == "mid" for c in V.GUARD_CASES)
    assert {c.value for c in V.GUARD_CASES} == {"below_lo", "lo", "hi", "above_hi", None}
    # the denominators: accepted on 2^40, refused on a float above it and on the very next one; 2^40 - 1 as integers is covered by the score cases
    assert V.denom_ok((V.BIG, V.BIG)) and not V.denom_ok((V.BIG + 1, V.BIG)) and float(V.denom_of((V.BIG + 1, V.BIG))) == 2.0 ** 40 + 2.0 ** 20
    assert not V.denom_ok(V.NEXT_ABOVE) and V.denom_of(V.NEXT_ABOVE) == np.nextafter(F(2.0 ** 40), F(np.inf)) and max(V.NEXT_ABOVE) < 2 ** 31
    assert all(dict(c.nums)[6] == V.NEXT_ABOVE for c in V.GUARD_CASES if c.name.endswith("denom-above_2p40"))
    assert {"nuc32_over", "nuc72_margin", "prot16_over"} <= {c.pool for c in V.GUARD_CASES}
