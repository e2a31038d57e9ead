"""twl_store_trim_columns / twl_store_trim_read (include/twl_trim.h; trim_kernels.hip.h, twl_trim.inc.hip) through the binding, on stores
built from host rows, against tests/trim_oracle.py, exactly: rows, kept, the kept-column list and the gap counts, where the kernels
switch (tests/trim_cases.py on the constants of twl_trim_describe), on both row planes, with unlisted rows, and with everything the call
refuses."""
import numpy as np
import pytest

import level_cases as LC
import trim_cases as TC
import trim_oracle as TO

pytestmark = pytest.mark.gpu
F32 = np.float32
GAP = TO.GAP


@pytest.fixture(scope="module")
def consts(gpu):
    from twilight_amd import trim

    T, R, C, F = trim.describe()
    assert T % 32 == 0 and C % 32 == 0 and T >= 64 and 4 < F < R
    return T, R, C, F


def _trim_and_compare(st, rows, ids, rule, arg_index, what=""):
    """rows: current rows by store id; ids: the listed ids; arg_index: the gap limit, or the position in ids of the reference row."""
    from twilight_amd import trim

    listed = [rows[i] for i in ids]
    W = len(listed[0])
    mask, want = TO.agree(listed, rule, arg_index)
    kept = trim.trim_columns(st, ids, rule, ids[arg_index] if rule == TO.TO_ROW else arg_index)
    assert kept == int(mask.sum()), what
    got = st.rows_of(ids)
    for i, g, w in zip(ids, got, want):
        assert g == w, f"{what}: row {i}"
    cols, gaps = trim.trim_read(st, W, kept)
    assert np.array_equal(cols, TO.kept_columns(mask)), what
    assert np.array_equal(gaps, TO.gap_counts(listed)), what
    assert trim.trim_ms(st) > 0
    return want


def _run_cases(cases):
    from twilight_amd import level

    for c in cases:
        st = level.Store(c.rows, "n")
        try:
            _trim_and_compare(st, c.rows, list(range(len(c.rows))), c.rule, c.arg, f"{c.name} ({c.branch})")
        finally:
            st.close()


def test_widths(gpu, consts):
    """W = 1; one below, on and one above a thread's 16 columns, a keep word, a column tile and a scan round."""
    T, R, C, F = consts
    _run_cases(TC.width_cases(T, C))


def test_row_counts(gpu, consts):
    """Row counts around the flush period of the packed byte counters and around the counts kernel's row slice, with an all-gap column."""
    T, R, C, F = consts
    cases = TC.row_count_cases(R, F)
    assert {len(c.rows) for c in cases} >= {1, F - 1, F, F + 1, R - 1, R, R + 1}
    _run_cases(cases)


def test_contents(gpu, consts):
    """The limit between two columns, max_gaps = 0 and = n, kept = 0 and = W, kept runs inside words, three scan rounds with the only kept
    column in the last word, '.', lower case and bytes >= 0x80, both ends of TWL_TRIM_TO_ROW."""
    T, R, C, F = consts
    cases = TC.content_cases(T, C)
    names = {c.name for c in cases}
    for must in ("limit 4 between columns of 4 and 5 gaps", "max_gaps = 0", "max_gaps = n", "kept = 0", "kept = W, no gap at all", "kept runs inside words",
                 "three scan rounds, one kept column in the last word", "'.' and lower case", "to the first row", "to the last row", "to an all-gap row"):
        assert must in names
    _run_cases(cases)


def test_rows_without_columns(gpu, consts):
    from twilight_amd import level, trim

    st = level.Store([b"", b"", b"ACGT"], "n")
    try:
        assert trim.trim_columns(st, [0, 1], TO.MAX_GAPS, 0) == 0
        cols, gaps = trim.trim_read(st, 0, 0)
        assert cols.size == 0 and gaps.size == 0
        assert st.rows() == [b"", b"", b"ACGT"]
    finally:
        st.close()


def _move_to_the_other_plane(st, ids):
    """A squeeze over a group without an all-gap column rewrites its rows into their other plane at the same length."""
    from twilight_amd import backbone

    L = len(st.rows_of(ids[:1])[0])
    assert backbone.squeeze_groups(st, [ids]) == [L]


def _two_plane_store(rng, T, n, W, plane_of, extra):
    """A store whose row i lies on plane plane_of(i) and holds live[i]; the other plane of every row holds a copy that differs at every
    column and has no gap.  extra: further rows of other lengths behind them, never listed."""
    from twilight_amd import level

    live = [r for r in TC._rows(TC.random_rows(rng, n, W, p_gap=0.5))]
    stale = [bytes((b ^ 0x55) if b != GAP else ord("N") for b in row) for row in live]
    st = level.Store(stale + extra, "n")
    everyone = list(range(n))
    _move_to_the_other_plane(st, everyone)
    back = [i for i in everyone if plane_of(i) == 0]
    if back:
        _move_to_the_other_plane(st, back)
    st.write_rows(everyone, live)
    assert st.rows_of(everyone) == live
    return st, live


def test_rows_on_both_planes(gpu, consts):
    """Rows alternating between the planes row by row, so that a group of four rows of the counts loop mixes them; ids listed in descending
    order; TWL_TRIM_TO_ROW with the reference row on the other plane than its neighbours."""
    T, R, C, F = consts
    rng = np.random.default_rng(11)
    n, W = 2 * F + 3, T + 33
    for rule, arg_index, plane_of in ((TO.MAX_GAPS, n // 2, lambda i: i % 2), (TO.TO_ROW, 0, lambda i: 1 if i == n - 1 else 0), (TO.TO_ROW, 4, lambda i: 0 if i == n - 5 else 1)):
        st, live = _two_plane_store(rng, T, n, W, plane_of, [])
        try:
            ids = list(range(n - 1, -1, -1))
            _trim_and_compare(st, live, ids, rule, arg_index, f"rule {rule}")
        finally:
            st.close()


def test_unlisted_rows_between_listed_ones_and_a_second_trim(gpu, consts):
    """Every third row of the store is listed nowhere (other lengths, every second of them on plane 1): untouched.  Then the trimmed rows are trimmed again, by
    the other rule and by the same limit: the second call sees the rows the first one left."""
    from twilight_amd import level

    T, R, C, F = consts
    rng = np.random.default_rng(12)
    n_store, W = 31, T + 200
    rows = {}
    for i in range(n_store):
        rows[i] = TC._rows(TC.random_rows(rng, 1, 40 + i if i % 3 == 2 else W, p_gap=0.0 if i % 6 == 5 else 0.45))[0]
    seqs = [rows[i] for i in range(n_store)]
    listed = [i for i in range(n_store) if i % 3 != 2]
    unlisted = [i for i in range(n_store) if i % 3 == 2]
    st = level.Store(seqs, "n")
    try:
        for i in unlisted:
            if i % 6 == 5:
                _move_to_the_other_plane(st, [i])      # (a row without a gap: the squeeze keeps its length)
        assert st.rows() == seqs
        after = _trim_and_compare(st, seqs, listed, TO.MAX_GAPS, len(listed) // 2, "first trim")
        assert st.rows_of(unlisted) == [seqs[i] for i in unlisted], "rows outside the call"
        now = dict(zip(listed, after))
        assert 0 < len(after[0]) < W
        after2 = _trim_and_compare(st, now, listed, TO.TO_ROW, 3, "second trim, to a row")
        now = dict(zip(listed, after2))
        after3 = _trim_and_compare(st, now, listed[::-1], TO.MAX_GAPS, len(listed) // 2 - 2, "third trim")
        assert len(after3[0]) <= len(after2[0]) <= len(after[0])
        assert st.rows_of(unlisted) == [seqs[i] for i in unlisted], "rows outside the calls"
    finally:
        st.close()


def test_refusals_change_nothing(gpu, consts):
    import twilight_amd as twl
    from twilight_amd import level, trim

    rng = np.random.default_rng(5)
    seqs = TC._rows(TC.random_rows(rng, 4, 50)) + TC._rows(TC.random_rows(rng, 3, 70)) + [b"AC-GT"]
    st = level.Store(seqs, "n")
    try:
        with pytest.raises(twl.TwlError, match="no twl_store_trim_columns has run"):
            trim.trim_read_raw(st, cols=True, gaps=True)
        bad = [("a null store", (None, 2, [0, 1], 0, 1, True), "bad argument"),
               ("a null id table", (st, 2, None, 0, 1, True), "bad argument"),
               ("a null output", (st, 2, [0, 1], 0, 1, False), "bad argument"),
               ("no rows", (st, 0, [0], 0, 0, True), "no rows listed"),
               ("a negative count", (st, -1, [0], 0, 0, True), "no rows listed"),
               ("an id outside the store", (st, 2, [0, len(seqs)], 0, 1, True), "out of range"),
               ("a negative id", (st, 2, [-1, 0], 0, 1, True), "out of range"),
               ("an id twice", (st, 3, [0, 1, 0], 0, 1, True), "listed twice"),
               ("two lengths", (st, 2, [3, 4], 0, 1, True), "differ in length"),
               ("an unknown rule", (st, 2, [0, 1], 2, 1, True), "unknown trim rule"),
               ("a negative rule", (st, 2, [0, 1], -1, 1, True), "unknown trim rule"),
               ("a negative gap limit", (st, 2, [0, 1], 0, -1, True), "gap limit"),
               ("a gap limit above n_ids", (st, 2, [0, 1], 0, 3, True), "gap limit"),
               ("a reference row outside ids", (st, 2, [0, 1], 1, 2, True), "not among the listed rows"),
               ("a reference row outside the store", (st, 2, [0, 1], 1, 99, True), "not among the listed rows")]
        for what, (store, n, ids, rule, arg, out), text in bad:
            with pytest.raises(twl.TwlError, match=text):
                trim.trim_columns_raw(store, n, ids, rule, arg, out)
            assert st.rows() == seqs, what
        with pytest.raises(twl.TwlError, match="no twl_store_trim_columns has run"):
            trim.trim_read_raw(st)
        with pytest.raises(twl.TwlError, match="bad argument"):
            trim.trim_read_raw(None)
        # a level that is still prepared
        one = np.asarray([1.0], dtype=F32)
        p = twl.make_params(LC.matrix_of("n"))
        st.prepare(p, [[level.Side([7], one, 5, 1, 1.0), level.Side([0], one, 50, 1, 1.0)]])
        with pytest.raises(twl.TwlError, match="still prepared"):
            trim.trim_columns(st, [0, 1, 2, 3], TO.MAX_GAPS, 1)
        st.commit([np.zeros(0, dtype=np.int8)])
        assert st.rows() == seqs
        # then the call goes through, and a read with null tables is no error
        _trim_and_compare(st, seqs, [6, 5, 4], TO.MAX_GAPS, 1, "after the refusals")
        trim.trim_read_raw(st)
        assert st.rows_of([0, 1, 2, 3, 7]) == seqs[:4] + seqs[7:]
    finally:
        st.close()
