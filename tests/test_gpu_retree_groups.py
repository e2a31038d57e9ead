"""twl_retree_set_pair_groups on the MI355X against the pair counts of the numpy restatement (tests/retree_stage_oracle.py), exactly: groups
on every edge of the 64 x 64 tile in one call, rows gathered through ids in any order, a row in two groups, one group of all rows against
twl_retree_pair_counts, and protein rows.  Every call has a guard band behind both outputs."""
import numpy as np
import pytest

import retree_oracle as R
import retree_stage_cases as cases
import retree_stage_oracle as RS

pytestmark = pytest.mark.gpu

GUARD = 256
_REF = {}


def _reference(type_, n, width, T=0.95, lower=0.0):
    """(rows, max_gaps, codes of the kept columns) of a family; made once per shape and shared, never changed."""
    key = (type_, n, width, T, lower)
    if key not in _REF:
        rows = cases.as_bytes(cases.family(type_, n, width, 900 + n + width, lower))
        mg = R.max_gaps(T, n)
        code = RS.codes(rows, type_, mg)
        code.setflags(write=False)
        _REF[key] = (rows, mg, code)
    return _REF[key]


def _blocks(flat, groups):
    assert (flat[len(flat) - GUARD:] == 0xFFFFFFFF).all(), "the call wrote behind its output"
    at, out = 0, []
    for g in groups:
        out.append(flat[at: at + len(g) ** 2].reshape(len(g), len(g)))
        at += len(g) ** 2
    assert at == len(flat) - GUARD
    return out


def _compare(match, both, code, letters, groups):
    for g, m, b in zip(groups, _blocks(match, groups), _blocks(both, groups)):
        want_m, want_b = RS.pair_counts(code[np.asarray(g)])
        assert (m == want_m).all(), (len(g), np.argwhere(m != want_m)[:5])
        assert (b == want_b).all(), (len(g), np.argwhere(b != want_b)[:5])
        assert (m == m.T).all() and (b == b.T).all()
        assert (np.diag(m) == letters[np.asarray(g)]).all() and (np.diag(b) == letters[np.asarray(g)]).all()


def test_groups_on_every_edge_of_the_tile_in_one_call(gpu):
    """Sizes 65, 1, 130, 2, 64, 63 in this order over a set of 200 rows of 600 columns (two staged slices); the ids are a shuffle, a
    descending run, every third row ... and some rows serve two groups."""
    from twilight_amd import retree_set

    rows, mg, code = _reference("n", 200, 600)
    rng = np.random.default_rng(3)
    groups = [[int(x) for x in rng.permutation(200)[:65]], [199], list(range(199, 69, -1)), [150, 7], list(range(0, 192, 3)), [int(x) for x in rng.permutation(200)[:63]]]
    assert [len(g) for g in groups] == [65, 1, 130, 2, 64, 63]
    assert 150 in groups[2] and 150 in groups[3] and 150 in groups[4]      # a row in several groups
    with retree_set.RetreeSet(rows, "n", mg) as rs:
        assert rs.kept == code.shape[1] < 600
        letters = rs.letters()
        match, both = rs.pair_groups(groups, guard_words=GUARD)
        upload, gaps, pack, assign, groups_ms, download = rs.timing()
    assert (letters == (code >= 0).sum(axis=1)).all()
    _compare(match, both, code, letters, groups)
    assert upload > 0 and gaps > 0 and pack > 0 and groups_ms > 0 and download > 0 and assign == 0


def test_a_row_twice_in_one_group(gpu):
    """The same row at two places of one group: the two places hold the row's letters off the diagonal too."""
    from twilight_amd import retree_set

    rows, mg, code = _reference("n", 200, 600)
    groups = [[5, 9, 5, 70], [9]]
    with retree_set.RetreeSet(rows, "n", mg) as rs:
        letters = rs.letters()
        match, both = rs.pair_groups(groups, guard_words=GUARD)
    _compare(match, both, code, letters, groups)
    assert match[0 * 4 + 2] == both[2 * 4 + 0] == letters[5]


def test_300_groups_of_one_member(gpu):
    from twilight_amd import retree_set

    rows, mg, code = _reference("n", 200, 600)
    groups = [[(7 * g) % 200] for g in range(300)]
    with retree_set.RetreeSet(rows, "n", mg) as rs:
        match, both = rs.pair_groups(groups, guard_words=GUARD)
        letters = rs.letters()
    for flat in (match, both):
        assert (flat[300:] == 0xFFFFFFFF).all()
        assert (flat[:300] == letters[[g[0] for g in groups]]).all()


@pytest.mark.parametrize("T", [0.95, 0.5])
def test_one_group_of_all_rows_is_twl_retree_pair_counts(gpu, T):
    from twilight_amd import retree, retree_set

    rows, mg, code = _reference("n", 130, 600, T)
    everyone = [list(range(130))]
    with retree_set.RetreeSet(rows, "n", mg) as rs:
        kept = rs.kept
        match, both = rs.pair_groups(everyone, guard_words=GUARD)
    (m,), (b,) = _blocks(match, everyone), _blocks(both, everyone)
    one_m, one_b, one_kept = retree.pair_counts(rows, "n", mg)
    assert kept == one_kept == code.shape[1]
    assert (m == one_m).all() and (b == one_b).all()
    want_m, want_b = RS.pair_counts(code)
    assert (m == want_m).all() and (b == want_b).all()
    want_m, want_b, _ = R.pair_counts(rows, "n", mg)
    assert (m == want_m).all() and (b == want_b).all()


def test_protein_groups(gpu):
    """6 planes, letters of either case: a tile and a partial one, and a group of 3."""
    from twilight_amd import retree_set

    rows, mg, code = _reference("p", 65, 130, lower=0.3)
    groups = [list(range(64, -1, -1)), [3, 60, 9]]
    with retree_set.RetreeSet(rows, "p", mg) as rs:
        letters = rs.letters()
        match, both = rs.pair_groups(groups, guard_words=GUARD)
    _compare(match, both, code, letters, groups)
