"""twl_retree_set_create, _letters and _assign on the MI355X against the assignment rule restated in exact integers
(tests/retree_stage_oracle.py): the seed every row goes to and its two counts with it.  Sizes on every edge of the 64-row tile of rows and
of the 64-seed tile, widths on every edge of the 64-column word and of the 512-column staged slice, both ends of the mask, a mask that
removes the deciding column, seeds out of order, equal ratios wherever two candidates of a row meet (two columns of one thread, two lanes
of a row, two seed tiles), rows and seeds without letters, a near tie that single precision cannot order, protein rows, calls without the
counts, and a set of more rows than one launch of the pack kernel takes."""
import ctypes as C

import numpy as np
import pytest

import retree_oracle as R
import retree_stage_cases as cases
import retree_stage_oracle as RS
from guide_stage_oracle import seed_ids

pytestmark = pytest.mark.gpu

_REF = {}


def _family(type_, n, width, lower=0.0):
    """The family of n rows of this width as a list of bytes; made once per shape and shared, never changed."""
    key = (type_, n, width, lower)
    if key not in _REF:
        _REF[key] = cases.as_bytes(cases.family(type_, n, width, 700 + 3 * n + width, lower))
    return _REF[key]


def _check(rows, type_, mg, seeds, want_counts=True):
    from twilight_amd import retree_set

    want_seed, want_m, want_b = RS.assign(rows, type_, mg, seeds)
    code = RS.codes(rows, type_, mg)
    with retree_set.RetreeSet(rows, type_, mg) as rs:
        assert rs.kept == code.shape[1]
        assert (rs.letters() == (code >= 0).sum(axis=1)).all()
        got_seed, got_m, got_b = rs.assign(seeds, want_counts=want_counts)
        upload, gaps, pack, assign, groups, download = rs.timing()
    assert upload > 0 and gaps > 0 and pack > 0 and assign > 0 and download > 0 and groups == 0
    bad = np.flatnonzero(got_seed != want_seed)
    assert len(bad) == 0, (len(rows), len(seeds), bad[:5], got_seed[bad[:5]], want_seed[bad[:5]])
    if want_counts:
        assert (got_m == want_m).all() and (got_b == want_b).all()
    else:
        assert got_m is None and got_b is None
    for t, i in enumerate(seeds):
        assert got_seed[i] == t      # a seed belongs to its own cluster
    return got_seed


@pytest.mark.parametrize("n,s", [(n, s) for n in (63, 64, 65, 130) for s in (2, 63, 64, 65, 129) if s <= n])
def test_sizes_on_every_edge_of_both_tiles(gpu, n, s):
    """N one below, on and one above the tile of rows and two tiles plus two; S = 2, one below, on and one above the tile of seeds, two tiles
    plus one.  The seeds are those of the stride rule; the mask is the default's."""
    rows = _family("n", n, 200)
    got = _check(rows, "n", R.max_gaps(0.95, n), seed_ids(n, s))
    assert len(set(got.tolist())) > 1


@pytest.mark.parametrize("width", [1, 63, 64, 65, 511, 512, 513, 1025])
def test_widths_on_every_edge_of_the_word_and_the_slice(gpu, width):
    rows = _family("n", 65, width)
    _check(rows, "n", R.max_gaps(0.95, 65), seed_ids(65, 7))


@pytest.mark.parametrize("mg", [0, 65])
def test_both_ends_of_the_mask(gpu, mg):
    """max_gaps = 0 keeps only the columns without a gap, max_gaps = n keeps every column."""
    rows = _family("n", 65, 130)
    kept = int(R.kept_columns(rows, mg).sum())
    assert (0 < kept < 130) if mg == 0 else kept == 130
    _check(rows, "n", mg, seed_ids(65, 7))


def test_a_mask_that_removes_the_deciding_column(gpu):
    rows, seeds, i, gaps_there = cases.deciding_column_rows()
    assert R.column_gaps(rows).tolist() == [0] * 20 + [gaps_there]
    got = _check(rows, "n", gaps_there, seeds)
    assert got[i] == 1
    got = _check(rows, "n", gaps_there - 1, seeds)
    assert got[i] == 0


def test_seeds_out_of_order(gpu):
    """seed_ids in a shuffled order: t is the position in the list, not the id."""
    rows = _family("n", 130, 200)
    seeds = [int(x) for x in np.random.default_rng(5).permutation(130)[:70]]
    assert seeds != sorted(seeds)
    _check(rows, "n", R.max_gaps(0.95, 130), seeds)


@pytest.mark.parametrize("ta,tb", [(3, 19), (3, 4), (3, 67)])
def test_equal_ratios_go_to_the_smaller_t(gpu, ta, tb):
    """Columns t and t + 16 belong to one thread, t and t + 1 to two lanes of a row, t and t + 64 to two seed tiles."""
    rows, seeds = cases.twin_seed_rows(ta, tb, 1000 + 100 * ta + tb)
    got = _check(rows, "n", len(rows), seeds)
    assert got[128] == ta and got[0] == tb
    assert (got[129:] == ta).all(), got[129:]


def test_rows_and_seeds_without_letters(gpu):
    """No letter in a kept column: the ratio is 0 / 1 with every seed, so such a row lands on seed 0 with counts 0, 0; a seed without letters
    keeps itself."""
    rows = list(_family("n", 65, 130))
    rows[10], rows[20], rows[64] = b"-" * 130, b"N" * 130, b"." * 130
    got = _check(rows, "n", 65, [5, 20, 40, 64, 63])      # 20 and 64 are seeds without letters
    assert got[10] == 0 and got[20] == 1 and got[64] == 3
    got = _check(rows, "n", 65, [20, 5, 40])               # a seed without letters first: everything at ratio 0 with all seeds goes to it
    assert got[10] == 0 and got[64] == 0
    # ... and a row whose only letters stand in a column the mask drops
    rows, seeds, i, gaps_there = cases.deciding_column_rows()
    rows = rows + [b"-" * 20 + b"A"]
    got = _check(rows, "n", gaps_there - 1, [1, 0])
    assert got[len(rows) - 1] == 0


def test_a_near_tie_that_single_precision_cannot_order(gpu):
    """8191 / 8192 at t = 0 against 8192 / 8193 at t = 1: the larger t is closer by a quarter of an fp32 ulp."""
    rows, seeds, i = cases.near_tie_rows()
    got = _check(rows, "n", len(rows), seeds)
    assert got[i] == 1
    got = _check(rows, "n", len(rows), seeds[::-1])
    assert got[i] == 0


def test_protein_rows(gpu):
    """6 planes, letters of either case, X, B, Z and * as no letter."""
    rows = _family("p", 130, 200, lower=0.3)
    text = b"".join(rows)
    assert all(ch in text for ch in b"XBZ*") and any(ch in text for ch in b"acdefghiklmnpqrstvwy")
    got = _check(rows, "p", R.max_gaps(0.95, 130), seed_ids(130, 65))
    assert len(set(got.tolist())) > 1


def test_without_the_counts(gpu):
    rows = _family("n", 65, 130)
    _check(rows, "n", R.max_gaps(0.95, 65), seed_ids(65, 9), want_counts=False)
    from twilight_amd import retree_set

    seeds = np.asarray(seed_ids(65, 9), dtype=np.int32)
    want_seed, want_m, want_b = RS.assign(rows, "n", 61, seeds)
    with retree_set.RetreeSet(rows, "n", 61) as rs:      # one of the two alone
        lib, p = rs._lib, lambda a: a.ctypes.data_as(C.c_void_p)
        for which in (0, 1):
            seed, counts = np.full(66, -7, dtype=np.int32), np.full(66, 0xFFFFFFFF, dtype=np.uint32)
            args = (None, p(counts)) if which else (p(counts), None)
            assert lib.twl_retree_set_assign(rs._h, 9, p(seeds), p(seed), *args) == 0
            assert (seed[:65] == want_seed).all() and seed[65] == -7 and counts[65] == 0xFFFFFFFF
            assert (counts[:65] == (want_b if which else want_m)).all()


def test_more_rows_than_one_pack_launch(gpu):
    """65 600 rows of 70 columns, 3 seeds: the pack kernel is launched over two slabs of rows, and letters() reaches past row 65 535."""
    from twilight_amd import retree_set

    n = 65600
    a = cases.family("n", n, 70, 4242)
    assert n > retree_set.describe()["pack_rows"]
    mg = R.max_gaps(0.95, n)
    seeds = seed_ids(n, 3)
    want_seed, want_m, want_b = RS.assign(a, "n", mg, seeds)
    code = RS.codes(a, "n", mg)
    with retree_set.RetreeSet(a, "n", mg) as rs:
        assert rs.kept == code.shape[1] < 70      # (the mask drops some of the gappy columns)
        letters = rs.letters()
        got_seed, got_m, got_b = rs.assign(seeds)
    assert (letters == (code >= 0).sum(axis=1)).all() and letters[65535:].any()
    assert (got_seed == want_seed).all() and (got_m == want_m).all() and (got_b == want_b).all()
    assert len(set(got_seed[65535:].tolist())) > 1
