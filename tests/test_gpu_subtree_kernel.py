"""twl_store_weighted_columns (include/twl_subtree.h, subtree_kernels.hip.h) on the MI355X against the sequential fp32 loop of
tests/subtree_cases.py, bit for bit through twl_store_read_cache: no tolerance anywhere, the order of the additions is the contract.

The kernel gives a workgroup 256 columns (one thread each) and stages the rows 256 at a time, so the shapes sit on both sides of one and
two column tiles (L = 1, 255, 256, 257, 513) and of one staging round (n = 255, 256, 257; 300 = one full round and a partial one), next to
n = 1, 2 and 65.  tests/test_subtree_oracle_cpu.py proves that summing these rows in reversed order changes the result, so a kernel that adds
in another order cannot pass here."""
import numpy as np
import pytest

import subtree_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["n", "p"])
def family(gpu, request):
    """One store per sequence type: rows of all five lengths interleaved; of every length's rows a half has been moved to the store's other
    plane (a one-group merge's finish rewrites rows there, at their own width), and a half (across both planes) has been rewritten with
    twl_store_write_rows."""
    from twilight_amd import level, merge

    seq_type = request.param
    rows = SC.store_rows(seq_type)
    st = level.Store(rows, seq_type)
    for L in SC.COLUMNS:
        moved = [i for j, i in enumerate(SC.class_ids(L)) if j % 4 >= 2]
        mg = merge.Merge(st, [moved])
        assert mg.finish() == L
        mg.close()
    new = SC.rewritten_rows(seq_type, rows)
    st.write_rows(list(new), [new[i] for i in new])
    rows = [new.get(i, r) for i, r in enumerate(rows)]
    assert st.rows_of(list(range(len(rows)))) == rows
    yield seq_type, st, rows
    st.close()


@pytest.mark.parametrize("L", SC.COLUMNS)
def test_weighted_columns_bit_for_bit(family, L):
    from twilight_amd import subtree

    seq_type, st, rows = family
    for n in SC.ROWS:
        ids, w = SC.case(seq_type, L, n)
        assert len(set(ids)) == n and (n < 3 or ids != sorted(ids))
        cache_id = 1000 * SC.COLUMNS.index(L) + n
        subtree.weighted_columns(st, ids, w, cache_id)
        want = SC.weighted_profile([rows[i] for i in ids], w, seq_type)
        got = st.cache(cache_id)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"L {L}, n {n}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} cells differ"
        if L > SC.SAME_LETTER_COLUMN:
            assert np.count_nonzero(got[SC.SAME_LETTER_COLUMN]) == 1 and got[SC.SAME_LETTER_COLUMN, 0] > 0      # one letter throughout: one chain over all rows


def test_the_profile_is_a_side_of_a_level(family):
    """The cached profile is what twl_store_write_cache would have stored: reading it back, writing it under another id and reading that
    gives the same bits (the contract of twl_store_count_columns: a cache id the level API takes)."""
    from twilight_amd import subtree

    seq_type, st, rows = family
    ids, w = SC.case(seq_type, 257, 65)
    subtree.weighted_columns(st, ids, w, 7001)
    st.write_cache(7002, st.cache(7001))
    assert np.array_equal(st.cache(7001).view(np.uint32), st.cache(7002).view(np.uint32))


def test_refusals_on_the_device_build(family):
    """Every refusal returns its status with its message and leaves the store usable."""
    import twilight_amd as twl
    from twilight_amd import subtree

    seq_type, st, rows = family
    a, b = SC.class_ids(255)[:2]
    other = SC.class_ids(256)[0]
    ok_w = np.array([0.25, 0.7], dtype=np.float32)
    subtree.weighted_columns(st, [a, b], ok_w, 9000)
    refused = [
        (([], np.zeros(0, np.float32), 9001), "bad argument"),
        (([a, len(rows)], ok_w, 9001), "sequence id out of range"),
        (([-1, a], ok_w, 9001), "sequence id out of range"),
        (([a, a], ok_w, 9001), "sequence id given twice"),
        (([a, other], ok_w, 9001), "the rows of the profile differ in length"),
        (([a, b], ok_w, 9000), "cache id in use"),
        (([a, b], ok_w, -1), "bad argument"),
    ]
    for (ids, w, cid), message in refused:
        with pytest.raises(twl.TwlError, match=message):
            subtree.weighted_columns(st, ids, w, cid)
    import ctypes as C

    lib = twl.load_library()
    lib.twl_store_weighted_columns.restype = C.c_int
    idv = np.array([a, b], dtype=np.int32)
    p_ids, p_w = idv.ctypes.data_as(C.POINTER(C.c_int32)), ok_w.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, C.c_int32(2), p_ids, p_w), (st._h, C.c_int32(2), None, p_w), (st._h, C.c_int32(2), p_ids, None)):
        assert lib.twl_store_weighted_columns(*args, C.c_int32(9001)) != 0
        assert b"bad argument" in lib.twl_last_error()
    # rows without columns: a store of its own
    from twilight_amd import level

    empty = level.Store([b"", b""], seq_type)
    with pytest.raises(twl.TwlError, match="the rows of the profile are empty"):
        subtree.weighted_columns(empty, [0, 1], ok_w, 0)
    empty.close()
    # the store is as usable as before: the next profile is right, and none of the refused ids exists
    subtree.weighted_columns(st, [b, a], ok_w, 9001)
    assert np.array_equal(st.cache(9001).view(np.uint32), SC.weighted_profile([rows[b], rows[a]], ok_w, seq_type).view(np.uint32))
