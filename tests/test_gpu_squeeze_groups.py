"""twl_store_squeeze_groups (include/twl_backbone.h; backbone_kernels.hip.h, twl_backbone.inc.hip) against squeeze_group of
tests/place_tree_oracle.py, byte for byte, where its kernels switch: around the column tile T, the row slice R and the scan chunk C
(taken from twl_squeeze_describe), on both row planes, and with everything the call refuses."""
import numpy as np
import pytest

import level_cases as LC
import level_oracle as LO
import oracle_lib as O
import place_tree_oracle as PO

pytestmark = pytest.mark.gpu
F = np.float32
GAP = 0x2D


@pytest.fixture(scope="module")
def consts(gpu):
    from twilight_amd import backbone

    T, R, C = backbone.describe()
    assert T % 32 == 0 and C % 32 == 0 and T >= 64 and R >= 3
    return T, R, C


def _random_group(rng, n, L, p_gap_col=0.3, p_gap=0.4):
    """n rows of L bytes: a column is all '-' with probability p_gap_col, otherwise letters with single gaps; at least one kept column's rows vary."""
    if L == 0:
        return [b""] * n
    block = rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), size=(n, L))
    block[rng.random((n, L)) < p_gap] = GAP
    block[:, rng.random(L) < p_gap_col] = GAP
    return [block[k].tobytes() for k in range(n)]


def _squeeze_and_compare(st, seqs, groups, untouched=()):
    from twilight_amd import backbone

    want = {}
    lens = []
    for g in groups:
        sq = PO.squeeze_group([seqs[i] for i in g])
        lens.append(len(sq[0]))
        want.update(zip(g, sq))
    got_len = backbone.squeeze_groups(st, groups)
    assert got_len == lens
    flat = [i for g in groups for i in g]
    got = st.rows_of(flat)
    for i, row in zip(flat, got):
        assert row == want[i], f"row {i} (group of {[len(g) for g in groups if i in g][0]} rows, length {len(seqs[i])})"
    if untouched:
        assert st.rows_of(list(untouched)) == [seqs[i] for i in untouched], "rows outside the call"
    assert backbone.squeeze_ms(st) > 0 or not flat


def test_lengths_and_row_counts(gpu, consts):
    """Every length around the column tile and the scan chunk with every row count around the row slice, all groups in one call."""
    from twilight_amd import level

    T, R, C = consts
    rng = np.random.default_rng(20261020)
    seqs, groups = [], []
    for L in (0, 1, T - 1, T, T + 1, 2 * T + 1, C - 1, C, C + 1):
        for n in (1, 2, R - 1, R, R + 1, 2 * R + 1):
            groups.append(list(range(len(seqs), len(seqs) + n)))
            seqs.extend(_random_group(rng, n, L))
    st = level.Store(seqs, "n")
    try:
        _squeeze_and_compare(st, seqs, groups)
    finally:
        st.close()


def _content_groups(T, R, C):
    """Named groups of 2R + 1 rows and C + T / 2 + 5 columns (two tiles and a part, one scan chunk and a part)."""
    rng = np.random.default_rng(7)
    n, L = 2 * R + 1, C + T // 2 + 5
    base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, L))
    out = {}
    out["every column all-gap"] = np.full((n, L), GAP, dtype=np.uint8)
    out["no gap at all"] = base.copy()
    for who, r in (("the last row of a slice", R - 1), ("the first row of the next slice", R), ("the last row of the group", 2 * R)):
        b = np.full((n, L), GAP, dtype=np.uint8)
        cols = np.arange(3, L, 7)
        b[r, cols] = ord("A")                       # a column that is '-' in every row but one
        out["one letter per kept column, in " + who] = b
    b = base.copy()
    for edge in (T, 2 * T, C):
        b[:, edge - 3: edge + 3] = GAP              # a dropped run across a tile edge / the scan chunk
    b[:, T + 16 - 1: T + 16 + 1] = GAP              # ... across two threads' 16 columns
    b[:, 31: 33] = GAP                              # ... across two words
    out["dropped runs across tile edges, the scan chunk, a thread and a word"] = b
    b = base.copy()
    b[:, 0] = GAP
    b[:, L - 1] = GAP
    out["first and last column dropped"] = b
    b = base.copy()
    b[:, 5: L: 11] = ord(".")
    b[:, 6: L: 11] = GAP
    out["columns of '.' stay, columns of '-' go"] = b
    b = rng.choice(np.frombuffer(b"acgtn", dtype=np.uint8), size=(n, L))
    b[:, 2: L: 5] = GAP
    out["lower case"] = b
    b = rng.integers(0x80, 0x100, size=(n, L)).astype(np.uint8)
    b[:, 1: L: 3] = GAP
    b[0, 1] = 0xAD                                   # ('-' with its top bit set is a letter)
    out["bytes >= 0x80"] = b
    return {k: [v[i].tobytes() for i in range(n)] for k, v in out.items()}


def test_contents(gpu, consts):
    from twilight_amd import level

    T, R, C = consts
    named = _content_groups(T, R, C)
    seqs, groups = [], []
    for rows in named.values():
        groups.append(list(range(len(seqs), len(seqs) + len(rows))))
        seqs.extend(rows)
    st = level.Store(seqs, "n")
    try:
        from twilight_amd import backbone

        want_len = [len(PO.squeeze_group(rows)[0]) for rows in named.values()]
        assert want_len[0] == 0 and want_len[1] == C + T // 2 + 5
        got_len = backbone.squeeze_groups(st, groups)
        for (name, rows), g, w, n in zip(named.items(), groups, want_len, got_len):
            assert n == w, name
            assert st.rows_of(g) == PO.squeeze_group(rows), name
    finally:
        st.close()


def test_mixed_groups_interleaved_ids_and_unlisted_rows(gpu, consts):
    """One call: a one-row group, a zero-length group, a 2R + 1-row group and groups of different lengths; the ids of the groups are
    interleaved in the store and listed in descending order; every fourth row of the store is listed nowhere."""
    from twilight_amd import level

    T, R, C = consts
    rng = np.random.default_rng(3)
    shapes = [(1, T + 7), (2, 0), (2 * R + 1, 2 * T + 1), (3, 17), (R, 1), (5, 300)]
    total = sum(n for n, _ in shapes)
    slots = [i for i in range(2 * total) if i % 4 != 3]      # the ids the groups take; i % 4 == 3 stays unlisted
    order = rng.permutation(len(slots))[:total]
    seqs = {}
    groups, at = [], 0
    for n, L in shapes:
        ids = sorted((slots[k] for k in order[at: at + n]), reverse=True)
        at += n
        for i, row in zip(ids, _random_group(rng, n, L)):
            seqs[i] = row
        groups.append(ids)
    n_store = max(seqs) + 2
    untouched = [i for i in range(n_store) if i not in seqs]
    for i in untouched:
        seqs[i] = _random_group(rng, 1, 40 + i, p_gap_col=0.5)[0]
    seqs = [seqs[i] for i in range(n_store)]
    st = level.Store(seqs, "n")
    try:
        _squeeze_and_compare(st, seqs, groups, untouched)
        # a second squeeze of the same groups finds nothing more to drop
        after = st.rows()
        _squeeze_and_compare(st, after, groups, untouched)
    finally:
        st.close()


def _move_to_the_other_plane(st, ids, rows):
    """A fresh merge of one group rewrites its rows into their other plane when it finishes, at their own width (one call per length)."""
    from twilight_amd import merge

    for L in sorted({len(rows[i]) for i in ids}):
        mg = merge.Merge(st, [[i for i in ids if len(rows[i]) == L]])
        assert mg.finish() == L
        mg.close()


def test_rows_on_both_planes(gpu, consts):
    """Groups on plane 1, on plane 0 and alternating row by row, so that a slice of R rows mixes the planes.  The other plane of every row
    holds a copy that differs at every column and has no all-gap column where the live rows have one."""
    from twilight_amd import level

    T, R, C = consts
    rng = np.random.default_rng(11)
    shapes = [(R + 1, T + 33), (3, 2 * T + 1), (2 * R + 1, 129)]
    live, plane, groups = [], [], []
    for k, (n, L) in enumerate(shapes):
        groups.append(list(range(len(live), len(live) + n)))
        live.extend(_random_group(rng, n, L))
        plane.extend([1] * n if k == 0 else [0] * n if k == 1 else [i % 2 for i in range(n)])
    stale = [bytes((b ^ 0x55) if b != GAP else ord("N") for b in row) for row in live]
    st = level.Store(stale, "n")
    try:
        everyone = list(range(len(live)))
        _move_to_the_other_plane(st, everyone, stale)
        _move_to_the_other_plane(st, [i for i in everyone if plane[i] == 0], stale)
        st.write_rows(everyone, live)
        assert st.rows_of(everyone) == live
        _squeeze_and_compare(st, live, groups)
    finally:
        st.close()


def test_refusals_change_nothing(gpu, consts):
    import twilight_amd as twl
    from twilight_amd import backbone, level

    rng = np.random.default_rng(5)
    seqs = _random_group(rng, 4, 50) + _random_group(rng, 3, 70) + [b"AC-GT"]
    st = level.Store(seqs, "n")
    try:
        bad = [("a null offset table", (1, None, [0, 1], True), "bad argument"),
               ("a null id table", (1, [0, 2], None, True), "bad argument"),
               ("a null output", (1, [0, 2], [0, 1], False), "bad argument"),
               ("a negative count", (-1, [0], [0], True), "bad argument"),
               ("offsets that do not start at 0", (1, [1, 3], [0, 1, 2], True), "start at 0"),
               ("offsets that do not ascend", (2, [0, 3, 2], [0, 1, 2, 3], True), "do not ascend"),
               ("an empty group", (2, [0, 2, 2], [0, 1], True), "empty group"),
               ("an id outside the store", (1, [0, 2], [0, len(seqs)], True), "out of range"),
               ("a negative id", (1, [0, 2], [-1, 0], True), "out of range"),
               ("an id twice in one group", (1, [0, 3], [0, 1, 0], True), "listed twice"),
               ("an id in two groups", (2, [0, 2, 4], [0, 1, 4, 1], True), "listed twice"),
               ("two lengths in one group", (1, [0, 2], [3, 4], True), "differ in length")]
        for what, (n, off, ids, out), text in bad:
            with pytest.raises(twl.TwlError, match=text):
                backbone.squeeze_groups_raw(st, n, off, ids, out)
            assert st.rows() == seqs, what
        # a level that is still prepared
        one = np.asarray([1.0], dtype=F)
        p = twl.make_params(LC.matrix_of("n"))
        st.prepare(p, [[level.Side([7], one, 5, 1, 1.0), level.Side([0], one, 50, 1, 1.0)]])
        with pytest.raises(twl.TwlError, match="still prepared"):
            backbone.squeeze_groups(st, [[0, 1, 2, 3]])
        st.commit([np.zeros(0, dtype=np.int8)])
        assert st.rows() == seqs
        # no group: nothing happens; then the call goes through
        assert backbone.squeeze_groups(st, []) == []
        assert st.rows() == seqs
        _squeeze_and_compare(st, seqs, [[0, 1, 2, 3], [6, 5, 4]], untouched=[7])
    finally:
        st.close()


def test_a_squeezed_group_enters_a_level(gpu, consts):
    """A 3-row group, squeezed, against a single sequence through twl_level_prepare / align / commit == level_oracle on the squeezed rows."""
    import twilight_amd as twl
    from twilight_amd import backbone, level

    rng = np.random.default_rng(9)
    raw = _random_group(rng, 3, 400, p_gap_col=0.35, p_gap=0.2)
    single = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=230))
    squeezed = PO.squeeze_group(raw)
    assert 0 < len(squeezed[0]) < 400
    w = np.asarray([0.5, 0.25, 1.0], dtype=F)
    gw = float(F(F(w[0] + w[1]) + w[2]))
    case = LC.PairCase("n", 0.95, [LC.SideCase(squeezed, w, gw), LC.SideCase([single], np.asarray([1.0], dtype=F), 1.0)])
    e = LC.expected(case)
    st = level.Store(raw + [single], "n")
    try:
        assert backbone.squeeze_groups(st, [[0, 1, 2]]) == [len(squeezed[0])]
        p = twl.make_params(LC.matrix_of("n"))
        sides = [level.Side([0, 1, 2], LO.member_weights(w, gw, 3), len(squeezed[0]), 3, gw), level.Side([3], np.asarray([1.0], dtype=F), len(single), 1, 1.0)]
        lens, info = st.prepare(p, [sides])
        assert tuple(lens[0]) == e["lens"]
        for sd in range(2):
            assert np.array_equal(np.ascontiguousarray(st.columns(0, sd)).view(np.uint32), np.ascontiguousarray(e["cols"][sd], dtype=F).view(np.uint32)), f"side {sd}"
        aln, n, err = st.align(p)
        cr, cq = e["cols"]
        oa, oerr, _ = O.align_pair(O.make_params(LC.matrix_of("n")), cr[:, :6], cq[:, :6], cr[:, 6], cr[:, 7], cq[:, 6], cq[:, 7], 3, 1)
        assert err[0] == oerr and n[0] == len(oa) and np.array_equal(aln[0, : n[0]], oa)
        st.commit([e["path_full"]])
        assert st.rows() == e["rows_after"]
    finally:
        st.close()
