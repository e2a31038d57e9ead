"""The kernels of the placement finish that keeps the backbone's length (keep_kernels.hip.h, twl_keep.inc.hip) through the binding
twilight_amd/keep.py with paths from the host (no DP is involved), against tests/keep_oracle.py: rows, per-sequence counts, totals and
every run record exactly -- bytes and integers only, no tolerance anywhere.  The inputs are those of tests/place_cases.py (tiles and thread
chunks of the path walk) and of tests/keep_cases.py (the rank scan of the run ends); tests/test_keep_oracle_cpu.py proves that each
reaches the branch it is listed for."""
import numpy as np
import pytest

import keep_cases as KC
import keep_oracle as KO
import place_cases as PC
import place_oracle as PO

pytestmark = pytest.mark.gpu


def _check_records(pl, ids, seqs_by_id, paths_by_id, run_off=None):
    """dropped_counts and dropped_runs of `ids` (in that order) against the oracle."""
    from twilight_amd import keep

    runs, letters = keep.dropped_counts(pl, ids)
    want = [KO.runs(paths_by_id[i]) for i in ids]
    assert runs.tolist() == [len(w) for w in want]
    assert letters.tolist() == [sum(n for _, _, n in w) for w in want]
    off, col, qpos, ln = keep.dropped_runs(pl, ids, run_off)
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    flat = [r for w in want for r in w]
    assert list(zip(col.tolist(), qpos.tolist(), ln.tolist())) == flat
    for i, w in zip(ids, want):
        assert all(0 <= q and q + n <= len(seqs_by_id[i]) for _, q, n in w)


def _keep(backbone, seqs, paths, calls, extra=(), minimal_pitch=False, seq_type="n"):
    """One store (backbone rows, sequences, then `extra` rows that are never placed), one placement, collect_host in the given calls,
    finish_keep: totals, rows, counts and records equal the oracle's; the backbone and the extra rows are the uploaded bytes."""
    import twilight_amd as twl
    from twilight_amd import api, keep, level, place

    B, L = len(backbone), len(backbone[0])
    all_rows = list(backbone) + list(seqs) + list(extra)
    if minimal_pitch:
        twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 1)          # the generous pitch fails: the store starts at the pitch its sequences need
    try:
        st = level.Store(all_rows, seq_type)
    finally:
        twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 0)
    pl = place.Placement(st, L)
    order = []
    for g in calls:
        pl.collect_host([B + k for k in g], [paths[k] for k in g])
        order += list(g)
    assert sorted(order) == list(range(len(seqs)))
    longest = PO.merge_insertions(L, paths)
    assert np.array_equal(pl.insertions(), longest)
    want_counts = [KO.counts(p) for p in paths]
    assert keep.finish_keep(pl) == (sum(r for r, _ in want_counts), sum(n for _, n in want_counts))
    got = st.rows_of(list(range(len(all_rows))))
    want = list(backbone) + [KO.keep_row(s, p, L) for s, p in zip(seqs, paths)] + list(extra)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"row {i} ({'backbone' if i < B else 'placed' if i < B + len(seqs) else 'not placed'})"
    for s, p, g in zip(seqs, paths, got[B:]):
        assert g == KO.strip_row(PO.expand_placed(s, p, longest), longest)
    by_id_s = {B + k: s for k, s in enumerate(seqs)}
    by_id_p = {B + k: p for k, p in enumerate(paths)}
    _check_records(pl, [B + k for k in order], by_id_s, by_id_p)                   # the collect order
    if len(seqs) > 1:
        _check_records(pl, [B + k for k in reversed(range(len(seqs)))], by_id_s, by_id_p)      # another order
        _check_records(pl, [B + k for k in range(1, len(seqs), 2)], by_id_s, by_id_p)          # a subset
    assert np.array_equal(pl.insertions(), longest)
    return st, pl


def _close(st, pl):
    pl.close()
    st.close()


# ---- (a) the path walk: tiles and thread chunks ----

PLACE_CALLS = {
    "tiles": [[0, 1, 2], [3], [4, 5, 6, 7]],
    "tiles2": [[0, 1]],
    "chunks": [[0, 1, 2, 3, 4, 5, 6]],
    "len4095": [[0, 1]],
    "len4096": [[1], [0]],
    "len4097": [[0, 1]],
}


@pytest.mark.parametrize("name", list(PLACE_CALLS))
def test_rows_and_records_on_the_placement_specs(gpu, name):
    """Runs that end on a tile's last code, cross a tile edge, fill one and two whole tiles, start the path and end it; runs on positions
    14-17 of a thread's 16 codes; paths of exactly 4095, 4096 and 4097 codes; a sequence without letters and one without insertions."""
    backbone, seqs, paths = PC.group_inputs(name)
    _close(*_keep(backbone, seqs, paths, PLACE_CALLS[name]))


# ---- (b) the rank scan of the run ends ----

@pytest.mark.parametrize("name", KC.GROUPS)
def test_rank_scan_of_the_run_ends(gpu, name):
    """Run ends on item 15 of a thread and item 0 of another, 257 run ends in one tile (more than threads), 4097 in one path (more than a
    tile has codes, over four tiles), a run end on each tile's last code, a path with no run, and with L = 0 a path that is one run."""
    backbone, seqs, paths = KC.group_inputs(name)
    _close(*_keep(backbone, seqs, paths, [list(range(len(seqs)))]))


@pytest.mark.parametrize("L", [255, 257, 513])
def test_round_families_and_a_row_that_is_not_placed(gpu, L):
    """The scan-round families of the merged finish, kept at L; at L = 257 every sequence carries a run of 400 and more letters, so the
    input rows are longer than the rows written; a sequence that is not placed keeps its row."""
    backbone, seqs, paths, _ = PC.round_inputs(L)
    _close(*_keep(backbone, seqs, paths, [[0, 1], [2, 3]], extra=[b"acgtNNAC-gt" * 3]))


# ---- (c) re-pitch: the store's pitch cannot hold L ----

def test_short_sequences_only_force_the_repitch(gpu):
    """A store of short sequences only, started at the pitch they need (256), and a placement of L = 300 that no row of the store has:
    twl_place_create accepts it, and finish_keep re-pitches both planes before it writes 300 columns."""
    from twilight_amd import keep, level, place
    import twilight_amd as twl
    from twilight_amd import api

    rng = np.random.default_rng(8)
    L = 300
    runs = [{0: 2}, {}, {299: 1, 300: 3}, {150: 4}]
    dels = [tuple(c for c in range(L) if c % 40 >= 3 + k) for k in range(4)]       # 3 + k letters per 40 columns: sequences of 24 .. 60 letters
    paths = [PC.make_path(L, r, d) for r, d in zip(runs, dels)]
    seqs = [PC.make_seq(rng, p) for p in paths]
    assert max(len(s) for s in seqs) < 100
    twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 1)
    try:
        st = level.Store(seqs, "n")
    finally:
        twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 0)
    pl = place.Placement(st, L)
    pl.collect_host(range(4), paths)
    want_counts = [KO.counts(p) for p in paths]
    assert keep.finish_keep(pl) == (sum(r for r, _ in want_counts), sum(n for _, n in want_counts))
    assert st.rows_of([0, 1, 2, 3]) == [KO.keep_row(s, p, L) for s, p in zip(seqs, paths)]
    _check_records(pl, [3, 0, 2, 1], dict(enumerate(seqs)), dict(enumerate(paths)))
    _close(st, pl)


# ---- (d) a second placement on the same store: the placed rows start on plane 1 ----

def test_second_placement_starts_on_plane_one(gpu):
    """A first placement is finished with twl_place_finish: its backbone and placed rows live on plane 1 at width W1.  Two of its placed
    rows (plane 1) and two fresh sequences (plane 0) are then placed against L2 columns with finish_keep: rows of both planes are read,
    each written to its other plane; the first backbone, not named anywhere, stays as the merged finish left it."""
    from twilight_amd import keep, level, place

    rng = np.random.default_rng(43)
    L, B = 300, 2
    backbone = [rng.choice(list(b"ACGTacgt-"), L).astype(np.uint8).tobytes() for _ in range(B)]
    runs1 = [{0: 3, 150: 2}, {150: 6, 300: 1}, {}, {299: 4}]
    paths1 = [PC.make_path(L, r, tuple(range(k, L, 37))) for k, r in enumerate(runs1)]
    seqs1 = [PC.make_seq(rng, p) for p in paths1]
    longest1 = PO.merge_insertions(L, paths1)
    rows1 = [PO.expand_backbone(r, longest1) for r in backbone] + [PO.expand_placed(s, p, longest1) for s, p in zip(seqs1, paths1)]
    W1 = L + int(longest1.sum())
    L2 = 280
    # second round: the merged rows of seqs1[0] and seqs1[1] (W1 bytes each, '.' and '-' among them: bytes like any other) and two fresh sequences
    runs2 = [{0: W1 - L2}, {5: 10, L2: W1 - L2 - 10}, {0: 2, 255: 3, 256: 1}, {}]
    dels2 = [(), (), (7, 8, 9), tuple(range(3, L2, 29))]
    paths2 = [PC.make_path(L2, r, d) for r, d in zip(runs2, dels2)]
    fresh = [PC.make_seq(rng, p) for p in paths2[2:]]
    n1 = B + len(seqs1)
    st = level.Store(backbone + seqs1 + fresh, "n")
    pl = place.Placement(st, L)
    pl.collect_host(range(B, n1), paths1)
    assert pl.finish(range(B)) == W1
    assert st.rows_of(list(range(n1))) == rows1
    ids2 = [B, B + 1, n1, n1 + 1]
    seqs2 = [rows1[B], rows1[B + 1]] + fresh
    assert all(len(s) == int(np.count_nonzero(p != 2)) for s, p in zip(seqs2, paths2))
    pl2 = place.Placement(st, L2)
    pl2.collect_host(ids2, paths2)
    want_counts = [KO.counts(p) for p in paths2]
    assert keep.finish_keep(pl2) == (sum(r for r, _ in want_counts), sum(n for _, n in want_counts))
    assert st.rows_of(ids2) == [KO.keep_row(s, p, L2) for s, p in zip(seqs2, paths2)]
    assert st.rows_of([0, 1, B + 2, B + 3]) == [rows1[0], rows1[1], rows1[B + 2], rows1[B + 3]]
    _check_records(pl2, [n1 + 1, B, n1, B + 1], dict(zip(ids2, seqs2)), dict(zip(ids2, paths2)))
    pl2.close()
    _close(st, pl)


# ---- (e) many sequences in one placement ----

def test_300_sequences_in_one_placement(gpu):
    """300 workgroups of the rows kernel and of the runs kernel, protein letters, paths on both sides of one tile."""
    rng = np.random.default_rng(44)
    L, B = 4000, 3
    backbone = [rng.choice(list(b"ACDEFGHIKLMNPQRSTVWYacdxy-"), L).astype(np.uint8).tobytes() for _ in range(B)]
    paths = []
    for k in range(300):
        runs = {int(c): int(rng.integers(1, 30)) for c in rng.choice(L + 1, k % 7, replace=False)}
        paths.append(PC.make_path(L, runs, tuple(rng.choice(L, k % 11, replace=False).tolist())))
    seqs = [PC.make_seq(rng, p, PC.AA) for p in paths]
    assert any(len(p) > PC.TILE for p in paths) and any(len(p) <= PC.TILE for p in paths)
    _close(*_keep(backbone, seqs, paths, [list(range(0, 300, 2)), list(range(1, 300, 2))], seq_type="p"))


# ---- (f) refusals ----

def test_either_finish_after_the_other_is_refused_and_the_store_stays(gpu):
    from twilight_amd import keep, level, place

    backbone, seqs, paths = KC.group_inputs("ranks16")
    B, L, n = len(backbone), len(backbone[0]), len(seqs)
    st, pl = _keep(backbone, seqs, paths, [list(range(n))])
    before = st.rows_of(list(range(B + n)))
    with pytest.raises(Exception, match="twl_place_finish after twl_place_finish_keep"):
        pl.finish(range(B))
    with pytest.raises(Exception, match="twl_place_finish_keep called twice"):
        keep.finish_keep(pl)
    with pytest.raises(Exception, match="after twl_place_finish"):
        pl.collect_host([0], [np.zeros(L, np.int8)])
    assert st.rows_of(list(range(B + n))) == before
    _check_records(pl, [B + k for k in range(n)], {B + k: s for k, s in enumerate(seqs)}, {B + k: p for k, p in enumerate(paths)})
    # the lists of the dropped_* calls
    with pytest.raises(Exception, match="the sequence was not collected"):
        keep.dropped_counts(pl, [B, 0])
    with pytest.raises(Exception, match="a sequence id is listed twice"):
        keep.dropped_counts(pl, [B, B])
    with pytest.raises(Exception, match="run_off is not the exclusive scan"):
        keep.dropped_runs(pl, [B, B + 1], run_off=[0, 1, 2])
    off, col, qpos, ln = keep.dropped_runs(pl, [])
    assert len(col) == 0 and keep.dropped_counts(pl, [])[0].tolist() == []
    rows_ms, runs_ms = keep.timing(pl)
    assert rows_ms > 0 and runs_ms > 0
    _close(st, pl)

    # the other way round, on a fresh store
    st = level.Store(list(backbone) + list(seqs), "n")
    pl = place.Placement(st, L)
    pl.collect_host(range(B, B + n), paths)
    with pytest.raises(Exception, match="twl_place_dropped_counts before twl_place_finish_keep"):
        keep.dropped_counts(pl, [B])
    W = pl.finish(range(B))
    merged = st.rows_of(list(range(B + n)))
    with pytest.raises(Exception, match="twl_place_finish_keep after twl_place_finish"):
        keep.finish_keep(pl)
    assert st.rows_of(list(range(B + n))) == merged and len(merged[0]) == W
    _close(st, pl)
