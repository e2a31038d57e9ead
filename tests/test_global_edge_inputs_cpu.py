"""The directed inputs of tests/test_gpu_global_edges.py are the edges they claim to be.  No GPU.

Every case of tests/global_cases.py goes through the checker alone (oracle_lib.align_pair with the trace hook, oracle_lib.align_batch
for the levels) and is held to the figures committed next to it AND to the property the GPU test needs of it:

A  the widest band of a round case is exactly Q rows (Q = 1023 ... 3073: one row below, on and above one, two and three rounds of the
   kernel's 1024 threads) when flen >= Q, reached in tile 0, and the pair stops with errorType 2 one row earlier when flen = Q - 1;
B  the convergence pair has tiles that end by convergence more than one round wide, one of them after having been more than two
   rounds wide, and its companion converges below one round;
C  the queue pool has the good and the failed pairs each of its calls is there for;
D  the scratch of the large level is above the release threshold, that of the small one far below.

A constant of global_cases.py moved to a neighbouring value (Q by one, the X-drop of section B by a factor of ten) fails here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import global_cases as G  # noqa: E402
import oracle_lib as O  # noqa: E402


# ---- A ----
def test_the_round_cases_stand_on_both_sides_of_one_two_and_three_rounds():
    have = {(c.P, c.Q) for c in G.ROUND_CASES}
    for rounds in (1, 2):
        assert {(6, rounds * G.T - 1), (6, rounds * G.T), (6, rounds * G.T + 1)} <= have
    assert (6, 3 * G.T + 1) in have and (22, G.T + 1) in have
    assert all(c.flens() == (c.Q + 7, c.Q, c.Q - 1) for c in G.ROUND_CASES)


@pytest.mark.parametrize("case", G.ROUND_CASES, ids=lambda c: c.name)
def test_round_case_is_exactly_q_rows_wide(case):
    batch = case.batch()
    assert tuple(batch.len[0]) == (case.Q + 40, case.Q) and batch.seq_len >= case.Q + 40
    for flen in case.flens():
        r = G.oracle_pair(batch, 0, **case.params(flen))
        tag = f"{case.name} flen {flen}: err {r.err} max_width {r.max_width} tiles {r.n_tiles} cells {r.cells} tile widths {[t.max_width for t in r.tiles]}"
        assert (r.err, r.max_width, r.cells) == case.expected(flen), tag
        if flen >= case.Q:
            assert r.n_tiles == case.tiles and len(r.tiles) == case.tiles, tag
            assert r.tiles[0].max_width == case.Q, tag                 # a diagonal of exactly Q rows in tile 0
            assert min(flen, batch.seq_len) == flen, tag               # (what twl_stats.window is to say)
        else:
            # the band is never flen + 1 rows wide in the trace: the diagonal on which the oracle stops is not traced
            assert r.n_tiles == 1 and r.tiles[0].max_width == case.Q - 1, tag


# ---- B ----
@pytest.mark.parametrize("case", G.CONV_CASES, ids=lambda c: c.name)
def test_convergence_case_has_its_figures(case):
    batch = case.batch()
    r = G.oracle_pair(batch, 0, **case.params())
    inner = r.tiles[:-1]                      # every tile but the pair's last
    tag = f"{case.name}: err {r.err} tiles {r.n_tiles} max_width {r.max_width} cells {r.cells} (widest, last k, last width) {[(t.max_width, t.last_k, t.last_width) for t in r.tiles]}"
    assert (r.err, r.n_tiles, r.max_width, r.cells) == (0, case.tiles, case.max_width, case.cells), tag
    assert tuple(t.last_width for t in inner) == case.last_widths and tuple(t.max_width for t in inner) == case.tile_widths, tag
    # tile 0 spans the whole pair: it stops in front of its last diagonal, so it ended by convergence (a tile that is not the pair's last did so as well)
    assert r.tiles[0].last_k < int(batch.len[0].sum()) - 2, tag


def test_tiles_converge_wider_than_one_round_and_once_after_more_than_two():
    case = G.CONV_BY_NAME["conv_wide"]
    wide = [(w, m) for w, m in zip(case.last_widths, case.tile_widths) if w > G.T]
    assert len(wide) >= 2 and any(m > 2 * G.T for _w, m in wide), (case.last_widths, case.tile_widths)


def test_the_companion_converges_below_one_round_after_a_band_of_several():
    case = G.CONV_BY_NAME["conv_narrow"]
    assert case.tile_widths[0] > 2 * G.T and 0 < case.last_widths[0] < G.T, (case.last_widths, case.tile_widths)
    assert {c.seq_len for c in G.CONV_CASES} == {3100} and all(int(c.batch().len.max()) <= 3100 for c in G.CONV_CASES)


# ---- C ----
_POOL = {}


def _pool(P):
    if P not in _POOL:
        _POOL[P] = G.queue_pool(P)
    return _POOL[P]


def test_the_queue_pool_is_24_distinct_live_pairs_and_two_with_an_empty_side():
    for P, hi in ((6, 1250), (22, 400)):
        pool = _pool(P)
        live, empty = pool.len[: G.QUEUE_LIVE], pool.len[G.QUEUE_LIVE:]
        assert pool.n_pairs == G.QUEUE_LIVE + 2 and (live >= 30).all() and (live < hi).all()
        assert empty.tolist() == [[0, int(empty[0, 1])], [int(empty[1, 0]), 0]] and empty[0, 1] > 0 and empty[1, 0] > 0
        assert len({pool.freq[i].tobytes() for i in range(G.QUEUE_LIVE)}) == G.QUEUE_LIVE
        sums = live.sum(axis=1)
        assert len(set(sums.tolist())) > 20           # (longest first is an order, not a tie)
    idx = G.queue_level_index(300)
    assert idx[: G.QUEUE_LIVE + 2].tolist() == list(range(G.QUEUE_LIVE + 2)) and int((idx < G.QUEUE_LIVE).sum()) == 300 - 2 * 11


@pytest.mark.parametrize("call", G.QUEUE_CALLS, ids=lambda c: c.name)
def test_queue_call_has_its_good_and_failed_pairs(call):
    pool = _pool(call.P)
    rs = G.oracle_pairs(pool, **call.pk())
    live = rs[: G.QUEUE_LIVE]
    errs = tuple(sum(1 for r in live if r.err == e) for e in (0, 1, 2))
    tag = f"{call.name}: errorTypes 0/1/2 {errs} max_width {max(r.max_width for r in live)} cells {sum(r.cells for r in rs)}"
    assert errs == call.errs and sum(errs) == G.QUEUE_LIVE, tag
    assert max(r.max_width for r in live) == call.max_width and sum(r.cells for r in rs) == call.cells, tag
    assert all(r.err == 0 and r.path.size == 0 and r.cells == 0 for r in rs[G.QUEUE_LIVE:]), tag
    # the level the oracle sees as a batch: the same error codes and cells, the empty-side pairs with length 0 and errorType 0
    oa, on, oerr, ost = O.align_batch(O.make_params(G.matrix_of(call.P), **call.pk()), pool, threads=8)
    assert oerr.tolist() == [r.err for r in rs] and ost.cells == call.cells, tag
    assert on.tolist() == [r.path.size if r.err == 0 else 0 for r in rs], tag


def test_the_queue_calls_are_what_the_gpu_test_needs():
    by = G.QUEUE_BY_NAME
    assert by["defaults"].pk() == {} and by["protein"].pk() == {} and by["open"].pk() == dict(xdrop=G.XDROP_OPEN, flen=4096)
    assert by["open"].max_width > G.T                                   # some first pairs are two rounds wide
    assert by["flen200"].errs[2] >= 4 and by["flen200"].errs[0] >= 4 and set(by["flen200"].pk()) == {"flen"}
    assert all(c.cus_times == 1 for c in G.QUEUE_CALLS if c.name != "marker64") and G.queue_level_size(by["defaults"], 256) == 296
    # marker64: on twice the CUs the pairs behind the first 256 are many pool pairs, and all of them run several tiles past the marker
    m64 = by["marker64"]
    pool = _pool(6)
    idx = G.queue_level_index(G.queue_level_size(m64, 256))
    live = idx[idx < G.QUEUE_LIVE]
    order = live[np.argsort(-pool.len[live].sum(axis=1), kind="stable")]      # order_pairs: longest first
    later = set(order[256:].tolist())
    assert m64.pk() == dict(marker=64) and len(later) >= 10 and all(int(pool.len[j].sum()) > 3 * 64 for j in later), sorted(later)
    assert by["xdrop800"].errs[1] >= 4 and by["xdrop800"].errs[0] >= 4 and set(by["xdrop800"].pk()) == {"xdrop"} and by["xdrop800"].pk()["xdrop"] > 40


# ---- D ----
def test_the_large_level_is_above_the_release_threshold_and_the_small_one_below():
    large, small = G.scratch_large(), G.scratch_small()
    assert large.n_pairs == 72 and large.seq_len == 4096 and int(large.len.min()) >= 60 and int(large.len.max()) <= 300
    words = G.scratch_words(4096, large.seq_len, 1024)
    assert words == 14 * 4098 + (1026 * 4098 + 3) // 4 == 1108509
    assert 72 * words * 4 > G.RELEASE_BYTES                              # 319 MB at 72 workgroups ...
    assert 72 * G.scratch_words(4096, large.seq_len, 2) * 4 < G.RELEASE_BYTES < 72 * words * 4      # ... of which the pointer bytes are the larger part
    assert small.n_pairs == 8 and 8 * G.scratch_words(4096, small.seq_len, 1024) * 4 < G.RELEASE_BYTES // 16
    for name, batch in (("large", large), ("small", small)):
        oa, on, oerr, ost = O.align_batch(O.make_params(G.matrix_of(6)), batch, threads=8)
        assert not oerr.any() and ost.cells == G.SCRATCH_CELLS[name], (name, oerr.tolist(), ost.cells)
