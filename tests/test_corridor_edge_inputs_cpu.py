"""The inputs of tests/test_gpu_corridor_edges.py are what tests/corridor_cases.py says they are (no GPU): the recorded c* of every pool from the oracle's trace
and exit hooks, the properties of the restated tile rule the GPU tests lean on, NaN as a safe sentinel, and a dropped and a kept tile in every matrix level."""
import numpy as np
import pytest

import corridor_cases as K
import dp_cases as D
import oracle_lib as O

M22 = D.matrix_of(22)
# the narrowest row window, in 64-row blocks, of the kernels a route's first launch and its tile jobs run on (twl_policy.inc.hip, prot_first_window)
WINDOW_OF_ROUTE = {"prot_plain16": 16, "prot_spec16": 16, "prot_spec_shared": 8, "prot_tiles": 8}


@pytest.mark.parametrize("pool", K.POOLS, ids=lambda p: p.name)
def test_recorded_smallest_safe_corridor_is_the_oracles(pool):
    b = pool.batch()
    cs = K.cstars(b, M22, **pool.params())
    spans = tuple(D.trace_pair(b, i, M22, **pool.params()).span for i in range(b.n_pairs))
    print(pool.name, "c*", cs, "spans", spans)
    K.check_pool(pool, cs, spans, min(WINDOW_OF_ROUTE[r] for r in pool.routes))
    # the knob values the GPU test uses split the pool: c* hands back strictly fewer pairs than c* - 1, and a knob of the longest Q nobody
    for c in set(cs):
        assert len(K.handed_back(cs, c)) < len(K.handed_back(cs, c - 1)) or c == 1
        assert c - 1 == 0 or sorted(K.handed_back(cs, c - 1)) == [n for n, v in enumerate(cs) if v >= c]
    assert K.handed_back(cs, pool.longest_q(b)) == [] and max(cs) <= pool.longest_q(b)


def test_two_end_tiles_of_a_band_decide_its_need():
    """cstar_of_rows looks at the first and the last tile of every traced diagonal; the tiles between them never need more (need is convex along a tile row)."""
    pool = K.POOL_BY_NAME["skew700"]
    b = pool.batch()
    for i in range(b.n_pairs):
        R, Q = int(b.len[i, 0]), int(b.len[i, 1])
        err, rows = K.band_of_pair(b, i, M22, **pool.params())
        assert err == 0 and len({t for t, *_ in rows}) >= 1
        brute = 0
        for _tile, Kd, lo, hi in rows:
            tiles = np.arange((lo // 64) * 64, hi + 1, 64)
            brute = max(brute, int(K.need(R, Q, tiles, (Kd // 64) * 64).max()))
        assert brute == K.cstar_of_rows(R, Q, rows) == pool.cstar[i]


def test_skewed_pair_leaves_the_line_between_the_corners_of_the_uncut_pair_by_hundreds_of_rows():
    """What `skew700` is for: measured against the pair it was cut from the path of pair 1 is hundreds of rows off; against its own corners it still needs the widest corridor."""
    pool = K.POOL_BY_NAME["skew700"]
    b = pool.batch()
    assert b.n_pairs == 4 and 650 <= int(b.len[:, 0].min()) and int(b.len[:, 0].max()) <= 750
    assert int(b.len[1, 1]) * 10 <= int(b.len[1, 0]) * 6 + 10 and pool.cstar[1] == max(pool.cstar)
    _, rows = K.band_of_pair(b, 1, M22, **pool.params())
    a = np.asarray(rows)
    R, Q = int(b.len[1, 0]), int(b.len[1, 1])
    mid = (a[:, 2] + a[:, 3]) // 2
    off_uncut = np.abs(mid - a[:, 1] // 2)            # the uncut pair's line: I = K / 2
    assert off_uncut.max() >= 100, int(off_uncut.max())
    assert a[:, 1].max() == R + Q - 2                  # the band reaches the last anti-diagonal: the path ends in the far corner


SHAPES = [(R, Q) for lv in K.LEVELS for R, Q in lv.shapes] + [(int(r), int(q)) for p in K.POOLS[:1] + K.POOLS[1:2] + K.POOLS[3:4] for r, q in p.batch().len.tolist()] + \
         [(1, 1), (64, 64), (63, 65), (2500, 1500), (1500, 2500), (5000, 70)]


def test_a_tile_kept_at_a_corridor_is_kept_at_every_larger_one():
    for R, Q in SHAPES:
        n = K.need_grid(R, Q)
        knobs = sorted({1, 2, 63, 64, 65, 448, int(n.max()), int(n.max()) + 1} | {int(v) for v in np.unique(n)[:50]} | {max(int(v) - 1, 1) for v in np.unique(n)[:50]})
        I0, K0 = K.tile_grid(R, Q)
        prev = None
        for c in knobs:
            if c <= 0:
                continue
            drop = K.dropped(R, Q, I0[None, :], K0[:, None], c)
            assert np.array_equal(drop, n > c)
            if prev is not None:
                assert not (drop & ~prev).any(), (R, Q, c)      # dropped now => dropped at the smaller knob
            prev = drop
        assert not K.dropped(R, Q, I0[None, :], K0[:, None], 0).any()                  # 0: the whole matrix
        assert not K.dropped(R, Q, I0[None, :], K0[:, None], max(Q, 1)).any()          # no tile is further than Q rows from a row of the matrix


def test_need_is_zero_exactly_for_the_tiles_the_line_falls_into():
    for R, Q in SHAPES:
        I0, K0 = K.tile_grid(R, Q)
        n = K.need_grid(R, Q)
        ic = K.line_row(R, Q, K0)
        assert (ic >= 0).all() and (ic < Q + 64).all(), (R, Q)
        inside = (I0[None, :] <= ic[:, None]) & (ic[:, None] <= I0[None, :] + 63)
        assert np.array_equal(n == 0, inside), (R, Q)
        # at most one tile per tile row, and exactly one wherever the line's row is a row of the stored matrix (in the last tile row K0 + 32 may lie past the far corner)
        assert (inside.sum(axis=1) <= 1).all() and (inside.sum(axis=1)[ic < K.pitch_of(Q)] == 1).all(), (R, Q)


def test_restated_rule_is_the_kernels_condition_written_out():
    """`I0 > ic + c || I0 + 63 < ic - c` (talco_kernel.hip.h) against `0 < c < need`, over every tile of every shape and a spread of knob values."""
    for R, Q in SHAPES:
        I0, K0 = K.tile_grid(R, Q)
        ic = K.line_row(R, Q, K0)[:, None]
        for c in (0, 1, 31, 63, 64, 65, 127, 128, 448, 5000):
            kernel = (c > 0) & ((I0[None, :] > ic + c) | (I0[None, :] + 63 < ic - c))
            assert np.array_equal(kernel, K.dropped(R, Q, I0[None, :], K0[:, None], c)), (R, Q, c)


def _grids(b, pk):
    op = O.make_params(M22, **pk)
    for i in range(b.n_pairs):
        R, Q = int(b.len[i, 0]), int(b.len[i, 1])
        yield i, O.column_score_grid(op, b.freq[i, 0, :R], b.freq[i, 1, :Q], float(np.float32(b.num[i, 0]) * np.float32(b.num[i, 1])))


def test_grid_form_of_the_oracles_column_score_is_the_oracles_column_score():
    lv = K.LEVEL_BY_NAME["q_mod64"]
    b = lv.batch(1)
    op = O.make_params(M22, **lv.params())
    rng = np.random.default_rng(5)
    for i, g in _grids(b, lv.params()):
        R, Q = int(b.len[i, 0]), int(b.len[i, 1])
        assert g.shape == (Q, R)
        d = float(np.float32(b.num[i, 0]) * np.float32(b.num[i, 1]))
        for q, r in zip(rng.integers(0, Q, 200).tolist() + [0, Q - 1], rng.integers(0, R, 200).tolist() + [0, R - 1]):
            want = np.float32(O.column_score(op, b.freq[i, 0, r], b.freq[i, 1, q], d))
            assert g[q, r].view(np.uint32) == want.view(np.uint32), (i, q, r)


@pytest.mark.parametrize("pool", [p for p in K.POOLS if "@" not in p.name], ids=lambda p: p.name)
def test_no_score_of_a_pool_is_nan(pool):
    """NaN marks an unscored tile: no pair may have a score that is one by itself (nor an infinity, whose sums could become one)."""
    b = pool.batch()
    for i, g in _grids(b, pool.params()):
        assert np.isfinite(g).all(), (pool.name, i)


@pytest.mark.parametrize("lv", K.LEVELS, ids=lambda lv: lv.name)
def test_every_matrix_level_has_a_dropped_and_a_kept_tile_and_no_nan_of_its_own(lv):
    for seed in (1, 2):
        b = lv.batch(seed)
        assert [tuple(x) for x in b.len.tolist()] == list(lv.shapes)
        assert 3 <= b.n_pairs <= 4 and len({(R + Q - 1 + 63) // 64 * ((Q + 63) // 64) for R, Q in lv.shapes}) >= 2      # items of different tile counts
        if lv.leaf >= 0:
            assert tuple(b.num[lv.leaf]) == (1, 1) and (b.num.prod(axis=1) > 1).sum() >= 2
            R, Q = lv.shapes[lv.leaf]
            assert (np.count_nonzero(b.freq[lv.leaf, 0, :R], axis=1) == 1).all() and (np.count_nonzero(b.freq[lv.leaf, 1, :Q], axis=1) == 1).all()
        for i, g in _grids(b, lv.params()):
            assert np.isfinite(g).all(), (lv.name, i)
    n_drop = n_keep = 0
    for R, Q in lv.shapes:
        I0, K0 = K.tile_grid(R, Q)
        drop = K.dropped(R, Q, I0[None, :], K0[:, None], K.MATRIX_KNOB)
        n_drop += int(drop.sum()); n_keep += int((~drop).sum())
        nan = K.nan_cells(R, Q, K.MATRIX_KNOB) & K.cell_mask(R, Q)
        assert nan.sum() <= drop.sum() * 64 * 64
    assert n_drop >= 1 and n_keep >= 1, (lv.name, n_drop, n_keep)
    # the edge knobs: ON the value a tile with exactly that need is kept, one row less drops it, on either side of the line; and every knob value used drops and keeps
    below, above = lv.edge_knobs()
    for side, c in (("below", below), ("above", above)):
        on = off = 0
        for R, Q in lv.shapes:
            I0, K0 = K.tile_grid(R, Q)
            ic = K.line_row(R, Q, K0)[:, None]
            dist = (I0[None, :] - ic) if side == "below" else (ic - I0[None, :] - 63)
            hit = dist == c
            assert np.array_equal(K.need_grid(R, Q)[hit], dist[hit])
            on += int((hit & ~K.dropped(R, Q, I0[None, :], K0[:, None], c)).sum())
            off += int((hit & K.dropped(R, Q, I0[None, :], K0[:, None], c - 1)).sum()) if c > 1 else 0
        assert on >= 1 and (off == on or c == 1), (lv.name, side, c, on, off)
    for c in lv.knobs():
        if c > 0:
            drops = [K.need_grid(R, Q) > c for R, Q in lv.shapes]
            assert any(d.any() for d in drops) and any((~d).any() for d in drops), (lv.name, c)


def test_matrix_levels_cover_the_shapes_they_are_for():
    qs = {Q for lv in K.LEVELS for _R, Q in lv.shapes}
    ks = {R + Q - 1 for lv in K.LEVELS for R, Q in lv.shapes}
    assert {63, 0, 1} <= {Q % 64 for Q in qs if Q > 64} and {63, 0, 1} <= {k % 64 for k in ks if k > 64}
    assert any(Q < 64 and Q > 1 for Q in qs)
    assert any(R == 1 for lv in K.LEVELS for R, _Q in lv.shapes) and any(Q == 1 for lv in K.LEVELS for _R, Q in lv.shapes)
    assert any(R >= 3 * Q > 3 for lv in K.LEVELS for R, Q in lv.shapes) and any(Q >= 3 * R > 3 for lv in K.LEVELS for R, Q in lv.shapes)
    assert any(lv.gap_char == 0.0 for lv in K.LEVELS) and any(lv.leaf >= 0 for lv in K.LEVELS)
