"""CPU checks of the oracle itself (no GPU): legality, known answers, tie-breaks, error protocol."""
import numpy as np
import pytest

import oracle_lib as O
from twilight_amd import synth

M = synth.nucleotide_matrix()


def onehot(seq, P=6):
    a = np.zeros((len(seq), P), dtype=np.float32)
    a[np.arange(len(seq)), ["ACGTN-".index(c) for c in seq]] = 1.0
    return a


def run_pair(ref, qry, **pk):
    p = O.make_params(M, **pk)
    R, Q = ref.shape[0], qry.shape[0]
    go = np.full(max(R, Q), p.gap_open, dtype=np.float32)
    ge = np.full(max(R, Q), p.gap_extend, dtype=np.float32)
    return O.align_pair(p, ref, qry, go[:R], ge[:R], go[:Q], ge[:Q], 1.0, 1.0)


def test_default_nucleotide_matrix():
    # reference scoring-matrix.cpp:97-110: match 18, transition (A<->G, C<->T) -4, mismatch -8, N row/col 0
    assert M[0, 0] == 18 and M[0, 2] == -4 and M[1, 3] == -4 and M[0, 1] == -8 and M[4, 2] == 0 and M[3, 4] == 0
    assert np.array_equal(M, M.T)


def test_column_score_known_answers():
    p = O.make_params(M)
    e = np.eye(6, dtype=np.float32)
    for a in range(5):
        for b in range(5):
            assert O.column_score(p, e[a], e[b], 1.0) == M[a, b]
    # letter vs gap column scores gapCharScore (= gapExtend), gap vs gap scores 0 (TALCO-XDrop.cpp:394-395)
    assert O.column_score(p, e[0], e[5], 1.0) == -5.0
    assert O.column_score(p, e[5], e[3], 1.0) == -5.0
    assert O.column_score(p, e[5], e[5], 1.0) == 0.0
    # weighted columns: sum_l sum_m r_l q_m M_lm / (refNum*qryNum)
    r = np.array([2, 0, 1, 0, 0, 1], dtype=np.float32)
    q = np.array([0, 3, 0, 0, 0, 0], dtype=np.float32)
    want = (2 * 3 * -8 + 1 * 3 * -8 + 1 * 3 * -5) / 12.0
    assert O.column_score(p, r, q, 12.0) == np.float32(want)


def test_identical_sequences_all_match():
    rng = np.random.default_rng(0)
    s = "".join(rng.choice(list("ACGT"), size=2500))
    aln, err, st = run_pair(onehot(s), onehot(s))
    assert err == 0 and len(aln) == 2500 and not aln.any()
    assert st.tiles >= 2            # 2500+2500 diagonals with marker 1024 -> several tiles


def test_single_deletion_and_insertion_are_placed():
    rng = np.random.default_rng(1)
    s = "".join(rng.choice(list("ACGT"), size=400))
    q = s[:200] + s[205:]           # query lacks 5 reference columns -> five 2s
    aln, err, _ = run_pair(onehot(s), onehot(q))
    assert err == 0 and (aln == 2).sum() == 5 and (aln == 1).sum() == 0
    aln2, err2, _ = run_pair(onehot(q), onehot(s))
    assert err2 == 0 and (aln2 == 1).sum() == 5 and (aln2 == 2).sum() == 0
    go, ge = np.full(400, -50.0, dtype=np.float32), np.full(400, -5.0, dtype=np.float32)      # twlo_align_pair_exits with a null hook is twlo_align_pair
    assert np.array_equal(O.align_pair_exits(O.make_params(M), onehot(s), onehot(q), go, ge, go[:395], ge[:395], 1.0, 1.0)[0], aln)


@pytest.mark.parametrize("members", [(1, 1), ((2, 5), (2, 5))])
def test_paths_are_legal_and_deterministic(members):
    b = synth.make_level_batch(6, 700, members=members, seed=42)
    p = O.make_params(M)
    a1, n1, e1, s1 = O.align_batch(p, b, threads=4)
    a2, n2, e2, s2 = O.align_batch(p, b, threads=1)
    assert np.array_equal(a1, a2) and np.array_equal(n1, n2) and s1.cells == s2.cells
    for i in range(b.n_pairs):
        assert e1[i] == 0
        assert synth.path_consumes(a1[i], n1[i]) == tuple(b.len[i])
        assert set(np.unique(a1[i, : n1[i]])) <= {0, 1, 2}


def test_tiling_does_not_depend_on_marker_for_clean_data():
    # with near-identical sequences every tile converges on the main diagonal: path independent of marker
    rng = np.random.default_rng(3)
    s = "".join(rng.choice(list("ACGT"), size=1500))
    q = s[:700] + "ACGTAC" + s[700:]
    base, e0, _ = run_pair(onehot(s), onehot(q))
    for marker in (32, 100, 513):
        aln, err, st = run_pair(onehot(s), onehot(q), marker=marker)
        assert err == 0 and np.array_equal(aln, base), marker


def test_error_protocol():
    b = synth.make_level_batch(3, 600, members=(1, 1), seed=9)
    _, n, err, _ = O.align_batch(O.make_params(M, flen=64), b)
    assert (err == 2).all() and (n == 0).all()                       # TALCO-XDrop.cpp:331-338
    b2 = synth.make_level_batch(3, 300, members=(1, 1), seed=21, sub=0.75, indel=0.05)
    _, n2, err2, _ = O.align_batch(O.make_params(M, xdrop=40), b2)
    assert (err2 == 1).all() and (n2 == 0).all()                     # :323-329


def test_first_row_column_end_gap_rule():
    # tile 0, first row/column: match = sim + gapOpen + gapExtend*max(0, max(i,j)-1)  (:445-448).
    # A query that is a suffix of the reference must get leading 2s (gap in query), nothing else.
    rng = np.random.default_rng(5)
    s = "".join(rng.choice(list("ACGT"), size=300))
    aln, err, _ = run_pair(onehot(s), onehot(s[40:]))
    assert err == 0 and (aln[:40] == 2).all() and not aln[40:].any()


def test_psgp_matches_reference_formula():
    # alignment-helper.cpp:188-189: min(0.1*gapOpen, float(gapOpen*scale*((num-g)*1.0/num)))
    g = np.array([0.0, 1.0, 2.5, 3.999], dtype=np.float32)
    go, ge = synth._psgp(g, 4, -50.0, -5.0, 0.5)
    assert go[0] == -50.0 and ge[0] == -5.0
    assert go[1] == np.float32(min(np.float32(-5.0), np.float32(-25.0 * (3.0 / 4.0))))
    assert ge[2] == np.float32(min(np.float32(-1.0), np.float32(-5.0 * (1.5 / 4.0))))
    assert go[3] == np.float32(-5.0)      # tiny remaining fraction clamps to 0.1*gapOpen


@pytest.mark.parametrize("kind", ["nuc", "nuc_profiles", "prot", "small_marker", "err2", "err1"])
def test_reference_layout_restatement_equals_the_checker(kind):
    """oracle/talco_faithful.cpp (vector<vector<float>>, 14 new[] per tile, AVX2 masked loads -- the reference's layout and allocation
    pattern, timed by bench.py as the reference's own code) against the checker: paths, error codes, band cells."""
    from twilight_amd import synth

    pk = {}
    if kind == "prot":
        M, batch = synth.protein_matrix(), synth.make_level_batch(4, 300, P=22, members=((1, 5), (1, 5)), seed=5, sub=0.2)
    else:
        M = synth.nucleotide_matrix()
        members = (1, 1) if kind in ("nuc", "err2", "err1") else ((2, 6), (1, 4))
        batch = synth.make_level_batch(5, 700, members=members, seed=17, **({"sub": 0.75, "indel": 0.05} if kind == "err1" else {}))
        if kind == "small_marker": pk = dict(marker=100)
        if kind == "err2": pk = dict(flen=96)
        if kind == "err1": pk = dict(xdrop=40)
    p = O.make_params(M, **pk)
    a, n, e, st = O.align_batch(p, batch, threads=2)
    fa, fn, fe, cells = O.align_batch_faithful(p, batch, threads=2)
    assert np.array_equal(e, fe) and np.array_equal(n, fn)
    for i in range(batch.n_pairs):
        assert np.array_equal(a[i, : n[i]], fa[i, : fn[i]]), f"pair {i}"
    assert cells == st.cells
    if kind == "err2": assert (e == 2).any()
    if kind == "err1": assert (e == 1).any()


def _mt_case_names():
    import mt_cases
    return mt_cases.NAMES


@pytest.mark.parametrize("name", _mt_case_names())
def test_tiles_chained_from_the_corner_are_the_whole_pair(name):
    """twlo_tile_from is one tile as a function of its start.  Chained from (0, 0) over the pairs of tests/mt_cases.py it reproduces twlo_align_pair_exits: path,
    errorType, tiles, band cells, and the starts the exit hook reports."""
    import mt_cases
    c = mt_cases.case(name)
    p = O.make_params(c.matrix, **c.pk)
    for i in range(c.batch.n_pairs):
        if c.batch.len[i].min() < 1:
            continue
        pv = O.PairView(c.batch, i)
        aln, err, st, rows = O.pair_exits(p, pv)
        start, first, last, segs, cells, tiles, starts, e = (0, 0), True, False, [], 0, 0, [], 0
        while not last:
            start, last, e, cl, seg = O.tile_from(p, pv, start, first)
            cells += cl
            tiles += 1
            if e or seg.shape[0] == 0:      # (:94-97: a tile that leaves nothing ends the pair without a path)
                segs = []
                break
            segs.append(seg)
            starts.append(start)
            first = False
        path = np.concatenate(segs) if segs else np.zeros(0, dtype=np.int8)
        assert e == err and tiles == st.tiles and cells == st.cells, (name, i, e, err, tiles, st.tiles, cells, st.cells)
        assert np.array_equal(path, aln), (name, i, path.shape, aln.shape)
        if err == 0:
            assert starts == [(r, q) for (_t, _k, _s, r, q) in rows], (name, i)
            assert starts[-1][0] <= pv.R - 1 and starts[-1][1] <= pv.Q - 1
