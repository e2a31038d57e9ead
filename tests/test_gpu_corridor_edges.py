"""The corridor of the precomputed protein scores where a band meets its edge (-m gpu).  Inputs: tests/corridor_cases.py, held to what they claim by
tests/test_corridor_edge_inputs_cpu.py.  Every comparison is exact: floats as floats (-0 equals +0, as test_column_scores_match_oracle allows), integers as integers.

THE MATRIX.  score_matrix_kernel's output of every pair of a level, read back through twl_dp_score_matrix and held cell by cell to the oracle's column score in
the tiles the restated rule keeps and to NaN in the tiles it drops.
THE EDGE.  Every pool at knob c* and c* - 1 of every distinct smallest safe corridor c* of its pairs, on the four routes that run on precomputed scores.
NO CORRIDOR behind the round-1 kernel, which does not check what it reads.
THE PASS REMEMBERS a lost corridor for levels of at most as many pairs, and forgets when the knob is set."""
import numpy as np
import pytest

import corridor_cases as K
import div_cases as V
import dp_cases as D
import oracle_lib as O
from twilight_amd import api

pytestmark = pytest.mark.gpu
M22 = D.matrix_of(22)


@pytest.fixture()
def knobs(gpu):
    gpu.set_knob(api.KNOB_THR_SMALL, 0)          # (also forgets what the levels of earlier tests found of the 512-row window)
    gpu.set_knob(api.KNOB_PROT_CORRIDOR, 448)    # (... and of the corridor)
    yield gpu
    gpu.set_knob(api.KNOB_THR_SMALL, 0)
    gpu.set_knob(api.KNOB_MT_WIDE, 1)
    gpu.set_knob(api.KNOB_MT_MAX_PAIRS, 1024)
    gpu.set_knob(api.KNOB_NO_SPEC, 0)
    gpu.set_knob(api.KNOB_PROT_CORRIDOR, 448)
    gpu.set_knob(api.KNOB_PROT_MODE, 0)
    gpu.set_knob(api.KNOB_ASSUME_ONEHOT_QUERY, 0)
    gpu.set_knob(api.KNOB_MT_MIN_MARKER, 512)


NOSPEC, NOMT, TILES128 = (api.KNOB_NO_SPEC, 1), (api.KNOB_MT_MAX_PAIRS, 0), (api.KNOB_MT_MIN_MARKER, 64)
PLAIN16 = b"<22, 16, 1, 4, 1, false"


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def corridor(twl, value):
    """Sets the knob -- which also makes the device forget what earlier levels found."""
    twl.set_knob(api.KNOB_PROT_CORRIDOR, value)


def parity(tag, got, want, idx=None):
    """Paths, lengths and error codes of a level against the oracle's of its pool (idx: the pool pair of every level pair)."""
    aln, ln, err = got
    oa, on, oerr = want
    idx = np.arange(len(on)) if idx is None else idx
    assert np.array_equal(err, oerr[idx]), f"{tag}: errorType gpu {err.tolist()} oracle {oerr[idx].tolist()}"
    assert np.array_equal(ln, on[idx]), f"{tag}: path length gpu {ln.tolist()} oracle {on[idx].tolist()}"
    for n, j in enumerate(idx):
        assert np.array_equal(aln[n, : ln[n]], oa[j, : on[j]]), f"{tag}: path of pair {n} (pool pair {j}) differs"


# ================================================================ the matrix, cell by cell ================================================================
def expected_matrix(b, i, pk):
    """([R + Q][pitch] float32 of the oracle's scores laid out [K][I], the mask of the floats that are cells)."""
    R, Q = int(b.len[i, 0]), int(b.len[i, 1])
    g = O.column_score_grid(O.make_params(M22, **pk), b.freq[i, 0, :R], b.freq[i, 1, :Q], float(np.float32(b.num[i, 0]) * np.float32(b.num[i, 1])))      # [Q][R]
    cells = K.cell_mask(R, Q)
    want = np.zeros(cells.shape, dtype=np.float32)
    kk, ii = np.nonzero(cells)
    want[kk, ii] = g[ii, kk - ii]
    return want, cells


@pytest.mark.parametrize("lv,knob", [(lv, knob) for lv in K.LEVELS for knob in lv.knobs()], ids=lambda v: v.name if isinstance(v, K.MatrixLevel) else str(v))
def test_score_matrix_cell_by_cell(knobs, lv, knob):
    """Every cell (I < Q, 0 <= K - I < R) of every pair of the level: the oracle's column score in a tile the restated rule keeps, NaN in a tile it drops, no NaN at
    knob 0.  Floats outside the matrix are not looked at.  A level of the same shapes from another seed runs first, so a tile the kernel did not write would hold that
    level's scores (or its NaN), not this one's.  The pairs whose band reads a NaN are finished by the ladder: parity with the oracle holds as well.
    Knob values: 64, 0, and per level the two values at which a tile sits exactly on the limit of the rule, on either side of the line, and one row less
    (corridor_cases.MatrixLevel.edge_knobs): there a `>` that became `>=`, or an `ic` that moved, changes which tiles hold NaN."""
    for key, value in (NOMT, NOSPEC):
        knobs.set_knob(key, value)
    pk = lv.params()
    p = knobs.make_params(M22, **pk)
    other, b = lv.batch(2), lv.batch(1)
    corridor(knobs, 0)             # (the level before fills the WHOLE buffer with another seed's scores: a kept tile left unwritten shows those, a dropped tile left unfilled shows finite floats)
    knobs.align_batch(p, other)
    corridor(knobs, knob)
    got = knobs.align_batch(p, b)
    st = knobs.get_stats(0)
    assert PLAIN16 in bytes(st.kernel) and st.matrix_mode == 4, bytes(st.kernel)
    oa, on, oerr, ost = O.align_batch(O.make_params(M22, **pk), b, threads=4)
    parity(lv.name, got, (oa, on, oerr))
    n_nan = 0
    for i, (R, Q) in enumerate(lv.shapes):
        sim, used = knobs.dp_score_matrix(i)
        assert used == knob and sim.shape == (R + Q, K.pitch_of(Q)), (lv.name, i, used, sim.shape)
        want, cells = expected_matrix(b, i, pk)
        drop = K.nan_cells(R, Q, knob) & cells
        keep = cells & ~drop
        n_nan += int(drop.sum())
        bad = np.argwhere(keep & ~(sim == want))
        assert len(bad) == 0, (f"{lv.name} pair {i} ({R} x {Q}) knob {knob}: {len(bad)} of {int(keep.sum())} kept cells differ from the oracle; first K {bad[0][0]} I {bad[0][1]}: "
                               f"kernel {float(sim[tuple(bad[0])])!r} oracle {float(want[tuple(bad[0])])!r}")
        bad = np.argwhere(drop & ~np.isnan(sim))
        assert len(bad) == 0, f"{lv.name} pair {i} ({R} x {Q}) knob {knob}: {len(bad)} of {int(drop.sum())} cells of dropped tiles are not NaN; first K {bad[0][0]} I {bad[0][1]}: {float(sim[tuple(bad[0])])!r}"
    assert (n_nan > 0) == (knob > 0), (lv.name, knob, n_nan)
    print(lv.name, "knob", knob, "NaN cells", n_nan, "re-run", int(st.n_relaunched))


def test_score_matrix_read_back_refuses_what_it_cannot_answer(knobs):
    """TWL_ERR_UNSUPPORTED (-4) after a call that did not precompute (a nucleotide level; twl_column_scores, which overwrites the buffer) and for a pair that did not run;
    TWL_ERR_BAD_ARGUMENT (-2) for a pair the call did not have or a device that was not selected."""
    import ctypes as C

    from twilight_amd import synth

    lib = api.load_library()
    dm = api.TwlScoreDims()

    def rc(pair, device=0):
        return lib.twl_dp_score_matrix(C.c_int(device), C.c_int32(pair), C.byref(dm), None)

    for key, value in (NOMT, NOSPEC):
        knobs.set_knob(key, value)
    corridor(knobs, 0)
    lv = K.LEVEL_BY_NAME["k_mod64"]
    b = lv.batch(1)
    b.len[1, 1] = 0                                     # a pair that does not run
    knobs.align_batch(knobs.make_params(M22, **lv.params()), b)
    assert rc(0) == 0 and (dm.R, dm.Q, dm.pitch, dm.corridor) == (312, 200, 256, 0)
    assert rc(1) == -4 and rc(3) == -2 and rc(-1) == -2 and rc(0, device=7) == -2
    knobs.column_scores(knobs.make_params(M22), b.freq[0, 0, :50], b.freq[0, 1, :40], 1, 1)
    assert rc(0) == -4
    knobs.align_batch(knobs.make_params(M22, **lv.params()), b)
    assert rc(2) == 0
    nb = synth.make_level_batch(2, 200, members=((1, 4), (1, 4)), seed=3)
    knobs.align_batch(knobs.make_params(synth.nucleotide_matrix()), nb)
    assert rc(0) == -4


# ================================================================ the edge of the corridor, route by route ================================================================
# route -> (knobs, pairs of the level as a function of the CU count, what the first kernel's name holds, re-runs counted exactly): GUARD_ROUTES of
# tests/test_gpu_div_edges.py without WHOLE.
EDGE_ROUTES = {
    "prot_plain16":     ((NOMT, NOSPEC), lambda cu: 12, PLAIN16, True),
    "prot_spec16":      ((NOMT,), lambda cu: 8, b"<22, 16, 1, 4, 1, true", False),
    "prot_spec_shared": ((NOMT,), lambda cu: cu // 2 + 8, b"<22, 8, 1, 4, 4, true", False),
    "prot_tiles":       ((TILES128,), lambda cu: 8, b"tile-parallel", False),
}
_ORACLE = {}


def oracle_of(pool):
    """(batch, paths, lengths, error codes, stats) of a pool, computed once for all routes and left unchanged."""
    if pool.name not in _ORACLE:
        b = pool.batch()
        oa, on, oerr, ost = O.align_batch(O.make_params(M22, **pool.params()), b, threads=8)
        assert not oerr.any(), (pool.name, oerr.tolist())
        for a in (oa, on, oerr):
            a.setflags(write=False)
        _ORACLE[pool.name] = (b, oa, on, oerr, ost)
    return _ORACLE[pool.name]


def level_of(pool, n_level):
    """The pool replicated to `n_level` pairs (rounded up to whole pools): (level, pool pair of every level pair, copies)."""
    b = oracle_of(pool)[0]
    k = b.n_pairs
    reps = max(1, -(-n_level // k))
    idx = np.arange(reps * k) % k
    return (b if reps == 1 else D.replicate(b, idx)), idx, reps


def run_level(twl, pool, level, idx, reps):
    """The level through twl_align_batch: parity of paths, lengths, error codes and band cells with the oracle; returns the stats."""
    _b, oa, on, oerr, ost = oracle_of(pool)
    got = twl.align_batch(twl.make_params(M22, **pool.params()), level)
    st = twl.get_stats(0)
    parity(pool.name, got, (oa, on, oerr), idx)
    assert st.band_cells == ost.cells * reps, f"{pool.name}: band cells gpu {st.band_cells} oracle {ost.cells} x {reps}"      # (no pair fails, see oracle_of)
    return st


@pytest.mark.parametrize("route,name", [(r, p.name) for p in K.POOLS for r in p.routes])
def test_band_at_the_edge_of_the_corridor(knobs, route, name):
    """The knob at c* and at c* - 1 of every distinct c* of the pool, and at the longest Q of the pool.  Parity with the oracle at every value.  The pairs the restated
    rule hands back are those with 0 < knob < c* (corridor_cases.handed_back).

    On `prot_plain16` every tile starts where the one before ended, so the band cells the kernel reads are the oracle's: n_relaunched is EXACTLY the handed-back pairs
    times the copies of the pool, in one more launch (the guard rung; every pool fits its window).  On the speculative and the tile-parallel routes the count is a LOWER
    BOUND: tiles also start from guessed positions and read scores the true path never visits, and talco_lean_kernel keeps the verdict per PAIR (`guardBad` is
    declared in front of the tile loop and a speculative tile that is restarted from the true start does not clear it), so a NaN a wrong guess read hands the pair
    back all the same.  A knob of at least the longest Q of the pool drops no tile (the CPU test proves it): nothing is re-run on any route."""
    kn, n_of, kernel, exact = EDGE_ROUTES[route]
    pool = K.POOL_BY_NAME[name]
    for key, value in kn:
        knobs.set_knob(key, value)
    level, idx, reps = level_of(pool, n_of(cus()))
    longest = pool.longest_q(oracle_of(pool)[0])
    for value in pool.knob_values() + [longest]:
        corridor(knobs, value)          # (and forget what the value before lost)
        st = run_level(knobs, pool, level, idx, reps)
        got = (bytes(st.kernel).rstrip(b"\0"), int(st.n_relaunched), int(st.n_launches))
        want = len(K.handed_back(pool.cstar, value)) * reps
        print(route, name, "knob", value, got, "copies", reps, "predicted", want)
        assert kernel in got[0] and st.matrix_mode == 4, got
        if value >= longest:
            assert want == 0 and got[1] == 0, f"{route} {name}: knob {value} covers every matrix, yet {got[1]} pairs re-run"
        elif exact:
            assert got[1] == want and got[2] == (2 if want else 1), f"{route} {name} knob {value}: re-ran {got[1]} pairs in {got[2]} launches; c* {pool.cstar} x {reps} copies predict {want}"
        else:
            assert got[1] >= want, f"{route} {name} knob {value}: re-ran {got[1]} pairs; c* {pool.cstar} x {reps} copies predict at least {want}"


# ================================================================ no corridor behind a kernel that does not check ================================================================
def test_no_corridor_behind_the_round1_kernel(knobs):
    """The X / X score one float below 2^-10 (the protein score twin of div_cases.py) is outside fast_div_in_range: with KNOB_PROT_MODE presim the level runs the round-1
    kernel on precomputed scores, which does not test what it loads -- so the plan must not hand it a corridor, whatever the knob says."""
    pool = V.SHORT_POOLS["short_prot"]
    mat = M22.copy()
    mat[20, 20] = V.down(V.SCORE_LO)
    assert not V.score_ok(mat[20, 20])
    corridor(knobs, 64)
    knobs.set_knob(api.KNOB_PROT_MODE, api.PROT_MODES["presim"])
    b = pool.batch()
    p = knobs.make_params(mat, **pool.params())
    plan = api.plan_describe(p, b.len, num_cu=cus())
    assert plan.startswith("general (IEEE division); mode 4") and plan.endswith("corridor 0"), plan
    oa, on, oerr, ost = O.align_batch(O.make_params(mat, **pool.params()), b, threads=8)
    got = knobs.align_batch(p, b)
    st = knobs.get_stats(0)
    parity("round-1 presim", got, (oa, on, oerr))
    assert not oerr.any() and st.band_cells == ost.cells
    assert b"talco_kernel<22, 8, 2," in bytes(st.kernel) and st.matrix_mode == 4 and st.n_relaunched == 0, (bytes(st.kernel), st.matrix_mode, st.n_relaunched)
    for i in range(b.n_pairs):
        sim, used = knobs.dp_score_matrix(i)
        cells = K.cell_mask(int(b.len[i, 0]), int(b.len[i, 1]))
        assert used == 0 and not np.isnan(sim[cells]).any(), (i, used)
    # the contrast: the lean kernel on precomputed scores, scores within the range, is planned with the knob's corridor
    knobs.set_knob(api.KNOB_PROT_MODE, api.PROT_MODES["lean_presim"])
    assert api.plan_describe(knobs.make_params(M22, **pool.params()), b.len, num_cu=cus()).endswith("corridor 64")


# ================================================================ the pass remembers ================================================================
def test_pass_remembers_a_lost_corridor_until_a_larger_level_or_the_knob(knobs):
    """`skew700` on prot_plain16 with the knob one below the c* of its cut pair.  twl_plan_describe plans without a device and so without a device's memory (its
    memory argument carries nothing of the corridor): it says `corridor <knob>` throughout, and what the device actually handed score_matrix_kernel is what
    twl_dp_score_matrix reports -- that is the value held to 0 here where the issue names plan_describe.
      1. the first level (12 pairs) runs in the corridor and re-runs the copies of pair 1;
      2. the same level again: corridor 0, nothing re-run, no NaN in the read-back;  2b. a smaller level (8 pairs): likewise;
      3. a larger level (16 pairs) is another pass: the corridor again, its copies of pair 1 re-run;  3b. and loses it again;
      4. setting the knob forgets: the same 16 pairs run in the corridor again."""
    for key, value in (NOMT, NOSPEC):
        knobs.set_knob(key, value)
    pool = K.POOL_BY_NAME["skew700"]
    knob = max(pool.cstar) - 1
    assert K.handed_back(pool.cstar, knob) == [1]
    corridor(knobs, knob)
    p = knobs.make_params(M22, **pool.params())

    def step(n_level, want_corridor, tag):
        level, idx, reps = level_of(pool, n_level)
        assert api.plan_describe(p, level.len, num_cu=cus()).endswith(f"corridor {knob}")
        st = run_level(knobs, pool, level, idx, reps)
        assert PLAIN16 in bytes(st.kernel), bytes(st.kernel)
        sim, used = knobs.dp_score_matrix(1)          # pool pair 1: the one that leaves the corridor
        cells = K.cell_mask(int(level.len[1, 0]), int(level.len[1, 1]))
        print(tag, "pairs", level.n_pairs, "corridor used", used, "re-run", int(st.n_relaunched), "launches", int(st.n_launches), "NaN cells", int(np.isnan(sim[cells]).sum()))
        assert used == want_corridor, f"{tag}: the level ran with corridor {used}"
        if want_corridor:
            assert st.n_relaunched == reps and st.n_launches == 2 and np.isnan(sim[cells]).any(), (tag, st.n_relaunched, st.n_launches)
        else:
            assert st.n_relaunched == 0 and st.n_launches == 1 and not np.isnan(sim[cells]).any(), (tag, st.n_relaunched, st.n_launches)

    step(12, knob, "1 first level")
    step(12, 0, "2 same level again")
    step(8, 0, "2b smaller level")
    step(16, knob, "3 larger level")
    step(16, 0, "3b same again")
    corridor(knobs, knob)
    step(16, knob, "4 after setting the knob")
