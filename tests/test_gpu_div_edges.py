"""The fast division of the lean DP kernels (fast_div, talco_div.hip.h) at the corners of its guard, on every route (-m gpu).

The inputs come from tests/div_cases.py; tests/test_div_edge_inputs_cpu.py holds each of them to what it claims.

SCORES.  Every score case through twl_dp_column_scores -- the DUMP instantiation of talco_lean_kernel itself, so the hoisted-reciprocal
division as the DP runs it -- against the oracle's IEEE division (twlo_column_score): equal as floats in EVERY cell of the grid (the
kernels may return -0 where the oracle returns +0; nothing downstream can see that).  The band of a score case is the whole matrix, so
no cell may be missing from the dump.  This is the bit-for-bit comparison of the two forms of the division that the comment above
fast_div names: entries on 2^-20 and 2^30, scores and gap_char on 2^-10 and 2^10, denominators 1, 3, 7, 11, 21, 2^40, 2^40 as the
rounded product of (2^20 + 1)(2^20 - 1), the largest float below 2^40, numerators of 2^-73, 2^-72, 0 and -(483 x 2^70).

GUARD.  See the second half of this file."""
import numpy as np
import pytest

import div_cases as V
import dp_cases as D
import oracle_lib as O
from twilight_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture()
def knobs(gpu):
    gpu.set_knob(api.KNOB_THR_SMALL, 0)          # (also forgets what the levels of earlier tests found of the 512-row window)
    yield gpu
    gpu.set_knob(api.KNOB_THR_SMALL, 0)
    gpu.set_knob(api.KNOB_MT_WIDE, 1)
    gpu.set_knob(api.KNOB_MT_MAX_PAIRS, 1024)
    gpu.set_knob(api.KNOB_NO_SPEC, 0)
    gpu.set_knob(api.KNOB_PROT_CORRIDOR, 448)
    gpu.set_knob(api.KNOB_PROT_MODE, 0)
    gpu.set_knob(api.KNOB_ASSUME_ONEHOT_QUERY, 0)
    gpu.set_knob(api.KNOB_MT_MIN_MARKER, 512)


# ---- scores ----
_KERNEL_OF_MODE = {"nuc2": b"<6, 16, 1, 2, 1, false, true", "nuc2_leaf": b"<6, 16, 1, 2, 1, false, true", "nuc5": b"<6, 16, 1, 5, 1, false, true",
                   "nuc1": b"<6, 16, 1, 1, 1, false, true", "nuc0": b"<6, 16, 1, 0, 1, false, true", "prot3": b"<22, 16, 1, 3, 1, false, true"}


@pytest.mark.parametrize("case", V.SCORE_CASES, ids=lambda c: c.name)
def test_fast_division_matches_ieee_division_at_the_corners(knobs, case):
    if case.onehot_query:
        # single-sequence query sides: the device-resident level path tells the kernels; through this entry the test says so itself
        knobs.set_knob(api.KNOB_ASSUME_ONEHOT_QUERY, 1)
    b = case.batch()
    got = knobs.dp_column_scores(knobs.make_params(case.matrix, **case.params()), b, 0)
    st = knobs.get_stats(0)
    kernel = bytes(st.kernel).rstrip(b"\0")
    assert _KERNEL_OF_MODE[case.mode] in kernel and st.n_relaunched == 0, (kernel, st.n_relaunched)
    R, Q = case.ref.shape[0], case.qry.shape[0]
    assert got.shape == (Q, R)
    missing = np.argwhere(np.isnan(got))
    assert len(missing) == 0, f"{case.name}: {len(missing)} cells never visited, first {missing[0].tolist()}"
    op = O.make_params(case.matrix, **case.params())
    d = float(case.denom)
    want = np.array([[O.column_score(op, case.ref[j], case.qry[i], d) for j in range(R)] for i in range(Q)], dtype=np.float32)
    assert not np.isnan(want).any() and not np.isinf(want).any()
    for i, j, corner, _n in case.planned:
        print(f"{case.name} {corner} ({i}, {j}): kernel {float(got[i, j])!r} ({got[i, j].view(np.uint32):#010x}) oracle {float(want[i, j])!r} ({want[i, j].view(np.uint32):#010x})")
        assert got[i, j] == want[i, j], f"{case.name}: {corner} at ({i}, {j}): kernel {float(got[i, j])!r}, IEEE quotient {float(want[i, j])!r}"
    diff = np.argwhere(got != want)
    assert len(diff) == 0, (f"{case.name}: {len(diff)} of {got.size} cells differ from the IEEE quotient; first ({diff[0][0]}, {diff[0][1]}): "
                            f"kernel {float(got[tuple(diff[0])])!r} oracle {float(want[tuple(diff[0])])!r} numerator {float(case.numer()[tuple(diff[0])])!r} denominator {d!r}")


# ================================================================ the guard, route by route ================================================================
# A guard case (div_cases.GUARD_CASES) is a pool of dp_cases.py with ONE profile entry per carrying pair one float outside fast_div's range (or exactly on its
# limit: the twin), replicated to the level size of a route as in tests/test_gpu_dp_edges.py.  For every route:
#   * paths, lengths and error codes are the oracle's, band cells under the rule of test_gpu_dp_edges.run_case;
#   * the first kernel is the intended one;
#   * n_relaunched is EXACTLY (pairs that carry an outside entry) x (copies of the pool) and n_launches is 2 -- one more than without the entry: every pool here is
#     a margin pool of the route's own window (or a short pool that fits every window), which alone is not re-run (test_gpu_dp_edges holds that);
#   * the on-the-limit twin is not re-run at all: n_relaunched == 0, one launch.
# The routes on PRECOMPUTED scores (protein: 16 waves x 1 block, speculative teams, tile-parallel) load their scores; score_matrix_kernel divides the IEEE way and the DP
# kernel never sees the entry: parity, and nothing re-run for either twin (the corridor is off: a band cell outside it would be re-run for its own reason).
# On the TILE-PARALLEL nucleotide route re-runs are not counted pair by pair (tiles run from predicted starts): parity, n_relaunched >= the carrying pairs for the
# outside twin and == 0 for the limit twin.
_ORACLE = {}


def oracle_of(case):
    """(pool, paths, lengths, error codes, stats) of a guard case, computed once for all routes."""
    if case.name not in _ORACLE:
        pool = case.batch()
        oa, on, oerr, ost = O.align_batch(O.make_params(D.matrix_of(case.P), **case.params()), pool, threads=8)
        assert not oerr.any(), (case.name, oerr.tolist())
        for a in (oa, on, oerr):
            a.setflags(write=False)
        _ORACLE[case.name] = (pool, oa, on, oerr, ost)
    return _ORACLE[case.name]


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(twl, case, n_level, matrix=None, pk=None):
    """The pool replicated to `n_level` pairs (rounded up to whole pools) through twl_align_batch; parity with the oracle; returns (stats, copies of the pool)."""
    pool, oa, on, oerr, ost = oracle_of(case)
    k = pool.n_pairs
    reps = max(1, -(-n_level // k))
    idx = np.arange(reps * k) % k
    level = pool if reps == 1 else D.replicate(pool, idx)
    aln, ln, err = twl.align_batch(twl.make_params(D.matrix_of(case.P), **case.params()), level)
    st = twl.get_stats(0)
    assert np.array_equal(err, oerr[idx]), f"{case.name}: errorType gpu {err[:2 * k].tolist()} oracle {oerr.tolist()}"
    assert np.array_equal(ln, on[idx]), f"{case.name}: path length gpu {ln[:2 * k].tolist()} oracle {on.tolist()}"
    for j in range(k):      # replicated pairs against the pool's result
        same = (aln[idx == j, : on[j]] == oa[j, : on[j]]).all(axis=1)
        assert same.all(), f"{case.name}: path of pool pair {j} differs in {int((~same).sum())} of {reps} copies"
    assert st.band_cells == ost.cells * reps, f"{case.name}: band cells gpu {st.band_cells} oracle {ost.cells} x {reps}"      # (no pair fails, see oracle_of)
    return st, reps


SMALL, NOSPEC, NOMT, WIDE0 = (api.KNOB_THR_SMALL, 2), (api.KNOB_NO_SPEC, 1), (api.KNOB_MT_MAX_PAIRS, 0), (api.KNOB_MT_WIDE, 0)
NO768, WHOLE, TILES128 = (api.KNOB_THR_SMALL, 1), (api.KNOB_PROT_CORRIDOR, 0), (api.KNOB_MT_MIN_MARKER, 64)
# route -> (guard cases without the value suffix, knobs, pairs of the level as a function of the CU count, what the first kernel's name holds, how re-runs are counted)
#   "exact": the lean kernels read the entry.   "presim": the scores are precomputed, nothing is re-run.   "tiles": tile-parallel, at least the carrying pairs.
GUARD_ROUTES = {
    # nucleotide
    "thr512":        (("nuc8_first_tile",), (SMALL, NOMT, WIDE0), lambda cu: 5 * cu + 120, b"<6, 4, 2, 2, 5, false", "exact"),
    "thr768":        (("nuc12_last_ref_col",), (NO768, NOMT, WIDE0), lambda cu: 4 * cu + 80, b"<6, 4, 3, 2, 4, false", "exact"),
    "few16":         (("nuc16_first_tile", "nuc16_ref_first_tile", "nuc16_last_ref_col", "nuc16_last_query_row", "nuc16_gap_letter", "nuc16_tile_behind",
                       "short_nuc_hi", "short_nuc_denom", "short_nuc_denom_one"), (NOMT, NOSPEC, WIDE0), lambda cu: 12, b"<6, 16, 1, 2, 1, false", "exact"),
    "spec16":        (("nuc16_last_query_row", "nuc16_tile_behind", "short_nuc_hi", "short_nuc_denom"), (NOMT, WIDE0), lambda cu: 12, b"<6, 16, 1, 2, 1, true", "exact"),
    "spec_shared":   (("nuc16_gap_letter", "nuc16_last_ref_col", "short_nuc_denom"), (NOMT, WIDE0), lambda cu: cu // 2 + 9, b"<6, 8, 2, 2, 4, true", "exact"),
    # tile-parallel (marker 128: ten tiles per pair of 600 columns): the entry inside a tile behind the first (query row 333, the gap letter), and in the reference
    # column in which the path crosses the anti-diagonals the fourth tile can begin on (div_cases.WHERE, tile_boundary)
    "tiles":         (("short_nuc_tile_behind", "short_nuc_tile_boundary"), (TILES128,), lambda cu: 8, b"tile-parallel", "tiles"),
    # protein
    "prot_thr512":   (("prot8_gap_letter", "prot8_first_tile"), (), lambda cu: cu + 40, b"<22, 8, 1, 3, 4, false", "exact"),
    "prot_sparse16": (("prot16_last_query_row", "prot16_last_ref_col", "short_prot_hi", "short_prot_denom"), (NOMT, NOSPEC), lambda cu: cu // 2 + 8, b"<22, 16, 1, 3, 1, false", "exact"),
    "prot_plain16":  (("prot16_last_query_row", "short_prot_first_tile"), (NOMT, NOSPEC, WHOLE), lambda cu: 12, b"<22, 16, 1, 4, 1, false", "presim"),
    "prot_spec16":   (("short_prot_first_tile", "short_prot_hi"), (NOMT, WHOLE), lambda cu: 8, b"<22, 16, 1, 4, 1, true", "presim"),
    "prot_spec_shared": (("short_prot_first_tile",), (NOMT, WHOLE), lambda cu: cu // 2 + 8, b"<22, 8, 1, 4, 4, true", "presim"),
    "prot_tiles":    (("short_prot_tile_behind",), (TILES128, WHOLE), lambda cu: 8, b"tile-parallel", "presim"),
}


def _route_cases():
    out = []
    for route, spec in GUARD_ROUTES.items():
        for base in spec[0]:
            out += [(route, c.name) for c in V.GUARD_CASES if c.name.rsplit("-", 1)[0] == base]
    return out


@pytest.mark.parametrize("route,name", _route_cases())
def test_entry_at_the_limit_of_the_guard(knobs, route, name):
    _, kn, n_of, kernel, counting = GUARD_ROUTES[route]
    case = V.GUARD_BY_NAME[name]
    for key, value in kn:
        knobs.set_knob(key, value)
    st, reps = run_case(knobs, case, n_of(cus()))
    got = (bytes(st.kernel).rstrip(b"\0"), int(st.n_relaunched), int(st.n_launches))
    print(route, name, got, "copies", reps)
    assert kernel in got[0], got
    carrying = len(case.rerun) * reps
    if counting == "presim":
        assert st.matrix_mode == 4 and got[1] == 0, f"{route} {name}: precomputed scores, yet {got[1]} pairs re-run; {got[0]}"
    elif counting == "tiles":
        assert st.speculative == 3
        assert (got[1] >= carrying) if carrying else (got[1] == 0), f"{route} {name}: re-ran {got[1]} pairs, {carrying} carry an entry outside the range"
    else:
        assert got[1] == carrying and got[2] == (2 if carrying else 1), (f"{route} {name}: re-ran {got[1]} pairs in {got[2]} launches; {len(case.rerun)} pairs x {reps} copies "
                                                                          f"carry an operand outside the range; {got[0]}")


# ---- score twins: one score on the limit of fast_div_in_range and one float past it ----
@pytest.mark.parametrize("kind,score,lean", [("nuc", V.SCORE_HI, True), ("nuc", V.up(V.SCORE_HI), False), ("prot", V.SCORE_LO, True), ("prot", V.down(V.SCORE_LO), False)])
def test_score_at_the_limit_plans_the_lean_kernel_and_one_past_it_the_ieee_kernel(knobs, kind, score, lean):
    """The 8 pairs of 600 columns of the short pools.  Nucleotide: a match score of 2^10 (mode 2 keeps its structure) against the float above it; protein: the X / X score
    at 2^-10 against the float below it.  On the limit the level starts on a lean kernel (speculative teams of 16 waves), past it on the round-1 kernel with the IEEE
    division -- `general (IEEE division)` of the plan, which tests/test_policy_cpu.py only describes.  Same paths as the oracle either way."""
    pool = V.SHORT_POOLS["short_nuc" if kind == "nuc" else "short_prot"]
    if kind == "nuc":
        mat = V._mode2(score, -8.0, -4.0)
    else:
        mat = D.matrix_of(22).copy()
        mat[20, 20] = score
    assert V.score_ok(score) == lean
    b = pool.batch()
    oa, on, oerr, ost = O.align_batch(O.make_params(mat, **pool.params()), b, threads=8)
    aln, ln, err = knobs.align_batch(knobs.make_params(mat, **pool.params()), b)
    st = knobs.get_stats(0)
    kernel = bytes(st.kernel).rstrip(b"\0")
    assert np.array_equal(err, oerr) and np.array_equal(ln, on) and not oerr.any()
    assert all(np.array_equal(aln[i, : ln[i]], oa[i, : on[i]]) for i in range(b.n_pairs))
    assert st.band_cells == ost.cells and st.n_relaunched == 0
    want = (b"talco_lean_kernel<6, 16, 1, 2, 1, true" if kind == "nuc" else b"talco_lean_kernel<22, 16, 1, 4, 1, true") if lean else (b"talco_kernel<6, 8, 2," if kind == "nuc" else b"talco_kernel<22, 8, 2,")
    assert want in kernel, kernel


# ---- guard plus window ----
# The walk of the re-run ladder (twl_run.inc.hip, climb_ladder; twl_policy.inc.hip, next_rung) over the committed spans, with the tile-parallel rungs off
# (KNOB_MT_MAX_PAIRS 0, KNOB_MT_WIDE 0): on every round the pairs that carry the guard's code take the IEEE-division kernel of the guard rung (nucleotide 2048 rows,
# protein 1024) and stay on their level; then the pairs that outgrew a window take the next window rung.  A lean kernel reports the guard only for a pair whose
# FIRST tile fits its window (div_cases.TILE_SPANS: the entry sits in query row 10, which every kernel loads with the first tile, and a tile that outgrows its window ends
# with the window's code before the vote); the IEEE kernels (guard rung, 4608 rows, global memory) never report it.
_LADDER = {"From512": ("throughput 768", 12, True, "From768"), "From768": ("lean 1024", 16, True, "Mid"), "MidNuc": ("lean 2048", 32, True, "Wide"),
           "MidProt": ("protein 16-wave", 16, True, "Wide"), "Wide": ("wide 4608", 72, False, "Global")}


def walk(case, reps, first_nv, start, prot):
    """(pairs re-run, launches, the rungs in order) for a level of `reps` copies of the pool whose first launch is a lean kernel of `first_nv` blocks."""
    tiles = V.TILE_SPANS[case.pool]

    def outcome(pair, nv, lean):
        if tiles[pair][0] >= nv:
            return "window"                       # (the first tile holds the pair's widest band)
        if lean and pair in case.rerun:
            return "guard"
        assert max(tiles[pair]) < nv
        return "ok"

    state = [outcome(p, first_nv, True) for p in range(len(tiles))]
    rerun, launches, rungs, at = 0, 1, [], start
    while at != "Global":
        guard = [p for p, s in enumerate(state) if s == "guard"]
        redo = guard or [p for p, s in enumerate(state) if s == "window"]
        if not redo:
            break
        if guard:
            name, nv, lean, nxt = "guard (IEEE division)", (16 if prot else 32), False, at
        else:
            name, nv, lean, nxt = _LADDER[("MidProt" if prot else "MidNuc") if at == "Mid" else at]
        for p in redo:
            state[p] = outcome(p, nv, lean)
        rerun += len(redo) * reps
        launches += 1
        rungs.append(name)
        at = nxt
    left = [p for p, s in enumerate(state) if s != "ok"]
    if left:
        rerun += len(left) * reps; launches += 1; rungs.append("global")
    return rerun, launches, tuple(rungs)


# route -> (guard case, knobs, pairs of the level, first kernel, NV of the first launch, level the ladder starts on, protein; the walk's result: pairs re-run per copy, launches, rungs)
WINDOW_ROUTES = {
    # few16 hands both pairs on (spans 31 and 32 >= 16); lean 2048 fits pair 0 and reports its entry, pair 1 outgrows it; the guard rung takes pair 0, wide 4608 pair 1
    "nuc32_over_p0-below_lo": ((NOMT, NOSPEC, WIDE0), lambda cu: 2, b"<6, 16, 1, 2, 1, false", 16, "Mid", False, (4, 4, ("lean 2048", "guard (IEEE division)", "wide 4608"))),
    "nuc32_over_p0-lo":       ((NOMT, NOSPEC, WIDE0), lambda cu: 2, b"<6, 16, 1, 2, 1, false", 16, "Mid", False, (3, 3, ("lean 2048", "wide 4608"))),
    # the entry in the pair that outgrows every lean window: no lean kernel ever finishes its first tile, the guard's code never appears, the 4608-row IEEE kernel takes it
    "nuc32_over_p1-below_lo": ((NOMT, NOSPEC, WIDE0), lambda cu: 2, b"<6, 16, 1, 2, 1, false", 16, "Mid", False, (3, 3, ("lean 2048", "wide 4608"))),
    "nuc72_margin_p1-below_lo": ((NOMT, NOSPEC, WIDE0), lambda cu: 2, b"<6, 16, 1, 2, 1, false", 16, "Mid", False, (4, 3, ("lean 2048", "wide 4608"))),
    # the whole ladder from the 512-row throughput window: 768 and 1024 rows (every pair outgrows 512 and 768), then the guard rung for pair 1
    "nuc16_margin_p1-below_lo": ((SMALL, NOMT, WIDE0), lambda cu: 5 * cu + 120, b"<6, 4, 2, 2, 5, false", 8, "From512", False, (7, 4, ("throughput 768", "lean 1024", "guard (IEEE division)"))),
    # protein: the 512-row throughput window hands every pair on; the 16-wave kernel reports pair 1's entry and is outgrown by pair 0; guard rung (1024 rows), then 4608 rows
    "prot16_over_p1-below_lo": ((), lambda cu: cu + 40, b"<22, 8, 1, 3, 4, false", 8, "Mid", True, (5, 4, ("protein 16-wave", "guard (IEEE division)", "wide 4608"))),
    "prot16_over_p1-lo":       ((), lambda cu: cu + 40, b"<22, 8, 1, 3, 4, false", 8, "Mid", True, (4, 3, ("protein 16-wave", "wide 4608"))),
    # ... and from the 16-wave first launch: pair 0 (span 16) outgrows it in its first tile, before the vote: as without the entry
    "prot16_over_p0-below_lo": ((NOMT, NOSPEC), lambda cu: cu // 2 + 8, b"<22, 16, 1, 3, 1, false", 16, "Wide", True, (1, 2, ("wide 4608",))),
}


@pytest.mark.parametrize("name", list(WINDOW_ROUTES))
def test_guarded_entry_in_a_pair_that_outgrows_its_window(knobs, name):
    kn, n_of, kernel, first_nv, start, prot, table = WINDOW_ROUTES[name]
    case = V.GUARD_BY_NAME[name]
    for key, value in kn:
        knobs.set_knob(key, value)
    st, reps = run_case(knobs, case, n_of(cus()))
    rerun, launches, rungs = walk(case, reps, first_nv, start, prot)
    assert (rerun, launches, rungs) == (table[0] * reps, table[1], table[2]), f"{name}: the walk gives {rerun // reps} re-runs per copy in {launches} launches over {rungs}, the table says {table}"
    got = (bytes(st.kernel).rstrip(b"\0"), int(st.n_relaunched), int(st.n_launches))
    print(name, got, "copies", reps, "walk", rerun, launches, rungs)
    assert kernel in got[0], got
    assert got[1] == rerun and got[2] == launches, f"{name}: re-ran {got[1]} pairs in {got[2]} launches, the walk gives {rerun} in {launches}: {rungs}; {got[0]}"
