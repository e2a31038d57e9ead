"""The DP kernels where the band meets the edge of a row window (talco_nuc.hip.h, talco_kernel.hip.h, talco_global.hip.h), through the C ABI (-m gpu).

The cases come from tests/dp_cases.py (every X-drop searched on the CPU; tests/test_dp_edge_inputs_cpu.py holds each case to its class):
MARGIN pools keep every pair's band within the last two 64-row blocks of a window of NV blocks -- past fcap = 64 * (NV - 2), the
wide-band branch of talco_lean_kernel, without leaving the window -- and JUST-OVER pools push one pair to a span of NV blocks exactly.
Each route below sends a pool (replicated where the route needs a level of more pairs than CUs) to the geometry whose window it is
about, with the existing knobs and pair counts only (twl_policy.inc.hip), and asserts

* paths, lengths and error codes are the oracle's bit for bit, band cells under the rule of tests/test_gpu_mt.py;
* the first kernel is the intended one and the ladder took as many launches as predicted (twl_stats.kernel names the FIRST launch only: on the
  `rung_*` routes the rung under test is not named by it but follows from next_rung in twl_policy.inc.hip, and is held by the launch count and
  by n_relaunched -- every pair of the pool outgrows the windows in front of that rung, and only the predicted ones outgrow the rung itself);
* twl_stats.n_relaunched is EXACTLY the number of pairs the CPU predicate (span >= NV, dp_cases.PairTrace.outgrows) says each window
  on the way hands back -- 0 for a margin pool on its own window: a spurious re-run shows here, a missed one as a wrong path;
* on the tile-parallel route (3072 rows) a tile that outgrows its window is computed in line instead: parity, and for just-over
  n_relaunched + mt_tiles_inline > 0.

Nothing is searched here and the trace is not recomputed: the spans are the committed ones."""
import numpy as np
import pytest

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
    gpu.set_knob(api.KNOB_FORCE_GLOBAL, 0)


_ORACLE = {}


def oracle_of(case):
    """(pool, paths, lengths, error codes, stats) of a case, computed once for all routes."""
    if case.name not in _ORACLE:
        pool = case.batch()
        oa, on, oerr, ost = O.align_batch(O.make_params(D.matrix_of(case.P), **case.params()), pool, threads=8)
        assert tuple(int(e) for e in oerr) == case.expected_errs(), (case.name, oerr.tolist())
        for a in (oa, on, oerr):
            a.setflags(write=False)
        _ORACLE[case.name] = (pool, oa, on, oerr, ost)
    return _ORACLE[case.name]


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(twl, case, n_level):
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
        assert same.all(), f"{case.name}: path of pool pair {j} differs in {int((~same).sum())} of {reps} copies (first: level pair {int(np.flatnonzero(idx == j)[np.argmin(same)])})"
    if np.all(oerr == 0) or st.n_relaunched == 0:      # (band cells of failed pairs count as well; only attempts in a window that was outgrown do not)
        assert st.band_cells == ost.cells * reps, f"{case.name}: band cells gpu {st.band_cells} oracle {ost.cells} x {reps}"
    return st, reps


def predicted(case, reps, ladder):
    """(pairs re-run, launches) when the windows of `ladder` (NV of the first launch, then of every rung) take the level in turn; what
    outgrows the last register window goes on to the global-memory kernel, which counts as a re-run as well."""
    rerun, launches = 0, 1
    for nv in ladder:
        c = sum(1 for s in case.spans if s >= nv) * reps
        if c == 0:
            break
        rerun += c
        launches += 1
    return rerun, launches


# route -> (cases, knobs, pairs of the level as a function of the CU count, what the first kernel's name holds, NV of the first launch and of the rungs behind it)
# KNOB_MT_WIDE 0 on the routes that count: a re-run set whose summed length reaches 3 markers per pair would take the tile-parallel 3072-row rung instead of
# `lean 2048`, and the pools of 1500 columns sit right on that line.  KNOB_MT_MAX_PAIRS 0 / KNOB_NO_SPEC 1: no tile-parallel first launch, remainder or rung, no speculative teams.
SMALL, NOSPEC, NOMT, WIDE0 = (api.KNOB_THR_SMALL, 2), (api.KNOB_NO_SPEC, 1), (api.KNOB_MT_MAX_PAIRS, 0), (api.KNOB_MT_WIDE, 0)
NO768, WHOLE = (api.KNOB_THR_SMALL, 1), (api.KNOB_PROT_CORRIDOR, 0)
ROUTES = {
    # nucleotide
    "thr512":        (("nuc8_margin", "nuc8_over", "nuc_flen455", "nuc_flen454"), (SMALL, NOMT, WIDE0), lambda cu: 5 * cu + 120, b"<6, 4, 2, 2, 5, false", (8, 12, 16, 32, 72)),
    "thr768":        (("nuc12_margin", "nuc12_over"), (NO768, NOMT, WIDE0), lambda cu: 4 * cu + 80, b"<6, 4, 3, 2, 4, false", (12, 16, 32, 72)),
    "rung_lean1024": (("nuc16_margin", "nuc16_over"), (NO768, NOMT, WIDE0), lambda cu: 4 * cu + 80, b"<6, 4, 3, 2, 4, false", (12, 16, 32, 72)),
    "few16":         (("nuc16_margin", "nuc16_over"), (NOMT, NOSPEC, WIDE0), lambda cu: 12, b"<6, 16, 1, 2, 1, false", (16, 32, 72)),
    "spec16":        (("nuc16_margin", "nuc16_over"), (NOMT, WIDE0), lambda cu: 12, b"<6, 16, 1, 2, 1, true", (16, 32, 72)),
    "spec_shared":   (("nuc16_margin", "nuc16_over"), (NOMT, WIDE0), lambda cu: cu // 2 + 9, b"<6, 8, 2, 2, 4, true", (16, 32, 72)),
    "rung_lean2048": (("nuc32_margin", "nuc32_over"), (NOMT, NOSPEC, WIDE0), lambda cu: 2, b"<6, 16, 1, 2, 1, false", (16, 32, 72)),
    "rung_wide4608": (("nuc72_margin", "nuc72_over"), (NOMT, NOSPEC, WIDE0), lambda cu: 2, b"<6, 16, 1, 2, 1, false", (16, 32, 72)),
    # protein
    "prot_thr512":   (("prot8_margin", "prot8_over", "prot_flen308", "prot_flen307"), (), lambda cu: cu + 40, b"<22, 8, 1, 3, 4, false", (8, 16, 72)),
    "rung_prot16":   (("prot16_margin", "prot16_over"), (), lambda cu: cu + 40, b"<22, 8, 1, 3, 4, false", (8, 16, 72)),
    "prot_plain16":  (("prot16_margin", "prot16_over"), (NOMT, NOSPEC, WHOLE), lambda cu: 12, b"<22, 16, 1, 4, 1, false", (16, 72)),
    "prot_sparse16": (("prot16_margin", "prot16_over", "prot_flen308", "prot_flen307"), (NOMT, NOSPEC), lambda cu: cu // 2 + 8, b"<22, 16, 1, 3, 1, false", (16, 72)),
    "prot_r1":       (("prot8_margin", "prot8_over", "prot_flen308", "prot_flen307"), ((api.KNOB_PROT_MODE, api.PROT_MODES["r1"]),), lambda cu: 12, b"talco_kernel<22, 8, 1,", (8, 72)),
}


@pytest.mark.parametrize("route,name", [(r, c) for r, spec in ROUTES.items() for c in spec[0]])
def test_band_at_the_edge_of_a_window(knobs, route, name):
    _, kn, n_of, kernel, ladder = ROUTES[route]
    case = D.BY_NAME[name]
    for key, value in kn:
        knobs.set_knob(key, value)
    st, reps = run_case(knobs, case, n_of(cus()))
    rerun, launches = predicted(case, reps, ladder)
    got = (bytes(st.kernel).rstrip(b"\0"), int(st.n_relaunched), int(st.n_launches))
    assert kernel in got[0], got
    if case.kind == "margin" and case.nv == ladder[0]:
        assert rerun == 0
    assert got[1] == rerun and got[2] == launches, f"{route} {name}: re-ran {got[1]} pairs in {got[2]} launches, predicted {rerun} in {launches} (spans {case.spans} x {reps}, windows {ladder}); {got[0]}"


@pytest.mark.parametrize("name", ["nuc48_margin", "nuc48_over"])
def test_band_at_the_edge_of_the_tile_parallel_3072_row_window(knobs, name):
    """12 pairs of 3500 columns (more than 8: the streak memory of small calls plays no part) with every knob at its default: tile-parallel, on the 1024-row stitch
    window first or -- when most pairs of the level before went wide -- on the 3072-row one at once; either way the 3072-row tiles and stitch take every pair, and the
    one that outgrows them goes on to the 4608-row kernel.  Tiles run from predicted starts, so re-runs are not counted pair by pair here."""
    case = D.BY_NAME[name]
    st, reps = run_case(knobs, case, 12)
    kernel = bytes(st.kernel).rstrip(b"\0")
    assert st.speculative == 3 and (b"<6, 16, 1, 2, 1, false, false, 2 / 1 / 3>" in kernel or b"<6, 16, 3, 2, 1, false, false, 2 / 1 / 3>" in kernel), kernel
    wide_first = b"<6, 16, 3," in kernel
    if case.kind == "over":
        assert st.n_relaunched + st.mt_tiles_inline > 0, (st.n_relaunched, st.mt_tiles_inline)
    elif wide_first:      # started on the 3072-row window: a margin pool never leaves it
        assert st.n_relaunched == 0, st.n_relaunched
    else:                 # started on the 1024-row stitch window, which spans of 47 blocks outgrow: the 3072-row rung took them
        assert st.n_relaunched > 0, st.n_relaunched


@pytest.mark.parametrize("name", ["nuc_flen455", "nuc_flen454", "prot_flen308", "prot_flen307"])
def test_flen_stop_on_the_global_memory_kernel(knobs, name):
    """The kernel without a window: flen equal to the widest band passes, one less stops that pair with errorType 2."""
    case = D.BY_NAME[name]
    knobs.set_knob(api.KNOB_FORCE_GLOBAL, 1)
    st, _ = run_case(knobs, case, case.n)
    assert b"talco_global_kernel" in bytes(st.kernel) and st.n_relaunched == 0, (st.kernel, st.n_relaunched)
