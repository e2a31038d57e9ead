"""The tile exit and the traceback walk of every DP kernel, branch by branch, through the C ABI (-m gpu).

talco_kernel.hip.h and talco_global.hip.h share the reference's tile exit (TALCO-XDrop.cpp:615-682) and the steps of its traceback
(:134-231) through talco_exit.hip.h, each with its own fetch of CS[last_k][0] and of a pointer nibble and its own walk loop;
talco_nuc.hip.h restates them.  Every kernel is sent every pool.  The pools come from tests/exit_cases.py: every exit kind and start state on tile 0 and on later tiles, pairs that
end on each residue of `last_k mod 8` in front of the marker and on the diagonals around it, trailing runs short and long, border exits,
runs that leave a 64-row x 16-group patch through its rows and through its groups, and the markers 2, 3, 7, 8, 9, 1023 and 1024.
tests/test_exit_edge_inputs_cpu.py holds each pool to the exits it claims; here every pool of a family goes down every route of that
family (knob tuples, level sizes and kernel-name fragments are test_gpu_dp_edges.ROUTES', imported), once, and the test asserts

* paths, lengths and error codes are the oracle's bit for bit; twl_stats.band_cells and twl_get_pair_cells per pair are the oracle's;
* the first kernel is the route's, nothing was re-run and the ladder was not entered (n_relaunched == 0, n_launches == 1): every pair's
  band stays inside the 512-row window, so the kernel named is the one that made every path;
* on the tile-parallel route (KNOB_MT_MIN_MARKER 64; the pools of marker 64 or more that the plan's sumLen >= 3 * marker * n admits):
  mt_tiles_predicted + mt_tiles_inline is the oracle's tile count, once with true starts and once with every second predicted start
  moved and a single round (KNOB_MT_PERTURB 1, KNOB_MT_ROUNDS 1), where the stitch launch both copies tile records and computes tiles
  in line (mt_tiles_inline > 0).

No route refuses a marker: twl_align_batch takes 2 <= marker <= 1024 on every first kernel (the tile-parallel plan alone asks for
KNOB_MT_MIN_MARKER), so the table of routes has no substitute markers.  Nothing is searched or traced here."""
import numpy as np
import pytest

import dp_cases as D
import exit_cases as E
import oracle_lib as O
from test_gpu_dp_edges import ROUTES, cus
from twilight_amd import api

pytestmark = pytest.mark.gpu

NUC_ROUTES = ("thr512", "thr768", "few16", "spec16", "spec_shared")
PROT_ROUTES = ("prot_thr512", "prot_plain16", "prot_sparse16", "prot_r1")
MT_KNOBS = ((api.KNOB_MT_MIN_MARKER, 64),)


@pytest.fixture()
def knobs(gpu):
    gpu.set_knob(api.KNOB_THR_SMALL, 0)          # (also forgets what the levels of earlier tests found of the 512-row window)
    yield gpu
    gpu.set_knob(api.KNOB_THR_SMALL, 0)
    gpu.set_knob(api.KNOB_MT_WIDE, 1)
    gpu.set_knob(api.KNOB_MT_MAX_PAIRS, 1024)
    gpu.set_knob(api.KNOB_MT_MIN_MARKER, 512)
    gpu.set_knob(api.KNOB_MT_PERTURB, 0)
    gpu.set_knob(api.KNOB_MT_ROUNDS, 2)
    gpu.set_knob(api.KNOB_NO_SPEC, 0)
    gpu.set_knob(api.KNOB_PROT_CORRIDOR, 448)
    gpu.set_knob(api.KNOB_PROT_MODE, 0)
    gpu.set_knob(api.KNOB_FORCE_GLOBAL, 0)


_ORACLE = {}


def oracle_of(case):
    """(pool, paths, lengths, cells per pair, tiles) of a case from the oracle, computed once for all routes and left unchanged."""
    if case.name not in _ORACLE:
        pool = case.batch()
        oa, on, oerr, ost = O.align_batch(O.make_params(D.matrix_of(case.P), **case.params()), pool, threads=8)
        assert not oerr.any(), (case.name, oerr.tolist())
        cells = np.zeros(pool.n_pairs, dtype=np.uint64)
        for i in range(pool.n_pairs):
            R, Q, P = int(pool.len[i, 0]), int(pool.len[i, 1]), pool.P
            _, _, st = O.align_pair(O.make_params(D.matrix_of(case.P), **case.params()), pool.freq[i, 0, :R, :P], pool.freq[i, 1, :Q, :P], pool.gap_open[i, 0, :R],
                                    pool.gap_extend[i, 0, :R], pool.gap_open[i, 1, :Q], pool.gap_extend[i, 1, :Q], int(pool.num[i, 0]), int(pool.num[i, 1]))
            cells[i] = st.cells
        assert int(cells.sum()) == ost.cells and ost.tiles == sum(len(x) for x in case.exits)
        for a in (oa, on, cells):
            a.setflags(write=False)
        _ORACLE[case.name] = (pool, oa, on, cells, int(ost.tiles))
    return _ORACLE[case.name]


def run_pool(twl, case, n_level):
    """The pool replicated to `n_level` pairs (rounded up to whole pools) through twl_align_batch; parity with the oracle; returns (stats, copies, tiles of the pool)."""
    pool, oa, on, cells, tiles = oracle_of(case)
    k = pool.n_pairs
    reps = max(1, -(-n_level // k))
    idx = np.arange(reps * k) % k
    level = pool if reps == 1 else D.replicate(pool, idx)
    aln, ln, err = twl.align_batch(twl.make_params(D.matrix_of(case.P), **case.params()), level)
    st = twl.get_stats(0)
    got_cells = twl.get_pair_cells(reps * k)
    assert not err.any(), f"{case.name}: errorType gpu {err[:2 * k].tolist()}"
    assert np.array_equal(ln, on[idx]), f"{case.name}: path length gpu {ln[:2 * k].tolist()} oracle {on.tolist()}"
    for j in range(k):      # replicated pairs against the pool's result
        same = (aln[idx == j, : on[j]] == oa[j, : on[j]]).all(axis=1)
        first = int(np.flatnonzero(idx == j)[np.argmin(same)])
        assert same.all(), (f"{case.name}: path of pool pair {j} (exits {case.exits[j]}, shape {case.shapes[j]}) differs in {int((~same).sum())} of {reps} copies; "
                            f"level pair {first} first differs at code {int(np.argmin(aln[first, : on[j]] == oa[j, : on[j]]))} of {int(on[j])}")
    assert st.band_cells == int(cells.sum()) * reps, f"{case.name}: band cells gpu {st.band_cells} oracle {int(cells.sum())} x {reps}"
    assert np.array_equal(got_cells, cells[idx]), f"{case.name}: cells per pair gpu {got_cells[:k].tolist()} oracle {cells.tolist()}"
    assert st.n_relaunched == 0 and st.n_launches == 1, (case.name, st.n_relaunched, st.n_launches, bytes(st.kernel).rstrip(b"\0"))
    return st, reps, tiles


def _cases(P, mt=False):
    return [c.name for c in E.CASES if c.P == P and (c.mt or not mt)]


@pytest.mark.parametrize("route,name", [(r, c) for r in NUC_ROUTES for c in _cases(6)] + [(r, c) for r in PROT_ROUTES for c in _cases(22)])
def test_exits_on_the_register_kernels(knobs, route, name):
    _, kn, n_of, kernel, _ladder = ROUTES[route]
    for key, value in kn:
        knobs.set_knob(key, value)
    st, _, _ = run_pool(knobs, E.BY_NAME[name], n_of(cus()))
    assert kernel in bytes(st.kernel), (route, name, bytes(st.kernel).rstrip(b"\0"))


@pytest.mark.parametrize("name", _cases(6) + _cases(22))
def test_exits_on_the_global_memory_kernel(knobs, name):
    case = E.BY_NAME[name]
    knobs.set_knob(api.KNOB_FORCE_GLOBAL, 1)
    st, _, _ = run_pool(knobs, case, len(case.pairs))
    assert b"talco_global_kernel" in bytes(st.kernel), bytes(st.kernel).rstrip(b"\0")


@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("name", _cases(6, mt=True) + _cases(22, mt=True))
def test_exits_through_tile_jobs_and_stitch(knobs, name, perturb):
    """MT == 1 tile jobs write a record per tile (true end cell, last flag, cnt, tailDir, tailLen, cells) that the stitch launch copies; with spoiled starts and one
    round it computes the tiles behind a wrong start in line as well."""
    case = E.BY_NAME[name]
    for key, value in MT_KNOBS + ((api.KNOB_MT_PERTURB, perturb),) + (((api.KNOB_MT_ROUNDS, 1),) if perturb else ()):
        knobs.set_knob(key, value)
    st, reps, tiles = run_pool(knobs, case, len(case.pairs))
    kernel = bytes(st.kernel).rstrip(b"\0")
    assert st.speculative == 3 and b"2 / 1 / 3> (tile-parallel" in kernel and (b"<%d, 16, " % case.P) in kernel, kernel
    assert st.mt_tiles_predicted + st.mt_tiles_inline == tiles * reps, (st.mt_tiles_predicted, st.mt_tiles_inline, tiles)
    if perturb:
        assert st.mt_tiles_inline > 0, (st.mt_tiles_predicted, st.mt_tiles_inline)
