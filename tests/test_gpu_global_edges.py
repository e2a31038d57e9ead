"""The global-memory DP kernel where its thread rounds, its work queue and its scratch switch (-m gpu).

talco_global_kernel (twilight_amd/csrc/talco_global.hip.h, launched by launch_global) is the last rung of the re-run ladder: no further
rung can disagree with it.  tests/test_gpu_global.py sends it bands of a few hundred and of 6 500 rows, a handful of pairs per call.
The cases of tests/global_cases.py (held to what they claim by tests/test_global_edge_inputs_cpu.py) stand where the kernel takes
another path:

A  bands of exactly 1023 / 1024 / 1025, 2047 / 2048 / 2049 and 3073 rows (protein: 1025): the cell loop, the convergence scan and the
   row re-initialisation stride by the workgroup's 1024 threads; flen above the band, equal to it, and one row short (errorType 2);
B  tiles that end by convergence while 1854, 1680 and 1206 rows survive: the scan posts to s_conv from several passes of a thread;
C  more pairs than workgroups: every workgroup takes a second pair on the scratch its first one left;
D  a call whose scratch is above the 256 MiB at which run_device releases it, a small call, the large one again.

Every comparison is that of test_gpu_global._compare -- errorType, path length and path bytes per pair, twl_stats.band_cells -- and the
band cells of every pair (twl_get_pair_cells) against oracle_lib.align_pair; the kernel named is talco_global_kernel<P>, one launch,
nothing re-run.  TWL_KNOB_POISON_TB fills the scratch with 0xFF bytes in front of the launch: the cases run with it off (the scratch
holds what the call before left there, or what a fresh allocation holds) and on, and give the same bytes.

The oracle's results are computed once per case, shared by the tests that need them and never written to."""
from dataclasses import dataclass

import numpy as np
import pytest

import global_cases as G
import oracle_lib as O
from test_gpu_dp_edges import cus
from twilight_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture
def forced(gpu):
    """Every pair of every call on the global-memory kernel.  Afterwards the poison knob is back at 1, where conftest.py's session fixture
    puts it for every GPU test (the library's own default is 0: left there, the tests behind this file would run on an unpoisoned scratch)."""
    gpu.set_knob(api.KNOB_FORCE_GLOBAL, 1)
    yield gpu
    gpu.set_knob(api.KNOB_FORCE_GLOBAL, 0)
    gpu.set_knob(api.KNOB_POISON_TB, 1)


@dataclass
class Expected:
    aln: np.ndarray
    n: np.ndarray
    err: np.ndarray
    cells: np.ndarray                    # per pair
    total: int


_ORACLE = {}


def oracle_of(key, batch_fn, **pk) -> Expected:
    """The oracle's paths, lengths, error codes (align_batch) and band cells per pair (align_pair) of a pool, once per `key`."""
    if key not in _ORACLE:
        batch = batch_fn()
        oa, on, oerr, ost = O.align_batch(O.make_params(G.matrix_of(batch.P), **pk), batch, threads=8)
        pairs = G.oracle_pairs(batch, trace=False, **pk)
        cells = np.array([r.cells for r in pairs], dtype=np.uint64)
        assert [r.err for r in pairs] == oerr.tolist() and int(cells.sum()) == ost.cells, key
        for a in (oa, on, oerr, cells):
            a.setflags(write=False)
        _ORACLE[key] = (batch, Expected(oa, on, oerr, cells, int(ost.cells)))
    return _ORACLE[key]


@dataclass
class Run:
    aln: np.ndarray
    n: np.ndarray
    err: np.ndarray
    cells: np.ndarray
    st: object


def run(twl, level, poison, **pk) -> Run:
    twl.set_knob(api.KNOB_POISON_TB, poison)
    aln, n, err = twl.align_batch(twl.make_params(G.matrix_of(level.P), **pk), level)
    return Run(aln, n, err, twl.get_pair_cells(level.n_pairs), twl.get_stats(0))


def compare(tag, got: Run, exp: Expected, P, idx=None):
    """`got` against the oracle's `exp`; pair i of the level is pair idx[i] of the oracle's pool (None: the pool itself)."""
    idx = np.arange(exp.n.size) if idx is None else np.asarray(idx)
    assert np.array_equal(got.err, exp.err[idx]), f"{tag}: errorType differs at level pairs {np.flatnonzero(got.err != exp.err[idx])[:8].tolist()}: gpu {got.err[:32].tolist()} oracle {exp.err.tolist()}"
    assert np.array_equal(got.n, exp.n[idx]), f"{tag}: path length differs at level pairs {np.flatnonzero(got.n != exp.n[idx])[:8].tolist()}: gpu {got.n[:32].tolist()} oracle {exp.n.tolist()}"
    for j in range(exp.n.size):      # every copy of a pool pair against the pool's path
        rows = np.flatnonzero(idx == j)
        same = (got.aln[rows, : exp.n[j]] == exp.aln[j, : exp.n[j]]).all(axis=1)
        assert same.all(), f"{tag}: path of pool pair {j} differs in {int((~same).sum())} of {rows.size} copies, first at level pair {int(rows[np.argmin(same)])}"
    assert got.st.band_cells == int(exp.cells[idx].astype(np.uint64).sum()), f"{tag}: band cells gpu {got.st.band_cells} oracle {int(exp.cells[idx].sum())}"
    assert np.array_equal(got.cells, exp.cells[idx]), f"{tag}: cells per pair differ at level pairs {np.flatnonzero(got.cells != exp.cells[idx])[:8].tolist()}"
    kernel = bytes(got.st.kernel).rstrip(b"\0")
    assert (b"talco_global_kernel<%d>" % P) in kernel, (tag, kernel)
    assert got.st.n_relaunched == 0 and got.st.n_launches == 1, (tag, got.st.n_relaunched, got.st.n_launches)


def same_bytes(tag, a: Run, b: Run):
    assert np.array_equal(a.err, b.err) and np.array_equal(a.n, b.n) and np.array_equal(a.cells, b.cells), tag
    for i in range(a.n.size):
        assert np.array_equal(a.aln[i, : a.n[i]], b.aln[i, : b.n[i]]), f"{tag}: pair {i}"
    assert a.st.band_cells == b.st.band_cells, tag


# ---- A. band width on the edges of a thread round ----
@pytest.mark.parametrize("name,which", [(c.name, w) for c in G.ROUND_CASES for w in (0, 1, 2)],
                         ids=[f"{c.name}-{w}" for c in G.ROUND_CASES for w in ("flen_above", "flen_equal", "flen_short")])
def test_band_of_exactly_q_rows(forced, name, which):
    """One pair whose band is Q rows at its widest (flen = Q + 7, Q) or stops with errorType 2 at Q - 1 rows (flen = Q - 1)."""
    case = G.ROUND_BY_NAME[name]
    flen = case.flens()[which]
    pk = case.params(flen)
    batch, exp = oracle_of(("round", name, flen), case.batch, **pk)
    assert (int(exp.err[0]), exp.total) == (case.expected(flen)[0], case.expected(flen)[2])
    runs = []
    for poison in (0, 1):
        got = run(forced, batch, poison, **pk)
        compare(f"{name} flen {flen} poison {poison}", got, exp, case.P)
        if flen >= case.Q:
            assert got.st.window == min(flen, batch.seq_len) == flen, (got.st.window, flen, batch.seq_len)
        assert got.st.grid == 1, got.st.grid
        runs.append(got)
    same_bytes(f"{name} flen {flen}: poison off / on", *runs)


# ---- B. convergence while the band is wider than one round ----
@pytest.mark.parametrize("poison", [0, 1])
def test_convergence_in_a_band_of_several_rounds(forced, poison):
    """conv_wide ends three tiles by convergence while 1854, 1680 and 1206 rows survive; conv_narrow converges 835 rows wide after a band
    of 2844.  Both in one call (two workgroups), then each alone (one)."""
    cases = G.CONV_CASES
    one = [oracle_of(("conv", c.name), c.batch, **c.params()) for c in cases]
    assert cases[0].params() == cases[1].params()
    pk = cases[0].params()
    exp2 = Expected(np.concatenate([e.aln for _b, e in one]), np.concatenate([e.n for _b, e in one]), np.concatenate([e.err for _b, e in one]),
                    np.concatenate([e.cells for _b, e in one]), sum(e.total for _b, e in one))
    assert exp2.cells.tolist() == [c.cells for c in cases] and not exp2.err.any()
    both = run(forced, G.join(*[b for b, _e in one]), poison, **pk)
    compare(f"both pairs, poison {poison}", both, exp2, 6)
    assert both.st.grid == 2 and both.st.window == cases[0].flen, (both.st.grid, both.st.window)
    for i, (c, (b, e)) in enumerate(zip(cases, one)):
        got = run(forced, b, poison, **pk)
        compare(f"{c.name} alone, poison {poison}", got, e, 6)
        assert np.array_equal(got.aln[0, : got.n[0]], both.aln[i, : both.n[i]]), c.name


# ---- C. more pairs than workgroups ----
@pytest.mark.parametrize("name,poisons", [("defaults", (0,)), ("open", (0, 1)), ("flen200", (0, 1)), ("xdrop800", (0,)), ("protein", (0,)), ("marker64", (0, 1))],
                         ids=["defaults", "open", "flen200", "xdrop800", "protein", "marker64"])
def test_every_workgroup_takes_a_second_pair(forced, name, poisons):
    """A level of cus() + 40 pairs (marker64: 2 cus() + 40), the pool of 26 over and over, on a persistent grid of cus() workgroups: a workgroup that has finished
    its pair takes the next from the queue, on the rotating rows, pointer rows, traceback bytes and LDS words its first pair left.

    The launch takes the live pairs longest first (order_pairs sorts by R + Q, pairs with an empty side last and not launched).  So what
    a workgroup takes second is never longer than what it took first: its rows are re-initialised up to ITS rowlen only, and everything
    behind that is still the first pair's.  In the calls with failed pairs (flen 200: errorType 2, X-drop 800: errorType 1) the first
    pair of most workgroups left its tile in the middle.  At the default marker the second pairs are the pool's two shortest and end in front of
    the marker, where no pointer row is read; with marker 64 on twice the level the second and third pairs are twelve pool pairs of 4 to 40 tiles,
    and every tile reads the pointer rows one element behind the band stored the diagonal before (global_cases.QUEUE_CALLS).  Every copy of a pool pair must come back as the oracle has the pool pair,
    whichever workgroup took it and whatever that workgroup ran before."""
    call = G.QUEUE_BY_NAME[name]
    pool, exp = oracle_of(("queue", call.P, name), lambda: G.queue_pool(call.P), **call.pk())
    assert exp.total == call.cells and tuple(int((exp.err[: G.QUEUE_LIVE] == e).sum()) for e in (0, 1, 2)) == call.errs
    idx = G.queue_level_index(G.queue_level_size(call, cus()))
    level = G.replicate(pool, idx)
    n_run = int((level.len.min(axis=1) > 0).sum())
    runs = []
    for poison in poisons:
        got = run(forced, level, poison, **call.pk())
        assert got.st.grid == cus() and n_run > got.st.grid, (got.st.grid, cus(), n_run)
        compare(f"{name} poison {poison}", got, exp, call.P, idx)
        empty = idx >= G.QUEUE_LIVE
        assert empty.sum() >= 2 and not got.n[empty].any() and not got.err[empty].any() and not got.cells[empty].any(), name
        runs.append(got)
    if len(runs) == 2:
        same_bytes(f"{name}: poison off / on", *runs)


# ---- D. scratch above and below the release threshold ----
@pytest.mark.parametrize("poison", [0, 1])
def test_scratch_released_and_allocated_again(forced, poison):
    """72 workgroups with rows of 4098 elements and 1026 rows of pointer bytes each take 319 MB: run_device releases the buffer behind
    the call.  The next call allocates a small one, the third the large one again and equals the first byte for byte.  Then the small
    level at marker 16 and the large one at marker 2: the pointer bytes at their smallest beside rows at their largest."""
    large_b, large = oracle_of(("scratch", "large"), G.scratch_large)
    small_b, small = oracle_of(("scratch", "small"), G.scratch_small)
    assert 72 * G.scratch_words(4096, large_b.seq_len, 1024) * 4 > G.RELEASE_BYTES
    first = run(forced, large_b, poison)
    compare("large, first call", first, large, 6)
    assert first.st.window == 4096 and first.st.grid == min(72, cus()), (first.st.window, first.st.grid)
    second = run(forced, small_b, poison)
    compare("small", second, small, 6)
    assert second.st.window == small_b.seq_len and second.st.grid == 8, (second.st.window, second.st.grid)
    third = run(forced, large_b, poison)
    compare("large, again", third, large, 6)
    same_bytes("large: first call / third call", first, third)
    assert third.st.window == 4096 and third.st.grid == first.st.grid
    _b, small16 = oracle_of(("scratch", "small", 16), G.scratch_small, marker=16)
    compare("small, marker 16", run(forced, small_b, poison, marker=16), small16, 6)
    _b, large2 = oracle_of(("scratch", "large", 2), G.scratch_large, marker=2)
    got = run(forced, large_b, poison, marker=2)
    compare("large, marker 2", got, large2, 6)
    assert got.st.window == 4096, got.st.window
