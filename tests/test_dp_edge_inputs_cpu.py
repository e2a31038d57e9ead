"""The directed inputs of tests/test_gpu_dp_edges.py are in the class each of them claims.  No GPU.

Every case of dp_cases.CASES goes through the checker alone: oracle_lib.align_pair with the trace hook gives, per pair, the largest
block span `(U >> 6) - (L >> 6)` and the largest width of any diagonal, and dp_cases.check_case holds them to the committed figures and
to the class (margin: every pair within the last two blocks of the window; just over: one pair at span NV exactly, none beyond NV + 1,
the others in the margin; fLen: flen equal to the widest band passes, one less stops with errorType 2).  The GPU tests take the number
of pairs each window hands back from the same predicate, so a case that quietly left its class fails here first."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dp_cases as D  # noqa: E402
import oracle_lib as O  # noqa: E402
from twilight_amd import synth  # noqa: E402


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_case_is_in_its_class(case):
    batch = case.batch()
    D.check_case(case, case.traces(batch), batch)


def test_every_window_has_both_classes_and_every_family_its_flen_pair():
    have = {(c.P, c.nv, c.kind) for c in D.CASES}
    for P, windows in ((6, D.NUC_WINDOWS), (22, D.PROT_WINDOWS)):
        for nv in windows:
            assert (P, nv, "margin") in have and (P, nv, "over") in have, (P, nv)
    for ok, stop in D.FLEN_PAIRS:
        assert ok.kind == "flen_ok" and stop.kind == "flen_stop" and stop.flen == ok.flen - 1
        assert (ok.P, ok.length, ok.n, ok.seed, ok.xdrop, ok.gen) == (stop.P, stop.length, stop.n, stop.seed, stop.xdrop, stop.gen)
    assert {ok.P for ok, _ in D.FLEN_PAIRS} == {6, 22}
    # one pair of cases with its width below fcap = 64 * (NV - 2) of the 512-row window, one inside the margin
    assert any(ok.flen < 64 * 6 for ok, _ in D.FLEN_PAIRS) and any(64 * 6 < ok.flen <= 512 for ok, _ in D.FLEN_PAIRS)


def test_the_trace_reports_the_band_of_the_diagonal_it_names():
    """The hook's (k, L, U) is the band of diagonal k itself: diagonal 0 of every tile is the single cell [0, 0] (the band of diagonal 1
    would be [0, 1]), the widths add up to the oracle's cell count, and the records are as many as its diagonals."""
    batch = synth.make_level_batch(1, 700, members=((1, 4), (1, 4)), seed=7)
    rec = []
    R, Q = int(batch.len[0, 0]), int(batch.len[0, 1])
    _, err, st = O.align_pair(O.make_params(D.matrix_of(6)), batch.freq[0, 0, :R, :6], batch.freq[0, 1, :Q, :6], batch.gap_open[0, 0, :R], batch.gap_extend[0, 0, :R],
                              batch.gap_open[0, 1, :Q], batch.gap_extend[0, 1, :Q], int(batch.num[0, 0]), int(batch.num[0, 1]),
                              trace=lambda _u, tile, k, L, U, _s: rec.append((tile, k, L, U)))
    assert err == 0 and st.tiles >= 2
    assert all((L, U) == (0, 0) for _t, k, L, U in rec if k == 0) and sum(1 for r in rec if r[1] == 0) == st.tiles
    assert all(0 <= L <= U <= k for _t, k, L, U in rec)
    assert len(rec) == st.diags and sum(U - L + 1 for _t, _k, L, U in rec) == st.cells
    assert max(U - L + 1 for _t, _k, L, U in rec) == st.max_width


def test_span_is_not_width():
    """449 rows fit 8 blocks wherever they start, 450 only when the band's first row sits low in its block; outgrows() is the kernel's rule."""
    span = lambda L, w: ((L + w - 1) >> 6) - (L >> 6)      # noqa: E731
    assert all(span(L, 449) <= 7 for L in range(256)) and span(63, 450) == 8 and span(0, 512) == 7 and span(1, 512) == 8
    t = D.PairTrace(err=0, tile_span=[3, 8, 7], tile_width=[200, 455, 449])
    assert t.span == 8 and t.width == 455 and t.outgrows(8) and not t.outgrows(9)
    assert D.outgrown([t, D.PairTrace(err=0, tile_span=[7], tile_width=[449])], 8) == 1
