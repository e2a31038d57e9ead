"""The directed inputs of tests/test_gpu_exit_edges.py take the exits they claim.  No GPU.

Every pool of exit_cases.CASES goes through the checker alone: the oracle's exit hook (twlo_align_pair_exits) gives one record per tile,
exit_cases.records turns records and final path into segments, trailing run, border fill and runs, exit_cases.tags_of is the predicate
of every class, and exit_cases.check_case holds all three to the constants committed with the case.  The GPU tests run the pools and
compare paths only, so a pool that quietly left its class fails here first."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dp_cases as D  # noqa: E402
import exit_cases as E  # noqa: E402
import oracle_lib as O  # noqa: E402

NV_SMALLEST = 8      # the 512-row windows (thr512, prot_thr512, prot_r1): every pool goes down every route of its family


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.name)
def test_case_takes_the_exits_it_claims(case):
    batch = case.batch()
    res = case.compute(batch)
    E.check_case(case, res, batch)
    spans = [tr.span for *_rest, tr in res]
    assert max(spans) < NV_SMALLEST, (case.name, spans)
    for path, _err, recs, _tags, _tr in res:      # the records tile the path: segments, then the trailing run
        assert sum(e.seg for e in recs) + recs[-1].tail_len == path.size
        assert [e.tile for e in recs] == list(range(len(recs))) and recs[-1].last and not any(e.last for e in recs[:-1])


@pytest.mark.parametrize("P", [6, 22])
def test_every_required_class_is_reached_in_both_families(P):
    have = set().union(*[set(c.tags) for c in E.CASES if c.P == P])
    missing = [t for t in E.REQUIRED if t not in have]
    assert not missing, (P, missing)
    markers = {c.marker for c in E.CASES if c.P == P}
    assert set(E.F_MARKERS) <= markers, markers
    # pools for the tile-parallel route: marker 64 or more and long enough for the plan, with converged and unconverged tiles and a trailing run among them
    mt = set().union(*[set(c.tags) for c in E.CASES if c.P == P and c.mt])
    assert {"conv.s0.later", "conv.s3.later", "conv.s1.later", "conv.s2.later", "unconv.followed", "tail1.long.unconv", "tail2.long.unconv"} <= mt, sorted(mt)
    assert not (set(E.NOT_REACHED) & have), sorted(set(E.NOT_REACHED) & have)


def test_names_are_unique_and_pools_small():
    assert len({c.name for c in E.CASES}) == len(E.CASES)
    assert all(2 <= len(c.pairs) <= 6 for c in E.CASES)


def test_the_new_entry_point_with_an_exit_hook_changes_nothing():
    """Hook or no hook, the path and the statistics are twlo_align_pair's; one record per tile."""
    case = E.BY_NAME["nuc_m128_0"]
    b = case.batch()
    M = D.matrix_of(6)
    R, Q = int(b.len[0, 0]), int(b.len[0, 1])
    args = (b.freq[0, 0, :R, :6], b.freq[0, 1, :Q, :6], b.gap_open[0, 0, :R], b.gap_extend[0, 0, :R], b.gap_open[0, 1, :Q], b.gap_extend[0, 1, :Q], int(b.num[0, 0]), int(b.num[0, 1]))
    p0, e0, s0 = O.align_pair(O.make_params(M, **case.params()), *args)
    raw = []
    p1, e1, s1 = O.align_pair_exits(O.make_params(M, **case.params()), *args, exits=lambda _u, *r: raw.append(r))
    assert e0 == e1 == 0 and np.array_equal(p0, p1) and (s0.cells, s0.diags, s0.tiles) == (s1.cells, s1.diags, s1.tiles)
    assert len(raw) == s1.tiles and [r[0] for r in raw] == list(range(s1.tiles))
    assert all(0 <= r[2] <= 2 and 0 <= r[3] <= 3 for r in raw)


def test_records_on_hand_made_paths():
    """exit_cases.records on paths written by hand: segment ends, the dropped code of later tiles, trailing run, border fill, runs."""
    # tile 0 ends at cell (2, 1): 0 2 0 consumes 3 reference and 2 query columns; tile 1 ends at (4, 4); then three trailing 1s
    path = np.array([0, 2, 0, 1, 0, 0, 1, 1, 1], dtype=np.int8)
    recs = E.records([(0, 9, 0, 3, 2, 1, 2, 1), (1, 5, 2, 0, 2, 3, 4, 4)], path, 5, 8)
    assert [(e.seg, e.tail_dir, e.tail_len, e.last) for e in recs] == [(3, 0, 0, False), (3, 1, 3, True)]
    assert recs[0].run == (1, 0, 1) and recs[1].run == (2, 1, 0) and not recs[0].border
    # a border exit: two fill codes 2, then the cell the walk left through
    path = np.array([2, 2, 0, 0, 1], dtype=np.int8)
    (e,) = E.records([(0, 4, 1, 0, 3, 2, 3, 2)], path, 4, 3)
    assert e.border and e.fill == 2 and e.run == (2, 1, 0) and (e.tail_dir, e.tail_len) == (0, 0)
    assert E.tags_of(8, 4, 3, [e], path) == {"before.mod4", "start2", "marker8.kind1", "marker8.s0"}
