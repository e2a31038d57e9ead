"""The directed inputs of tests/test_gpu_level_edges.py reach the branch each of them exists for.  No GPU.

Every restore case of level_cases.restore_specs is sent through the checker alone: oracle/level_oracle.py prepares the columns, the DP
oracle (oracle_lib.align_pair) gives the path, and level_cases.classify says which scan rounds, write chunks, scratch tiers and queued
segments that path reaches.  The GPU tests repeat the same assertion on the device's own path, so an input that quietly stopped
reaching its branch fails in both places."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import level_cases as LC  # noqa: E402
import oracle_lib as O  # noqa: E402


def oracle_path(case, e):
    cr, cq = e["cols"]
    P = case.P
    oa, oerr, _ = O.align_pair(O.make_params(LC.matrix_of(case.seq_type)), cr[:, :P], cq[:, :P], cr[:, P], cr[:, P + 1], cq[:, P], cq[:, P + 1],
                               len(case.sides[0].rows), len(case.sides[1].rows))
    assert oerr == 0
    return np.asarray(oa, dtype=np.int8)


@pytest.mark.parametrize("group", ["scan", "runs", "hand_back"])
@pytest.mark.parametrize("seq_type", ["n", "p"])
def test_restore_inputs_reach_their_branch(seq_type, group):
    for spec in LC.restore_specs(seq_type, group):
        e0 = LC.expected(spec.case, path_wo_gc=np.zeros(0, dtype=np.int8))       # (columns only; the path comes next)
        path = oracle_path(spec.case, e0)
        LC.check_spec(spec, LC.classify(spec.case, path))


def test_classify_on_hand_made_paths():
    """classify() itself: boundaries, tiers and the hand-back rule on a pair small enough to read."""
    c = LC.make_edge_case("n", 1, length=50, identical=True, lead=(31, 127), trail=(0, 5), runs=([(10, 3)], [(10, 40)]))
    cl = LC.classify(c, np.zeros(50, dtype=np.int8))
    assert cl["boundaries"] == [(0, 31, 127), (10, 3, 40), (50, 0, 5)] and cl["arena"] == 201 and cl["lens"] == (50, 50)
    assert cl["tiers"] == {"nw_global", "lead_two_sided", "queued_two_sided", "trailing_run"}
    assert cl["final_len"] >= 50 + 127 + 40 + 5
    assert not LC.too_big(31, 127) and LC.too_big(32, 127) and LC.too_big(1, 128) and LC.too_big(150, 150) and not LC.too_big(2047, 1) and not LC.too_big(0, 500)
    # the same runs on a path with a gap: element 9 consumes a reference column only, so the two runs in front of kept column 10 no longer meet
    p = np.concatenate([np.zeros(9, np.int8), [2], np.zeros(40, np.int8), [1]]).astype(np.int8)
    cl = LC.classify(c, p)
    assert cl["boundaries"] == [(0, 31, 127), (10, 3, 0), (11, 0, 40), (51, 0, 5)] and "queued_one_sided" in cl["tiers"]
