"""The levels and ownerships of tests/test_gpu_level_exchange.py contain every class they exist for.  No GPU.

Every pair of exchange_cases.main_level goes through the checker alone: oracle/level_oracle.py prepares the columns, the DP oracle gives the
path, level_cases.expected restores it.  That says which pairs lose columns (their final path travels from the path buffer, where == 2)
and which do not (from the DP output, where == 1), how long every final path is and which pair the device hands back; the ownerships say
which rank packs which kinds.  The GPU test asserts the same facts on the device's own paths, so a case that quietly degenerated fails in
both places."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exchange_cases as EC  # noqa: E402
import level_cases as LC  # noqa: E402
import level_oracle as LO  # noqa: E402
import oracle_lib as O  # noqa: E402
from test_level_edge_inputs_cpu import oracle_path  # noqa: E402


def _facts(lv):
    """Per pair: (lost columns, final length, handed back, expected results) from the checker."""
    out = []
    for p in lv.pairs:
        e0 = LC.expected(p.case, path_wo_gc=np.zeros(0, dtype=np.int8))
        path = oracle_path(p.case, e0)
        e = LC.expected(p.case, path_wo_gc=path)
        orig = tuple(len(s.rows[0]) for s in p.case.sides)
        cl = LC.classify(p.case, path, e)
        out.append(dict(lost=e["lens"] != orig, final=len(e["path_full"]), hand_back="hand_back" in cl["tiers"], exp=e, n=len(path), orig=orig))
    return out


@pytest.fixture(scope="module")
def main_n():
    lv = EC.main_level("n")
    return lv, _facts(lv)


def test_pairs_are_of_their_kind_and_length(main_n):
    lv, facts = main_n
    assert 20 <= len(lv.pairs) <= 26
    for p, f in zip(lv.pairs, facts):
        assert f["lost"] == (p.where != 1), f"{p.name}: removed columns {f['lost']}"        # (the pair that takes no part has lost columns too: the single-store run leaves it out the same way)
        assert p.final_len is None or f["final"] == p.final_len, f"{p.name}: final path of {f['final']}"
        assert f["hand_back"] == p.hand_back, f"{p.name}: handed back {f['hand_back']}"
        assert max(f["orig"]) <= 700
    for kind in (1, 2):
        have = {f["final"] for p, f in zip(lv.pairs, facts) if p.where == kind}
        assert set(EC.LENGTHS) - {1} <= have, f"kind {kind}: final lengths {sorted(have)}"
    assert 1 in {f["final"] for p, f in zip(lv.pairs, facts) if p.where == 1}
    assert sum(p.hand_back for p in lv.pairs) == 1 and sum(p.where == 0 for p in lv.pairs) == 1
    # the longest final path of the level is a restored one and no other pair reaches it: out_stride is exactly its length
    finals = sorted((f["final"], p.where, p.name) for p, f in zip(lv.pairs, facts) if p.where)
    assert finals[-1][1:] == (2, "longest_600") and finals[-1][0] > finals[-2][0]
    # a DP output row holds 2 * seq_len codes and no DP path of two non-empty sides comes near it: the longest lies below the level's seq_len
    assert max(f["n"] for f in facts) <= max(max(f["orig"]) for f in facts)


def test_ownerships_reach_their_classes(main_n):
    lv, facts = main_n
    by = {o.name: o for o in lv.ownerships}
    assert sorted(o.world for o in lv.ownerships) == [2, 2, 3, 8]
    n = len(lv.pairs)
    for o in lv.ownerships:
        assert len(o.owner) == n and all(0 <= r < o.world for r in o.owner)
    k = EC.kinds_per_rank(lv, by["w2_round_robin"])
    for r in range(2):
        assert k[r].count(1) >= 2 and k[r].count(2) >= 2, k[r]
        assert sum(a != b for a, b in zip(k[r], k[r][1:])) >= 3, f"rank {r}: kinds {k[r]} are not interleaved"
    k = EC.kinds_per_rank(lv, by["w3_rank1_owns_nothing_descending"])
    assert k[1] == [] and set(k[0]) == set(k[2]) == {1, 2}
    pl = EC.plan(by["w3_rank1_owns_nothing_descending"].owner, lv.takes_part, [0] * n, 3, (2,))
    assert pl.mine[2] == sorted(pl.mine[2], reverse=True) and len(pl.mine[2]) > 2 and pl.mine[0] == sorted(pl.mine[0])
    k = EC.kinds_per_rank(lv, by["w8_round_robin"])
    assert all(len(k[r]) >= 2 for r in range(8))
    assert any(set(k[r]) == {1} for r in range(8)) and any(set(k[r]) == {2} for r in range(8))      # a rank with one kind launches once
    k = EC.kinds_per_rank(lv, by["w2_rank1_owns_all"])
    assert k[0] == [] and len(k[1]) == n - 1
    # the handed-back pair and the pair that takes no part have neighbours on both sides in the pair order
    for i, p in enumerate(lv.pairs):
        if p.hand_back or p.where == 0:
            assert 0 < i < n - 1


def test_second_level_is_smaller_and_dealt_differently(main_n):
    lv, facts = main_n
    cases2 = EC.second_level(lv, [f["exp"] for f in facts])
    nodes = [i for ab in EC.second_level_pairs(lv) for i in ab]
    assert len(set(nodes)) == len(nodes) == 12
    bound1 = [sum(f["orig"]) for f in facts]
    bound2 = [len(c.sides[0].rows[0]) + len(c.sides[1].rows[0]) for c in cases2]
    stride1 = max(f["final"] for p, f in zip(lv.pairs, facts) if p.where)
    assert max(bound2) < stride1                       # whatever level 2's paths are, its out_stride is smaller than level 1's
    own1 = lv.ownerships[0]
    own2 = EC.second_level_owner(lv, own1)
    pl1 = EC.plan(own1.owner, lv.takes_part, bound1, own1.world)
    pl2 = EC.plan(own2, [1] * len(cases2), bound2, own1.world)
    assert pl2.block_max < pl1.block_max
    for k, (a, b) in enumerate(EC.second_level_pairs(lv)):
        assert own2[k] != own1.owner[a]
    assert set(own2) == {0, 1}
    for c in cases2:
        for s in c.sides:
            assert s.cache is not None and len(s.cache) == len(s.rows[0]) and len(s.rows) == 2


def test_protein_level_has_both_kinds_on_both_ranks():
    lv = EC.main_level("p", small=True)
    facts = _facts(lv)
    for p, f in zip(lv.pairs, facts):
        assert f["lost"] == (p.where != 1) and f["hand_back"] == p.hand_back and (p.final_len is None or f["final"] == p.final_len), p.name
    k = EC.kinds_per_rank(lv, lv.ownerships[0])
    assert all(set(k[r]) == {1, 2} for r in range(2)), k


def test_gap_only_pair_fills_its_dp_row_but_for_one_code():
    """With gaps cheaper than mismatches the DP oracle aligns A...A and C...C in one match and R + Q - 2 gaps: 2 * seq_len - 1 codes, the
    longest path a DP output row can hold (a path of R + Q codes would have no match at all; the walk starts on one)."""
    lv = EC.gap_only_level()
    go, ge = EC.GAP_ONLY["gap_open"], EC.GAP_ONLY["gap_extend"]
    seq_len = max(len(s.rows[0]) for p in lv.pairs for s in p.case.sides)
    for p in lv.pairs:
        cols = []
        for sd in range(2):
            c, _, runs = LO.prepare_side(LC.side_profile(p.case, sd), 1, lv.thr, go, ge, "n")
            assert not runs                          # nothing removed: where == 1
            cols.append(c)
        (cr, cq), P = cols, p.case.P
        path, err, _ = O.align_pair(O.make_params(LC.matrix_of("n"), gap_open=go, gap_extend=ge), cr[:, :P], cq[:, :P], cr[:, P], cr[:, P + 1], cq[:, P], cq[:, P + 1], 1, 1)
        assert err == 0 and len(path) == p.final_len, f"{p.name}: {len(path)} codes"
    assert lv.pairs[1].final_len == 2 * seq_len - 1
