"""Every case of tests/mt_cases.py reaches the branch of the tile-parallel kernels it is listed for -- proven with the oracle (whole pairs, single tiles from a
given start) and the restatements of tests/mt_oracle.py alone, no GPU.  tests/test_gpu_mt_edges.py runs the same cases on the device; if a case stops reaching
its class (another generator, another seed), this file fails.

Out of scope, here as there: wide re-runs (the MT 4 pair scout, the 3072-row geometry) and the 512-row tile geometry -- they depend on what a pass remembers and have
behavioural tests in tests/test_gpu_mt.py."""
import collections

import numpy as np
import pytest

import mt_cases as MC
import mt_oracle as MO
import oracle_lib as O
from twilight_amd import api

_FACTS = {}


def facts(name):
    """Per case, computed once: the launch order, the plan with the case's knobs, the oracle's view of every pair that runs, the restated anchor table."""
    if name not in _FACTS:
        c = MC.case(name)
        b = c.batch
        order = MO.launch_order(b.len)
        pl = MO.plan(b.len, order, b.seq_len, c.marker, anchor=c.knob(api.KNOB_MT_ANCHOR, 1), lead2=c.knob(api.KNOB_MT_LEAD2), marg=c.knob(api.KNOB_MT_MARGIN))
        op = O.make_params(c.matrix, **c.pk)
        tiles = MO.Tiles(op, b)
        pairs = {}
        for p in order:
            aln, err, st, rows = O.pair_exits(op, tiles.view(p))
            starts = ([(0, 0)] + [(r, q) for (_t, _k, _s, r, q) in rows])[: st.tiles]
            pairs[p] = dict(starts=starts, tiles=int(st.tiles), err=int(err), cells=int(st.cells), width=int(st.max_width), kinds=[k for (_t, k, _s, _r, _q) in rows], aln=aln)
        anchors = MO.anchor_table(b, pl, c.marker, pl["dims"]["lead2"], detail=True) if pl["dims"]["anchors"] else (None, {})
        _FACTS[name] = dict(case=c, order=order, plan=pl, params=op, tiles=tiles, pairs=pairs, anchor=anchors[0], info=anchors[1])
    return _FACTS[name]


@pytest.mark.parametrize("name", MC.NAMES)
def test_every_level_meets_the_policys_condition_and_fits_every_window(name):
    f = facts(name)
    c, b = f["case"], f["case"].batch
    assert c.knob(api.KNOB_MT_MIN_MARKER) == 64 and c.marker in (128, 250) and 1 <= b.n_pairs <= 6
    assert MO.takes_the_path(b.len, f["order"], c.marker), "sumLen >= 3 * marker * n_run and 2 * n_run <= CUs"
    # bands within the narrowest window a tile job or the stitch launch of either geometry has (two blocks of margin: 768 - 128 rows nucleotide, 512 - 128
    # protein), so that no pair is re-run and every record carries a result or an errorType
    assert max(v["width"] for v in f["pairs"].values()) <= (640 if b.P == 6 else 384)
    for row, p in enumerate(f["order"]):
        # tile t of the pair starts on anti-diagonal >= (marker - 1) * t, which must lie in the pair: the plan has a slot for every tile the oracle runs
        assert f["pairs"][p]["tiles"] <= f["plan"]["T"][row] <= f["plan"]["dims"]["slots"]


def test_boundary_arithmetic():
    f = facts("boundary")
    b, m = f["case"].batch, f["case"].marker
    edge = (m - 1) * 10 - 1
    assert [int(b.len[p].sum()) - 2 - edge for p in range(3)] == [-1, 0, 1]
    assert f["order"] == [2, 1, 0] and f["plan"]["T"] == [11, 11, 10]                 # T switches between s = 10 and s + 1
    assert f["plan"]["dims"]["n_scout"] == 10 + 10 + 9 and f["plan"]["dims"]["n_tile"] == 32
    assert [s for (p, s, row) in f["plan"]["scouts"] if s == 10] == [10, 10]          # boundary 10 has a scout for the two longer pairs only
    assert [f["pairs"][p]["tiles"] for p in f["order"]] == [10, 10, 10]


def test_stepped_over_and_landed_boundaries():
    f = facts("stepped")
    m = f["case"].marker
    kinds = set()
    for p, v in f["pairs"].items():
        d = [r + q for r, q in v["starts"]]
        adv = collections.Counter(d[t + 1] - d[t] for t in range(1, len(d) - 1))      # (tile 0 advances like any other; counted from tile 1 to be on the safe side)
        assert set(adv) <= {m - 1, m} and adv[m - 1] >= 3 and adv[m] >= 3, (p, adv)
        kinds |= set(v["kinds"])
    assert {0, 1} <= kinds                                                            # converged exits and the pair's end in front of the marker


def _tail(f, p):
    v = f["pairs"][p]
    pv = f["tiles"].view(p)
    nxt, last, err, _cells, seg = f["tiles"](p, v["starts"][-1], len(v["starts"]) == 1)
    assert last and err == 0
    if nxt[0] == pv.R - 1 and nxt[1] < pv.Q - 1:
        n = pv.Q - nxt[1] - 1
        assert np.all(seg[-n:] == 1)
        return 1, n
    if nxt[1] == pv.Q - 1 and nxt[0] < pv.R - 1:
        n = pv.R - nxt[0] - 1
        assert np.all(seg[-n:] == 2)
        return 2, n
    assert nxt == (pv.R - 1, pv.Q - 1)
    return 0, 0


def test_tails_and_ends():
    f = facts("tails")
    got = {p: _tail(f, p) for p in f["order"]}
    assert got[0][0] == 1 and got[0][1] > 0 and got[1][0] == 2 and got[1][1] > 0 and got[2] == (0, 0), got


def test_degenerate_pairs_beside_long_ones():
    f = facts("degenerate")
    b, pl = f["case"].batch, f["plan"]
    assert b.len[1, 0] == 1 and b.len[2, 1] == 1 and b.len[3, 0] == 0 and b.len[4].sum() < f["case"].marker
    assert 3 not in f["order"] and len(f["order"]) == 5
    row = {p: f["order"].index(p) for p in f["order"]}
    assert pl["T"][row[4]] == 1 and not any(r == row[4] for (_p, _s, r) in pl["scouts"])      # one tile, no scout
    for p in (1, 2):      # scouts exist (the plan counts R + Q) and every one of them leaves early: the anchor row stays -1, and so does the chain behind tile 0
        assert pl["T"][row[p]] > 1 and np.all(f["anchor"][row[p]] == -1)
        assert all(f["info"][(row[p], s)]["why"] == "early" for s in range(1, pl["T"][row[p]]))
        R, Q = int(b.len[p, 0]), int(b.len[p, 1])
        ch = MO.chain(np.full(pl["dims"]["sp_pitch"], -16843010, dtype=np.int32), R, Q, pl["dims"]["slots"], f["case"].marker)      # (0xFEFEFEFE: nobody wrote)
        assert ch[0].tolist() == [0, 0] and np.all(ch[1:] == -1)
    assert np.all(f["anchor"][row[4]] == -1)
    assert sorted(v["why"] for v in f["info"].values()).count("trusted") > 30          # ... beside long pairs whose boundaries anchor


def test_scout_start_clamps():
    f = facts("boundary")      # default leads: the first boundaries start before anti-diagonal 0
    m = f["case"].marker
    assert all(f["info"][(row, 1)]["clamped_d0"] and f["info"][(row, 1)]["d0"] == 0 for row in range(3)) and (m - 1) * 1 - 1 < 128
    assert not f["info"][(0, 3)]["clamped_d0"]
    f = facts("clamps")
    b = f["case"].batch
    assert b.len[0, 0] >= 8 * b.len[0, 1] and b.len[1, 1] >= 8 * b.len[1, 0]
    fired = {k: v["clamps"] for k, v in f["info"].items() if any(v["clamps"])}
    row = f["order"].index(1)
    # the reference-row clamp fires at the last boundary of the pair with Q >> R, nowhere else; the query-row clamp cannot fire inside a pair (mt_oracle.line_cell)
    assert fired == {(row, 20): (False, True)}, fired
    assert (f["case"].marker - 1) * 20 - 1 == int(b.len[1].sum()) - 2                 # ... which reports from the pair's last anti-diagonal


def test_scout_marker_clamp_and_overlapping_ranges():
    f = facts("long")
    c, pl = f["case"], f["plan"]
    m, lead, marg = c.marker, c.knob(api.KNOB_MT_LEAD), pl["dims"]["marg"]
    assert pl["dims"]["anchors"] == 0 and lead == 900 and marg == 64
    slots = [s for (_p, s, _row) in pl["scouts"]]
    clamped = [s for s in slots if (m - 1) * s - 1 >= lead and s + 2 + marg + lead > MO.K_MAX_MARKER]
    assert clamped and min(clamped) == 59, clamped[:3]
    both = [s for s in slots if s >= m - 3 and s + 1 in slots]
    assert both and int(c.batch.len[0].sum()) >= 16003
    for s in both:      # the report ranges [(marker - 1) * s - 1, marker * s + 1] of s and s + 1 share anti-diagonals
        assert m * s + 1 >= (m - 1) * (s + 1) - 1
    assert f["pairs"][0]["tiles"] == 131 and f["pairs"][0]["err"] == 0


@pytest.mark.parametrize("name", ["anchors_leaf", "anchors_profile"])
def test_anchor_classes(name):
    f = facts(name)
    info = f["info"]
    assert {v["window"] for v in info.values() if v["why"] == "trusted"} == set(range(9)), "boundaries decided in each of the nine windows"
    whys = collections.Counter(v["why"] for v in info.values())
    assert whys["few"] >= 1 and whys["close"] >= 1, whys                               # rejected for fewer than 36 matches / for a runner-up within 8
    ties = [(k, v) for k, v in info.items() if v["tie"]]
    # offsets 0 and +1 tie and 0 wins; offsets -1 and +1 tie and the negative one wins (the order 0, -1, 1, -2, 2, ...)
    assert sorted((v["value"] - 128, tuple(v["tied"])) for _k, v in ties) == [(-1, (1,)), (0, (1,))], ties
    assert set().union(*(v["left"] for v in info.values())) == {"r-", "r+", "q-", "q+"}, "windows past either end of either side"
    assert (name == "anchors_leaf") == bool(np.all(f["case"].batch.num == 1))
    for (row, slot), v in info.items():
        assert f["anchor"][row, slot] == v["value"] and (v["value"] == -1 or 0 <= v["value"] < 256)


def test_anchor_early_outs_and_protein_letters():
    f = facts("degenerate")
    assert sum(1 for v in f["info"].values() if v["why"] == "early") == 11 + 11         # every boundary of the R = 1 and of the Q = 1 pair
    # (the third early out, a boundary beyond R + Q - 2, cannot be reached from the plan: a scout exists only for boundaries inside the pair -- mt_oracle.tiles_of)
    for nm in MC.NAMES:
        g = facts(nm)
        for (p, s, row) in g["plan"]["scouts"]:
            assert (g["case"].marker - 1) * s - 1 <= int(g["case"].batch.len[p].sum()) - 2
    f = facts("protein")
    b = f["case"].batch
    assert b.P == 22 and b.n_pairs == 4 and f["case"].marker == 250
    letters = np.concatenate([MO.consensus(b.freq[p, s], int(b.len[p, s]), s, 22) for p in range(4) for s in range(2)])
    assert set(letters[letters < 100].tolist()) == set(range(20))                       # the twenty letters, not the wildcard, not the gap
    assert sum(1 for v in f["info"].values() if v["why"] == "trusted") >= 40


def test_error_cases_name_the_failing_tile():
    f = facts("err1")
    assert {p: (v["err"], v["tiles"]) for p, v in f["pairs"].items()} == {0: (0, 24), 1: (1, 11), 2: (0, 24)}
    f2 = facts("err2")
    assert f2["case"].pk["flen"] == 128
    assert {p: (v["err"], v["tiles"]) for p, v in f2["pairs"].items()} == {0: (2, 8), 1: (2, 1), 2: (2, 6)}
    for g in (f, f2):
        for p, v in g["pairs"].items():
            if v["err"]:
                t = v["tiles"] - 1           # the tile that fails, from its true start
                _nxt, last, err, cells, seg = g["tiles"](p, v["starts"][t], t == 0)
                assert err == v["err"] and last and seg.shape[0] == 0 and cells > 0
                if t > 0:                    # ... and the one before it does not
                    assert g["tiles"](p, v["starts"][t - 1], t - 1 == 0)[2] == 0
