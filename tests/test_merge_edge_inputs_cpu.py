"""The directed merge inputs (tests/merge_cases.py) are what tests/test_gpu_merge_edges.py takes them for: the committed final paths are
the oracle's (merge_oracle.merge_pair over level_oracle.update_frequency, recomputed here), the families lose the columns and have the
pitches the level-buffer runs need, the rows of the plane cases differ between the planes, and every constructed host path is well formed
and has its exceptional code where the case says.  No GPU needed."""
import functools

import numpy as np
import pytest

import level_cases as LC
import merge_cases as MC
import merge_oracle as MO


@functools.lru_cache(maxsize=None)
def _oracle(name, thr):
    return MC.oracle_paths(name, thr)


# ---- (A) the families and their runs ----

@pytest.mark.parametrize("name,thr", MC.GOLDEN_KEYS, ids=[MC.golden_key(*k) for k in MC.GOLDEN_KEYS])
def test_committed_paths_are_the_oracles(name, thr):
    want, got = _oracle(name, thr), MC.golden_paths(name, thr)
    assert sorted(got) == sorted(want) == sorted(p for level in MC.FAMILIES[name].levels for p in level)
    for k, o in want.items():
        assert o.retries == 0, f"pair {k}: the oracle's first DP run ended with an error"
        assert MO.path_ok(o.path, *o.lens)
        assert np.array_equal(got[k], o.path), f"pair {k}"
        assert np.array_equal(MC.unrle(MC.rle(o.path)), o.path)


def test_families_are_what_the_issue_asks_for():
    assert len(MC.FAMILIES["nuc6"].groups) == 6 and MC.FAMILIES["prot4"].seq_type == "p"
    for name, fam in MC.FAMILIES.items():
        rows = MC.family_rows(name)
        for g, rr in zip(fam.groups, rows):
            assert 3 <= len(rr) <= 9 and 150 <= len(rr[0]) <= 320 and len(rr[0]) == g.len and all(len(r) == len(rr[0]) for r in rr)
            cols = np.frombuffer(b"".join(rr), dtype=np.uint8).reshape(len(rr), -1)
            assert set(np.flatnonzero((cols == ord("-")).all(axis=0)).tolist()) == set(g.empty)
        assert any(g.empty for g in fam.groups) and not all(g.empty for g in fam.groups)
        lens = [(len(rows[r][0]), len(rows[q][0])) for r, q in fam.levels[0]]
        assert len({l for pr in lens for l in pr}) == 2 * len(lens), "lengths differ between and within the pairs"
    prot = b"".join(r for rr in MC.family_rows("prot4") for r in rr).upper()
    assert set(prot) - set(b"ACGTN-"), "protein letters"


def test_columns_lost_at_095():
    """At -r 0.95 every pair of every level loses columns on a side, one pair at least on both, and no two runs are too big for the
    restore kernel whichever boundary they met at; at -r 1 nothing is removed and the paths differ."""
    o95, o1 = _oracle("nuc6", 0.95), _oracle("nuc6", 1.0)
    both = 0
    for k, o in o95.items():
        assert o.runs[0] or o.runs[1], f"pair {k} loses no column"
        both += bool(o.runs[0] and o.runs[1])
        assert not any(LC.too_big(lr, lq) for _, lr in o.runs[0] for _, lq in o.runs[1]), f"pair {k}"
    assert both >= 1
    assert all(o.runs == ([], []) for o in o1.values())
    first = MC.FAMILIES["nuc6"].levels[0]
    assert any(not np.array_equal(o95[k].path, o1[k].path) for k in first)


@pytest.mark.parametrize("run", list(MC.RUNS))
def test_run_is_what_it_is_listed_for(run):
    spec = MC.RUNS[run]
    fam = MC.FAMILIES[spec.family]
    paths = MC.golden_paths(spec.family, spec.thr)
    lens = {k: g.len for k, g in enumerate(fam.groups)}
    applied = []
    for step in spec.steps:
        assert len(step.source) == len(step.pairs) and set(step.restore) <= set(range(len(step.pairs)))
        seq_len, dp_pitch, path_pitch = MC.level_pitches(lens, step.pairs)
        for i, (pr, src) in enumerate(zip(step.pairs, step.source)):
            n = len(paths[pr])
            assert n not in (dp_pitch, path_pitch), f"pair {pr}: as long as a pitch"
            assert src in (None, 0, 1, 2)
            assert (src == 2) == (i in step.restore) or src in (None, 0), "from_dp 2 is a restored pair, from_dp 1 is not"
            if spec.thr != 1.0:
                assert src == 2, "a pair that lost columns is final in the path buffer only"
        if len(step.pairs) > 1:      # a wrong pitch lands inside another pair's row
            assert any(max(lens[r], lens[q]) < seq_len for r, q in step.pairs) and any(lens[r] + lens[q] < path_pitch for r, q in step.pairs)
            assert dp_pitch != path_pitch
        for pr, src in zip(step.pairs, step.source):
            if src is not None:
                applied.append(pr)
                lens[pr[0]] = len(paths[pr])
                del lens[pr[1]]
    assert sorted(applied) == sorted(p for level in fam.levels for p in level)
    assert len(lens) == 1 and len(spec.steps) >= 2
    first = spec.steps[0]
    want = {"thr1_dp_output": {1}, "thr1_dp_output_and_path_buffer": {1, 2}, "thr095_path_buffer": {2}, "skipped_middle_pair": {1, 2, None},
            "host_row_among_level_rows": {0, 1, 2}}[run]
    assert set(first.source) == want
    if run == "thr1_dp_output":
        assert not any(s.restore for s in spec.steps)
    if run == "thr095_path_buffer":
        assert all(s.restore == list(range(len(s.pairs))) for s in spec.steps)
    if run == "skipped_middle_pair":
        assert len(first.pairs) == 3 and first.source[1] is None and first.source[2] is not None
        assert spec.steps[1].pairs == [first.pairs[1]] and spec.steps[1].source == [1]


# ---- (B) the planes ----

@pytest.mark.parametrize("name", list(MC.PLANE_WIDTHS))
def test_plane_case(name):
    c = MC.plane_case(name)
    n = len(c.live)
    assert sorted(i for g in c.groups for i in g) + c.extra == list(range(n))
    for i in range(n):
        a, b = np.frombuffer(c.live[i], np.uint8), np.frombuffer(c.stale[i], np.uint8)
        assert len(a) == len(b) and (a != b).all(), f"row {i}: the stale copy must differ at every column"
    assert {c.plane[i] for i in c.groups[0]} == {1} and {c.plane[i] for i in c.groups[1]} == {0}
    g2 = c.groups[2]
    assert len(g2) == 2 * MC.ROWS_PER_WG + 5
    for at in range(0, len(g2), MC.ROWS_PER_WG):
        assert {c.plane[i] for i in g2[at: at + MC.ROWS_PER_WG]} == {0, 1}, "a slice of the rewrite on one plane only"
    assert [c.plane[i] for i in c.extra] == [0, 1]
    maps = MO.Maps([len(c.live[g[0]]) for g in c.groups])
    for call in c.calls:
        maps.apply(*call)
    _, W = maps.rows([[c.live[i] for i in g] for g in c.groups])
    assert W == c.W == MC.PLANE_WIDTHS[name]
    pitch = MC.least_pitch(max(len(r) for r in c.live))
    assert pitch == 256
    if name == "beyond_the_pitch":
        assert W + 1 > pitch and W == pitch, "the smallest W that re-pitches the planes"
    else:
        assert W + 1 == pitch, "the largest W that does not"


# ---- (C) host paths on the kernels' edges ----

def _replay(case):
    maps = MO.Maps([len(f[0]) for f in case.files])
    for f in case.files:
        assert f and all(len(r) == len(f[0]) for r in f)
    for call in case.calls:
        assert len(call[0]) == len(call[1]) == len(call[2])
        maps.apply(*call)                      # (asserts path_ok against the sides' current widths)
    _, W = maps.rows(case.files)
    assert W == case.W
    return maps


def test_rank_indices_are_the_edges():
    assert MC.RANK_INDICES == (0, 63, 64, 255, 256, 4095, 4096, MC.RANK_LEN - 1)
    assert MC.RANK_LEN > MC.TILE + MC.THREADS and (MC.RANK_LEN - MC.TILE) % MC.THREADS not in (0, 1) and (MC.RANK_LEN - 1) % MC.WAVE not in (0, MC.WAVE - 1)


@pytest.mark.parametrize("code", [1, 2])
@pytest.mark.parametrize("at", MC.RANK_INDICES)
def test_rank_case(code, at):
    c = MC.rank_case(code, at)
    (path,) = c.calls[0][2]
    assert len(path) == MC.RANK_LEN and np.flatnonzero(path).tolist() == [at] and path[at] == code
    wr, wq = len(c.files[0][0]), len(c.files[1][0])
    assert MO.path_ok(path, wr, wq) and wr + wq - int(np.count_nonzero(path == 0)) == MC.RANK_LEN
    maps = _replay(c)
    short = maps.pos[0] if code == 1 else maps.pos[1]      # the side without the exceptional column steps over it
    assert short.tolist() == [x for x in range(MC.RANK_LEN) if x != at]


@pytest.mark.parametrize("n", [256, 257])
def test_round_case(n):
    c = MC.round_case(n)
    assert len(c.calls[0][2][0]) == n and {0, 1, 2} == set(c.calls[0][2][0].tolist())
    _replay(c)


def test_three_pairs_case():
    c = MC.three_pairs_case()
    maps = MO.Maps([len(f[0]) for f in c.files])
    maps.apply(*c.calls[0])
    ref, qry, paths = c.calls[1]
    sizes = [len(p) for p in paths]
    assert sizes == c.note["sizes"] == [300, 5000, 40] and sizes != sorted(sizes) and sizes != sorted(sizes, reverse=True)
    off, at = [], 0
    for rg, qg in zip(ref, qry):
        for side in (rg, qg):
            assert len(side) in (1, 2)
            if len(side) == 2:
                assert all(not np.array_equal(maps.pos[g], np.arange(len(maps.pos[g]))) for g in side), "composed once before the call"
            off.append(at)
            at += maps.width[side[0]]
    assert off == c.note["rank_off"]
    assert {len(s) for s in ref + qry} == {1, 2} and sum(len(s) for s in ref + qry) == 10
    _replay(c)


def test_column_tile_case():
    c = MC.column_tile_case()
    assert sorted(len(f[0]) for f in c.files) == [1, 255, 256, 257, 513] and len(c.calls) == 4
    assert all(len(call[2]) == 1 for call in c.calls)
    assert (max(len(f[0]) for f in c.files) + MC.THREADS - 1) // MC.THREADS == 3
    maps = _replay(c)
    assert len(maps.pos[0]) == 257 and not np.array_equal(maps.pos[0], np.arange(257))


def test_rewrite_width_cases():
    W = MC.REWRITE_WIDTHS
    assert {w % MC.COLS for w in W if w < 64 and w != 16} == {0, 1, 15} == {w % MC.COLS for w in W if 290 <= w <= 310}
    assert 16 in W
    for w in W:
        c = MC.rewrite_width_case(w)
        assert len(c.files[0]) > MC.ROWS_PER_WG
        _replay(c)


def test_lone_column_case():
    c = MC.lone_column_case()
    maps = _replay(c)
    assert len(c.files[1][0]) == 1 and maps.pos[1].tolist() == [c.note["at"]] and c.W == 400
    assert maps.pos[0].tolist() == [x for x in range(400) if x != c.note["at"]]
