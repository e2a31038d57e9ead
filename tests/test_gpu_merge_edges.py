"""The merge kernels (merge_kernels.hip.h, twl_merge.inc.hip) where their path sources, row planes, lanes, waves, rounds, tiles and column
chunks switch, against tests/merge_oracle.py: maps integer for integer, paths and rows byte for byte, no tolerance anywhere.  The inputs
come from tests/merge_cases.py; tests/test_merge_edge_inputs_cpu.py proves that each of them is what it is listed for and that the
expected paths of the level-buffer runs (tests/golden/merge_edge_paths.json) are merge_oracle.merge_pair's.  No DP oracle and no command
line run here."""
import numpy as np
import pytest

import merge_cases as MC
import merge_oracle as MO
from test_gpu_merge import _Case

pytestmark = pytest.mark.gpu


# ---- (A) paths taken from the level buffers ----

class _Levels:
    """A family on a store as host/merge.cpp's mergeProfileLevel drives it: every group's cached profile from twl_store_count_columns,
    levels of pairs of cached sides without members, the DP with gapCharScore 0, and a merge whose maps are held, after every apply, to
    merge_oracle.Maps fed the oracle's paths and to a twin merge on a second store fed the same paths from the host."""

    def __init__(self, family, thr):
        import twilight_amd as twl
        from twilight_amd import level, merge, place

        self.level = level
        fam = MC.FAMILIES[family]
        self.thr, self.seq_type = thr, fam.seq_type
        self.files = MC.family_rows(family)
        self.want = MC.golden_paths(family, thr)
        flat = [r for f in self.files for r in f]
        self.ids, at = [], 0
        for f in self.files:
            self.ids.append(list(range(at, at + len(f))))
            at += len(f)
        M = MC.matrix_of(fam.seq_type)
        self.p, self.pz = twl.make_params(M), twl.make_params(M, gap_char=0.0)
        self.st, self.st2 = level.Store(flat, fam.seq_type), level.Store(flat, fam.seq_type)
        for k, ids in enumerate(self.ids):
            place.count_columns(self.st, ids, k)
        self.mg, self.twin = merge.Merge(self.st, self.ids), merge.Merge(self.st2, self.ids)
        self.ref = MO.Maps([len(f[0]) for f in self.files])
        # a node is named by its lowest group, which is also the id of its cached profile (the commit keeps the reference side's id)
        self.node = {k: {"len": len(f[0]), "num": len(f), "weight": MO.F(len(f)), "groups": [k]} for k, f in enumerate(self.files)}

    def maps(self, mg=None):
        mg = mg or self.mg
        return [mg.map(g).tolist() for g in range(len(self.files))]

    def check_maps(self):
        want = [p.tolist() for p in self.ref.pos]
        assert self.maps() == want, "the maps after the apply from the level buffers"
        assert self.maps(self.twin) == want, "the twin's maps after the same paths from the host"

    def align(self, pairs, restore=()):
        """prepare / align / restore of one level.  Returns (stride, path lengths, the final paths read back); every path read back must
        be the oracle's."""
        nd = self.node
        sides = [[self.level.Side(members=[], member_weight=[], len=nd[k]["len"], num=nd[k]["num"], weight=float(nd[k]["weight"]), cache_id=k) for k in pr] for pr in pairs]
        seq_len, _, stride = MC.level_pitches({k: v["len"] for k, v in nd.items()}, pairs)
        lens, _ = self.st.prepare(self.p, sides, gappy_threshold=self.thr, seq_len=seq_len)
        if self.thr == 1.0:
            assert lens.tolist() == [[nd[r]["len"], nd[q]["len"]] for r, q in pairs]
        aln_len, err = self.st.align_in_hbm(self.pz)
        assert not err.any()
        plen = [int(x) for x in aln_len]
        got = [self.st.read_path(i, plen[i]) for i in range(len(pairs))]
        if len(restore):
            fin = self.st.restore(self.p, list(restore), stride)
            assert (fin > 0).all(), fin
            for t, i in enumerate(restore):
                plen[i] = int(fin[t])
                got[i] = self.st.read_final(i, plen[i])
        for i, pr in enumerate(pairs):
            if self.thr == 1.0 or i in restore:
                assert np.array_equal(got[i], self.want[pr]), f"pair {pr}: final path"
        return stride, plen, got

    def sides(self, pairs):
        return [list(self.node[r]["groups"]) for r, _ in pairs], [list(self.node[q]["groups"]) for _, q in pairs]

    def apply(self, pairs, source, stride, plen, got):
        """The apply under test (source[i]: from_dp 1 / 2, 0 = got[i] handed back from the host, None = skipped), the same on the oracle and
        on the twin, the maps compared, then the commit and the nodes' bookkeeping."""
        n = len(pairs)
        refg, qryg = self.sides(pairs)
        call_len = [0 if source[i] is None else plen[i] for i in range(n)]
        host = [got[i] if source[i] == 0 else None for i in range(n)]
        self.mg.apply_level(refg, qryg, call_len, stride, [s or 0 for s in source], paths=host if 0 in source else None)
        take = [i for i in range(n) if source[i] is not None]
        self.ref.apply([refg[i] for i in take], [qryg[i] for i in take], [self.want[pairs[i]] for i in take])
        self.twin.apply_host([refg[i] for i in take], [qryg[i] for i in take], [got[i] for i in take])
        self.check_maps()
        self.st.commit_from_dp(host, call_len, stride, restored=[i for i in range(n) if source[i] == 2])
        for i in take:
            r, q = pairs[i]
            a, b = self.node[r], self.node.pop(q)
            a["len"], a["num"], a["weight"] = plen[i], a["num"] + b["num"], MO.F(a["weight"] + b["weight"])
            a["groups"] += b["groups"]

    def step(self, step):
        stride, plen, got = self.align(step.pairs, step.restore)
        self.apply(step.pairs, step.source, stride, plen, got)

    def finish(self):
        want, W = self.ref.rows(self.files)
        assert self.mg.finish() == W and self.twin.finish() == W
        for ids, rows in zip(self.ids, want):
            assert self.st.rows_of(ids) == rows
            assert self.st2.rows_of(ids) == rows

    def __enter__(self):
        return self

    def __exit__(self, *exc):      # (also when a test fails: nothing of it is left for the interpreter's exit)
        self.mg.close()
        self.twin.close()
        self.st.close()
        self.st2.close()


@pytest.mark.parametrize("run", list(MC.RUNS))
def test_apply_from_the_level_buffers(gpu, run):
    """twl_merge_apply's three sources as mergeProfileLevel drives them: from_dp 1 = the DP output at pitch 2 * seq_len, 2 = the path buffer
    at the restore's pitch refLen + qryLen (both pitches exceed every pair's own path, and the pairs of the first level differ in length),
    0 = a downloaded row handed back from the host, and a skipped middle pair (path_len 0) whose maps stay the identity while the pair
    behind it reads its own row.  The commit leaves a skipped pair untouched and ends the level (include/twl_level.h), so the skipped pair is
    prepared again as a level of its own and applied there.  Every run goes on through the levels that merge the merged pairs with each
    other, from the level buffers again: the first groups' maps are composed two or three times and a side holds two or four groups."""
    spec = MC.RUNS[run]
    with _Levels(spec.family, spec.thr) as lv:
        for k, step in enumerate(spec.steps):
            lv.step(step)
            if k == 0 and None in step.source:
                for g in step.pairs[step.source.index(None)]:
                    assert lv.mg.map(g).tolist() == list(range(len(lv.files[g][0]))), "a skipped pair's maps stay the identity"
        assert sorted(lv.node[0]["groups"]) == list(range(len(lv.files)))
        lv.finish()


def test_level_sources_that_are_refused(gpu):
    """Every refusal next to a good call: the maps are what they were, and the good call that follows passes.  from_dp 1 with a path longer
    than the DP output's rows can only be asked for groups wider than the level's pairs (path_len <= ref width + qry width is checked first,
    and a level's seq_len covers its own sides), so that call names the two widest groups while the level holds the narrowest pair."""
    import twilight_amd as twl

    with _Levels("nuc6", 1.0) as lv:
        _refusals(twl, lv)


def _refusals(twl, lv):
    mg = lv.mg

    def refused(message, *args, **kw):
        before = lv.maps()
        with pytest.raises(twl.TwlError, match=message):
            mg.apply_level(*args, **kw)
        assert lv.maps() == before

    # a level of the narrowest pair alone: its DP rows are 2 * 170 codes long
    small = [(2, 3)]
    stride, plen, got = lv.align(small)
    too_long = 2 * lv.node[3]["len"] + 1
    assert too_long <= lv.node[0]["len"] + lv.node[1]["len"]
    refused("from_dp 1 without a DP output of that length", [[0]], [[1]], [too_long], too_long, [1])
    refused("path_len outside", [[2]], [[3]], [too_long], too_long, [1])
    lv.apply(small, [1], stride, plen, got)
    # a level of two pairs
    two = [(0, 1), (4, 5)]
    stride, plen, got = lv.align(two)
    refg, qryg = lv.sides(two)
    refused("from_dp 2: twl_level_restore first", refg, qryg, plen, stride, [2, 2])                    # no restore yet
    refused("from_dp 2: twl_level_restore first", refg, qryg, plen, stride, [1, 2])
    refused("from_dp needs the prepared and aligned level of these pairs", refg[:1], qryg[:1], plen[:1], stride, [1])
    refused("from_dp needs the prepared and aligned level of these pairs", refg + [[2, 3]], qryg + [[2, 3]], plen + [0], stride, [1, 1, 1])
    fin = lv.st.restore(lv.p, [0, 1], stride)
    assert fin.tolist() == plen
    assert max(plen) < stride - 1
    refused("from_dp 2: twl_level_restore first", refg, qryg, plen, stride - 1, [2, 2])                # not the restore's pitch
    refused("from_dp 2: twl_level_restore first", refg, qryg, plen, stride + 1, [1, 2])
    lv.apply(two, [2, 1], stride, plen, got)
    for step in MC.RUNS["thr1_dp_output_and_path_buffer"].steps[1:]:
        lv.step(step)
    lv.finish()


# ---- (B) rows on both planes, and a finish that re-pitches them ----

def _move_to_the_other_plane(st, ids, rows):
    """A fresh merge of one group rewrites its rows into their other plane when it finishes, at their own width (one call per length)."""
    from twilight_amd import merge

    for L in sorted({len(rows[i]) for i in ids}):
        mg = merge.Merge(st, [[i for i in ids if len(rows[i]) == L]])
        assert mg.finish() == L
        mg.close()


@pytest.mark.parametrize("name", list(MC.PLANE_WIDTHS))
def test_rows_on_both_planes(gpu, name):
    """merge_rewrite_kernel reads every row from its own plane and writes the other one: a group on plane 1, a group on plane 0 and a group
    of 2 * 16 + 5 rows that alternate, so every slice of 16 rows mixes the planes.  The other plane of every row holds a copy that differs at
    every column (the store is created with those, every row is moved to plane 1, the rows meant for plane 0 are moved back, and the live
    rows are written over the current plane).  The store starts at the least pitch, 256 (twl_store_create: max_len + 1 rounded up to 256
    when the generous allocation fails): W = 255 still fits (twl_merge_finish needs W + 1), W = 256 is the smallest width for which
    grow_rows reallocates and copies both planes first.  The two rows outside the merge, one per plane, stay as they are."""
    import twilight_amd as twl
    from twilight_amd import api, level

    c = MC.plane_case(name)
    twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 1)          # the generous pitch fails: the store starts at the pitch its rows need
    try:
        st = level.Store(c.stale, "n")
    finally:
        twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 0)
    try:
        _finish_on_both_planes(st, c)
    finally:
        st.close()


def _finish_on_both_planes(st, c):
    from twilight_amd import merge

    n = len(c.live)
    everyone = list(range(n))
    _move_to_the_other_plane(st, everyone, c.stale)
    _move_to_the_other_plane(st, [i for i in everyone if c.plane[i] == 0], c.stale)
    assert st.rows_of(everyone) == c.stale
    st.write_rows(everyone, c.live)
    assert st.rows_of(everyone) == c.live
    mg = merge.Merge(st, c.groups)
    ref = MO.Maps([len(c.live[g[0]]) for g in c.groups])
    for call in c.calls:
        mg.apply_host(*call)
        ref.apply(*call)
        assert [mg.map(g).tolist() for g in range(3)] == [p.tolist() for p in ref.pos]
    want, W = ref.rows([[c.live[i] for i in g] for g in c.groups])
    assert mg.finish() == W == c.W
    for k, (ids, rows) in enumerate(zip(c.groups, want)):
        got = st.rows_of(ids)
        for i, g, w in zip(ids, got, rows):
            assert g == w, f"group {k}, row {i} (plane {c.plane[i]} before the finish)"
    assert st.rows_of(c.extra) == [c.live[i] for i in c.extra], "rows outside the merge"


# ---- (C) where the kernels switch, with host paths ----

def _run_case(case):
    c = _Case(case.files)
    try:
        for call in case.calls:
            c.apply(*call)                # (the maps are compared after every call)
        assert c.finish() == case.W
    finally:
        c.close()


@pytest.mark.parametrize("code", [1, 2])
@pytest.mark.parametrize("at", MC.RANK_INDICES)
def test_rank_kernel_one_code_on_an_edge(gpu, code, at):
    """merge_ranks_kernel: the only query-only (1) or reference-only (2) code of a path of a tile and 304 codes sits on lane 0, on the last
    lane of a wave, on the first lane of the next, on the last thread of a round, on the first code of the next round, on the last code
    of a tile, on the first of the next, on the path's last code: every rank behind it is off by one in one table and not in the other."""
    _run_case(MC.rank_case(code, at))


@pytest.mark.parametrize("n", [256, 257])
def test_rank_kernel_one_round_and_one_code_more(gpu, n):
    _run_case(MC.round_case(n))


def test_three_pairs_of_very_different_sizes_in_one_call(gpu):
    """Paths of 300, 5000 and 40 codes in one launch, sides of one and two groups that have been composed once: the rank arena's offsets
    (0, 180, 380, 3280, 5880, 5904) and the ten rows of the compose table."""
    _run_case(MC.three_pairs_case())


def test_column_blocks_of_the_map_kernels(gpu):
    """merge_iota / merge_compose / merge_inverse with grid.y = 3: groups of 1, 255, 256, 257 and 513 columns, four levels."""
    _run_case(MC.column_tile_case())


@pytest.mark.parametrize("W", MC.REWRITE_WIDTHS)
def test_rewrite_last_chunk_of_columns(gpu, W):
    """merge_rewrite_kernel: W % 16 = 0, 1 and 15 below 64 and near 300, and W = 16: one whole chunk; 17 rows: a slice of one row."""
    _run_case(MC.rewrite_width_case(W))


def test_rewrite_group_of_one_column(gpu):
    _run_case(MC.lone_column_case())
