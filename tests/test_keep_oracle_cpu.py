"""tests/keep_oracle.py against itself and against tests/place_oracle.py, on every directed input the GPU tests of the keep-length finish use
(tests/test_gpu_keep_edges.py): the direct row is the merged row with the insertion columns deleted, the records give the sequence back,
the counts are those of the path, and every spec still reaches the branch of the kernels it is listed for.  No GPU needed."""
import numpy as np
import pytest

import keep_cases as KC
import keep_oracle as KO
import place_cases as PC
import place_oracle as PO

PLACE_GROUPS = ("tiles", "tiles2", "chunks", "len4095", "len4096", "len4097")


def _families():
    for g in PLACE_GROUPS:
        yield "place-" + g, PC.group_inputs(g)
    for g in KC.GROUPS:
        yield "keep-" + g, KC.group_inputs(g)
    for L in sorted(PC.ROUND_CASES):
        yield "round-%d" % L, PC.round_inputs(L)[:3]


FAMILIES = dict(_families())


@pytest.mark.parametrize("name", list(FAMILIES))
def test_direct_row_is_the_stripped_merged_row(name):
    backbone, seqs, paths = FAMILIES[name]
    L = len(backbone[0])
    longest = PO.merge_insertions(L, paths)
    assert KO.insertion_mask(longest).sum() == longest.sum() and len(KO.insertion_mask(longest)) == L + longest.sum()
    for r in backbone:
        assert KO.strip_row(PO.expand_backbone(r, longest), longest) == r
    for s, p in zip(seqs, paths):
        merged = PO.expand_placed(s, p, longest)
        row = KO.keep_row(s, p, L)
        assert len(row) == L and b"." not in row
        assert KO.strip_row(merged, longest) == row
        recs = KO.runs(p)
        assert [(c, s[q: q + n]) for c, q, n in recs] == KO.records_of_merged(merged, longest)
        assert KO.rebuild(row, [(c, s[q: q + n]) for c, q, n in recs]) == s
        assert KO.counts(p) == (len(PC.runs_of(p)), int(np.count_nonzero(np.asarray(p) == 1)))
        assert [c for c, _, _ in recs] == sorted(c for c, _, _ in recs) and len({c for c, _, _ in recs}) == len(recs)
        assert KO.insertion_lines(b"x", s, p).count(b"\n") == len(recs)


def test_strip_on_records():
    recs = [(b"b", b".A..C-G.."), (b"n", b".AXYCTG..")]
    longest = [1, 2, 0, 0, 2]
    assert KO.strip(recs, longest) == [(b"b", b"AC-G"), (b"n", b"ACTG")]
    assert KO.records_of_merged(recs[1][1], longest) == [(1, b"XY")]


def test_hand_derived_rows_and_records():
    """The example of tests/test_place_cpu.py, kept at the backbone's 4 columns."""
    new = [(b"AXYCTG", [0, 1, 1, 0, 0, 0]), (b"ZACTG", [1, 0, 0, 0, 0]), (b"ACG", [0, 0, 2, 0]), (b"ACTGWW", [0, 0, 0, 0, 1, 1]), (b"", [2, 2, 2, 2])]
    assert [KO.keep_row(s, p, 4) for s, p in new] == [b"ACTG", b"ACTG", b"AC-G", b"ACTG", b"----"]
    assert [KO.runs(p) for _, p in new] == [[(1, 1, 2)], [(0, 0, 1)], [], [(4, 4, 2)], []]
    assert KO.insertion_lines(b"s0", *new[0]) == b"s0\t1\tXY\n" and KO.insertion_lines(b"s3", *new[3]) == b"s3\t4\tWW\n"


@pytest.mark.parametrize("spec", PC.PLACE_SPECS + KC.KEEP_SPECS, ids=lambda s: s.name)
def test_specs_reach_their_branches(spec):
    path = spec.path()
    got = dict(PC.classify(path, spec.L))
    got.update(KC.classify_runs(path))
    for key, want in spec.reach.items():
        assert got[key] == want, (spec.name, key, got[key], want)


def test_the_rank_scan_has_its_directed_specs():
    """What the issue lists: run ends on item 15 of a thread and item 0 of the next, 257 and 4097 one-letter runs in one path, a path
    with no run, a path that is one single run with L = 0."""
    got = {s.name: KC.classify_runs(s.path()) for s in KC.KEEP_SPECS}
    assert got["ends_15_and_32"]["end_on_item_15"] and got["ends_15_and_32"]["end_on_item_0"]
    assert got["runs257"]["runs"] == 257 == got["runs257"]["letters"] and got["runs257"]["more_ends_than_threads_in_a_tile"]
    assert got["runs4097"]["runs"] == 4097 == got["runs4097"]["letters"] and got["runs4097"]["more_ends_than_a_tile_of_codes"]
    assert got["no_run"]["runs"] == 0
    one = [s for s in KC.KEEP_SPECS if s.name == "one_run_37"][0]
    assert one.L == 0 and got["one_run_37"]["one_run_is_the_path"]
