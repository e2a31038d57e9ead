"""twl_guide_set_shared_groups on the MI355X against sum_b min(c_i[b], c_j[b]) of the numpy restatement (tests/guide_oracle.py), exactly: groups
on every edge of the 64 x 64 tile in one call, rows gathered through ids in any order, many groups of one member, and one group of all
rows against twl_guide_shared.  Every call has a guard band behind its output."""
import numpy as np
import pytest

import guide_oracle as O
from test_gpu_guide_assign import _reference

pytestmark = pytest.mark.gpu

GUARD = 256


def _blocks(flat, groups):
    assert (flat[len(flat) - GUARD:] == 0xFFFFFFFF).all(), "the call wrote behind its output"
    at, out = 0, []
    for g in groups:
        out.append(flat[at: at + len(g) ** 2].reshape(len(g), len(g)))
        at += len(g) ** 2
    assert at == len(flat) - GUARD
    return out


def _compare(got, counts, groups):
    for g, block in zip(groups, got):
        want = O.shared_counts(counts[np.asarray(g)])
        assert (block == want).all(), (len(g), np.argwhere(block != want)[:5])
        assert (block == block.T).all()


def test_groups_on_every_edge_of_the_tile_in_one_call(gpu):
    """Sizes 65, 1, 130, 2, 64, 63 in this order over a set of 200 sequences; the ids are a shuffle, a descending run, every third row ... and
    some rows serve two groups."""
    from twilight_amd import guide

    seqs, counts = _reference("n", 200)
    rng = np.random.default_rng(3)
    groups = [[int(x) for x in rng.permutation(200)[:65]], [199], list(range(199, 69, -1)), [150, 7], list(range(0, 192, 3)), [int(x) for x in rng.permutation(200)[:63]]]
    assert [len(g) for g in groups] == [65, 1, 130, 2, 64, 63]
    with guide.GuideSet(seqs, "n") as gs:
        flat = gs.shared_groups(groups, guard_words=GUARD)
        count_ms, assign_ms, groups_ms, download_ms = gs.timing()
    _compare(_blocks(flat, groups), counts, groups)
    assert count_ms > 0 and groups_ms > 0 and download_ms > 0 and assign_ms == 0


def test_300_groups_of_one_member(gpu):
    from twilight_amd import guide

    seqs, counts = _reference("n", 200)
    groups = [[(7 * g) % 200] for g in range(300)]
    with guide.GuideSet(seqs, "n") as gs:
        flat = gs.shared_groups(groups, guard_words=GUARD)
        w = gs.weights()
    assert (flat[300:] == 0xFFFFFFFF).all()
    assert (flat[:300] == w[[g[0] for g in groups]]).all()
    assert (w == counts.astype(np.int64).sum(axis=1)).all()


def test_one_group_of_all_rows_is_twl_guide_shared(gpu):
    from twilight_amd import guide

    seqs, counts = _reference("n", 130)
    with guide.GuideSet(seqs, "n") as gs:
        flat = gs.shared_groups([list(range(130))], guard_words=GUARD)
    (block,) = _blocks(flat, [list(range(130))])
    assert (block == guide.shared(seqs, "n")).all()
    assert (block == O.shared_counts(counts)).all()


def test_protein_groups(gpu):
    """7776 bins are no multiple of the staged slice: the padding bins must add nothing.  A tile and a partial one, and a group of 3."""
    from twilight_amd import guide

    seqs, counts = _reference("p", 65)
    groups = [list(range(64, -1, -1)), [3, 60, 9]]
    with guide.GuideSet(seqs, "p") as gs:
        flat = gs.shared_groups(groups, guard_words=GUARD)
    _compare(_blocks(flat, groups), counts, groups)
