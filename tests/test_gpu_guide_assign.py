"""twl_guide_set_assign on the MI355X against the assignment rule restated in Python integers (tests/guide_stage_oracle.py), exactly: the seed
every sequence goes to and the shared count with it.  Sizes on every edge of the 64-row tile of sequences and of the 64-seed tile, equal
ratios wherever two candidates of a row meet (two columns of one thread, two lanes of a row, two seed tiles), seeds out of order, sequences
and seeds without windows, a saturated bin, protein bins, and a call without shared_out."""
import numpy as np
import pytest

import guide_oracle as O
import guide_stage_oracle as G

pytestmark = pytest.mark.gpu

VALID = {"n": b"ACGT", "p": b"AGPSTCDENQFWYHKRILMV"}


def _family(type_, n, seed):
    """n sequences of 200-400 letters: mutated pieces of three unrelated ancestors, so that the ratios spread from 0 to 1."""
    rng = np.random.default_rng(seed)
    letters = np.array(list(VALID[type_]), dtype=np.uint8)
    anc = [rng.choice(letters, 400) for _ in range(3)]
    out = []
    for i in range(n):
        s = anc[int(rng.integers(0, 3))][: int(rng.integers(200, 401))].copy()
        hit = rng.random(len(s)) < rng.choice([0.0, 0.02, 0.1])
        s[hit] = rng.choice(letters, int(hit.sum()))
        out.append(s.tobytes())
    return out


_REF = {}


def _reference(type_, n):
    """(sequences, counts) of the family of n sequences; computed once per size and shared, never changed."""
    if (type_, n) not in _REF:
        seqs = _family(type_, n, 300 + n)
        counts = O.counts_matrix(seqs, type_)
        counts.setflags(write=False)
        _REF[(type_, n)] = (seqs, counts)
    return _REF[(type_, n)]


def _check(seqs, counts, type_, seeds, want_shared=True):
    from twilight_amd import guide

    want_seed, want_s = G.assign(counts, list(seeds))
    with guide.GuideSet(seqs, type_) as gs:
        assert (gs.weights() == counts.astype(np.int64).sum(axis=1)).all()
        got_seed, got_s = gs.assign(seeds, want_shared=want_shared)
    bad = np.flatnonzero(got_seed != np.array(want_seed))
    assert len(bad) == 0, (len(seqs), len(seeds), bad[:5], got_seed[bad[:5]], [want_seed[i] for i in bad[:5]])
    if want_shared:
        assert (got_s == np.array(want_s, dtype=np.uint32)).all()
    else:
        assert got_s is None
    return got_seed


@pytest.mark.parametrize("n,s", [(63, 2), (63, 63), (64, 64), (64, 63), (65, 65), (65, 64), (130, 2), (130, 63), (130, 65), (130, 129)])
def test_sizes_on_every_edge_of_both_tiles(gpu, n, s):
    """N one below, on and one above the tile of sequences and two tiles plus two; S = 2, one below, on and one above the tile of seeds, two
    tiles plus one.  The seeds are those of the stride rule."""
    seqs, counts = _reference("n", n)
    got = _check(seqs, counts, "n", G.seed_ids(n, s))
    assert len(set(got.tolist())) > 1


def test_seeds_out_of_order(gpu):
    """seed_ids in a shuffled order: t is the position in the list, not the id."""
    seqs, counts = _reference("n", 130)
    rng = np.random.default_rng(5)
    seeds = [int(x) for x in rng.permutation(130)[:70]]
    assert seeds != sorted(seeds)
    got = _check(seqs, counts, "n", seeds)
    for t, i in enumerate(seeds):
        assert got[i] == t      # a seed belongs to its own cluster


@pytest.mark.parametrize("ta,tb", [(3, 19), (3, 4), (3, 67), (19, 67), (64, 128), (0, 63)])
def test_equal_ratios_go_to_the_smaller_t(gpu, ta, tb):
    """Seeds ta < tb are one text X, the other 127 seeds are unrelated to it.  Columns t and t + 16 belong to one thread, t and t + 1 to two lanes
    of a row, t and t + 64 to two seed tiles.  Every mutant of X, and a copy of X that is no seed, has the same ratio with both: ta wins.
    The sequence at ta has the LARGER id, so that an order by id would show."""
    rng = np.random.default_rng(1000 + 100 * ta + tb)
    letters = np.array(list(b"ACGT"), dtype=np.uint8)
    x = rng.choice(letters, 300)
    others = [rng.choice(letters, 300).tobytes() for _ in range(127)]
    mutants = []
    for i in range(40):
        m = x.copy()
        hit = rng.random(300) < 0.03
        m[hit] = rng.choice(letters, int(hit.sum()))
        mutants.append(m.tobytes())
    seqs = [x.tobytes()] + others + [x.tobytes()] + mutants + [x.tobytes()]      # ids: 0 = X, 1 .. 127 others, 128 = X, 129 .. 168 mutants, 169 = X
    seeds = list(range(1, 128))
    seeds.insert(ta, 128)
    seeds.insert(tb, 0)
    assert len(seeds) == 129 and seeds[ta] == 128 and seeds[tb] == 0
    counts = O.counts_matrix(seqs, "n")
    got = _check(seqs, counts, "n", seeds)
    assert got[128] == ta and got[0] == tb
    assert (got[129:] == ta).all(), got[129:]


def test_sequences_and_seeds_without_windows(gpu):
    """w = 0: the ratio is 0 / 1 with every seed, so such a sequence lands on seed 0; a seed with w = 0 keeps itself and attracts only what is
    at ratio 0 with every seed before it."""
    seqs, counts = _reference("n", 65)
    seqs = list(seqs)
    seqs[10], seqs[20], seqs[64] = b"ACGTA", b"", b"NNNNNNNNNNNNNN"
    counts = O.counts_matrix(seqs, "n")
    got = _check(seqs, counts, "n", [5, 20, 40, 64, 63])      # 20 and 64 are seeds without windows
    assert got[10] == 0 and got[20] == 1 and got[64] == 3
    got = _check(seqs, counts, "n", [20, 5, 40])              # a seed without windows first: everything at ratio 0 with all seeds goes to it
    assert got[10] == 0 and got[64] == 0


def test_a_saturated_bin_as_sequence_and_as_seed(gpu):
    """A homopolymer of 70 000 letters has one bin at 65 535, and w is the saturated sum."""
    rng = np.random.default_rng(9)
    rnd = [bytes(rng.choice(list(b"ACGT"), 300).tolist()) for _ in range(4)]
    seqs = [b"A" * 70000, rnd[0], b"A" * 90000, rnd[1], b"A" * 100 + b"C" * 70000, rnd[2], b"A" * 500 + rnd[3]]
    counts = O.counts_matrix(seqs, "n")
    assert counts.max() == 65535
    got = _check(seqs, counts, "n", [0, 1, 4])      # the homopolymer as seed; 2 is as saturated as 0: ratio 1
    assert got[2] == 0
    got = _check(seqs, counts, "n", [1, 6, 3])      # ... and as a sequence among seeds it shares few windows with
    assert got[0] == 1 and got[2] == 1


def test_protein_bins(gpu):
    """7776 bins are no multiple of the staged slice: the padding bins must add nothing."""
    seqs, counts = _reference("p", 65)
    _check(seqs, counts, "p", G.seed_ids(65, 7))


def test_without_shared_out(gpu):
    seqs, counts = _reference("n", 65)
    _check(seqs, counts, "n", G.seed_ids(65, 9), want_shared=False)
