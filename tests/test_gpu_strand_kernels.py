"""The strand calls on the MI355X (include/twl_strand.h), exactly:
twl_guide_set_opposite against twl_guide_shared on the family followed by its reverse complements (O(a, b) is the cross block; no oracle in
between), and twl_guide_set_strand_assign against the restatement (tests/strand_oracle.py) in t, d and s.  Sizes on every edge of the 64-row
tile of sequences and of the 64-seed tile, taken from twl_guide_describe; mixed seed flips; rows without windows, a palindromic row, two
identical seeds, a row that is the reverse complement of a flipped seed, the saturated homopolymer, seeds in the last partial tile."""
import numpy as np
import pytest

import guide_oracle as G
import strand_oracle as SO

pytestmark = pytest.mark.gpu

LETTERS = np.array(list(b"ACGT"), dtype=np.uint8)
_REF = {}


def _tile():
    from twilight_amd import guide

    return guide.describe()["pair_tile"]


def _family(n, seed):
    """n sequences of 200-400 letters: mutated pieces of three unrelated ancestors, every third of them reverse-complemented at random."""
    rng = np.random.default_rng(seed)
    anc = [rng.choice(LETTERS, 400) for _ in range(3)]
    out = []
    for _ in range(n):
        s = anc[int(rng.integers(0, 3))][: int(rng.integers(200, 401))].copy()
        hit = rng.random(len(s)) < rng.choice([0.0, 0.02, 0.1])
        s[hit] = rng.choice(LETTERS, int(hit.sum()))
        b = s.tobytes()
        out.append(SO.reverse_complement(b) if rng.random() < 0.33 else b)
    return out


def _reference(n):
    """(sequences, counts) of the family of n sequences; computed once per size and shared, never changed."""
    if n not in _REF:
        seqs = _family(n, 700 + n)
        counts = G.counts_matrix(seqs, "n")
        counts.setflags(write=False)
        _REF[n] = (seqs, counts)
    return _REF[n]


# ---- twl_guide_set_opposite ----

def _check_opposite(seqs, ids):
    from twilight_amd import guide, strand

    chosen = [seqs[i] for i in ids]
    m = len(ids)
    both = guide.shared(chosen + [SO.reverse_complement(s) for s in chosen], "n")
    with guide.GuideSet(seqs, "n") as gs:
        flat = strand.opposite(gs, ids, guard_words=4)
        t = strand.timing(gs)
    assert (flat[m * m:] == 0xFFFFFFFF).all(), "the call wrote behind its output"
    got = flat[: m * m].reshape(m, m)
    assert (got == both[:m, m:]).all(), np.argwhere(got != both[:m, m:])[:5]
    assert (got == got.T).all()
    assert t[0] > 0 and t[2] > 0 and t[1] == 0
    return got


@pytest.mark.parametrize("edge", ["one", "below", "on", "above", "two_tiles_plus_two"])
def test_opposite_is_the_cross_block_of_the_shared_counts(gpu, edge):
    T = _tile()
    n = {"one": 1, "below": T - 1, "on": T, "above": T + 1, "two_tiles_plus_two": 2 * T + 2}[edge]
    seqs, _ = _reference(n)
    got = _check_opposite(seqs, list(range(n)))
    assert n == 1 or len(set(got.flatten().tolist())) > 2


def test_opposite_of_a_shuffled_part_of_a_larger_set(gpu):
    """The ids are positions in the set, in any order; rows that are not listed play no part.  Rows without windows and a saturated row among them."""
    T = _tile()
    seqs = list(_reference(2 * T + 2)[0])
    seqs[3], seqs[T], seqs[T + 5] = b"", b"ACGTA", b"A" * 70000 + seqs[T + 5]
    rng = np.random.default_rng(11)
    ids = [int(x) for x in rng.permutation(len(seqs))[: T + 9]]
    for must in (3, T, T + 5):
        if must not in ids:
            ids[must % len(ids)] = must
    assert len(set(ids)) == len(ids) and ids != sorted(ids)
    _check_opposite(seqs, ids)


# ---- twl_guide_set_strand_assign ----

def _check_assign(seqs, counts, seeds, flip, want_shared=True):
    from twilight_amd import guide, strand

    want_t, want_d, want_s = SO.assign(counts, list(seeds), flip)
    with guide.GuideSet(seqs, "n") as gs:
        got_t, got_d, got_s = strand.assign(gs, seeds, flip, want_shared=want_shared)
        t = strand.timing(gs)
        assert gs.timing()[1] == 0      # twl_guide_set_timing does not count the strand calls
    bad = np.flatnonzero((got_t != want_t) | (got_d != want_d))
    assert len(bad) == 0, (len(seqs), len(seeds), bad[:5], got_t[bad[:5]], want_t[bad[:5]], got_d[bad[:5]], want_d[bad[:5]])
    if want_shared:
        assert (got_s == want_s).all(), np.flatnonzero(got_s != want_s)[:5]
    else:
        assert got_s is None
    assert t[0] > 0 and t[1] > 0 and t[2] == 0
    return got_t, got_d


def _sizes():
    """(sequences, seeds): 1, T - 1, T, T + 1 and 2 T + 1 rows that are no seeds or all rows; 1, T - 1, T, T + 1 and 2 T + 2 seeds."""
    T = _tile()
    return [(1, 1), (T - 1, 1), (T - 1, T - 1), (T, T), (T + 1, T), (T + 1, T + 1), (2 * T + 1, 1), (2 * T + 1, T - 1), (2 * T + 1, T + 1), (2 * T + 2, 2 * T + 2),
            (4 * T + 3, 2 * T + 2)]


@pytest.mark.parametrize("k", range(11))
def test_sizes_on_every_edge_of_both_tiles_with_mixed_flips(gpu, k):
    n, s = _sizes()[k]
    seqs, counts = _reference(n)
    rng = np.random.default_rng(50 + k)
    flip = rng.integers(0, 2, s).astype(np.uint8)
    seeds = SO.seed_ids(n, s)
    got_t, got_d = _check_assign(seqs, counts, seeds, flip)
    for t, i in enumerate(seeds):
        assert got_t[i] == t and got_d[i] == flip[t]      # a seed goes to itself, in its own direction
    assert n < 60 or s < 2 or (len(set(got_t.tolist())) > 1 and len(set(got_d.tolist())) == 2)


def test_seeds_out_of_order_and_in_the_last_partial_tile(gpu):
    """seed_ids shuffled: t is the position in the list; the rows of the last, partial tile of sequences are seeds too."""
    T = _tile()
    n = 2 * T + 2
    seqs, counts = _reference(n)
    rng = np.random.default_rng(5)
    seeds = [int(x) for x in rng.permutation(n)[: T + 6]]
    for must in (n - 1, n - 2):
        if must not in seeds:
            seeds[must % len(seeds)] = must
    assert len(set(seeds)) == len(seeds) and seeds != sorted(seeds)
    flip = rng.integers(0, 2, len(seeds)).astype(np.uint8)
    _check_assign(seqs, counts, seeds, flip)
    _check_assign(seqs, counts, seeds, flip, want_shared=False)


def test_rows_without_windows_and_a_seed_without_windows(gpu):
    """w = 0: the ratio is 0 / 1 with every candidate, so the row lands on seed 0 in the direction 0, whatever seed 0's flip (d = r XOR flip)."""
    T = _tile()
    seqs = list(_reference(T + 1)[0])
    seqs[10], seqs[20], seqs[T] = b"ACGTA", b"", b"NNNNNNNNNNNNNN"
    counts = G.counts_matrix(seqs, "n")
    for flip in ([1, 0, 1, 0, 1], [0, 1, 0, 1, 0]):
        got_t, got_d = _check_assign(seqs, counts, [5, 20, 40, T, T - 1], np.array(flip, dtype=np.uint8))      # 20 and T are seeds without windows
        assert got_t[10] == 0 and got_d[10] == 0 and got_t[20] == 1 and got_d[20] == flip[1] and got_t[T] == 3 and got_d[T] == flip[3]
    got_t, got_d = _check_assign(seqs, counts, [20, 5, 40], np.array([1, 0, 0], dtype=np.uint8))                  # a seed without windows first
    assert got_t[10] == 0 and got_d[10] == 0 and got_t[T] == 0 and got_d[T] == 0


@pytest.mark.parametrize("flip_x", [0, 1])
def test_a_palindromic_row_goes_forward(gpu, flip_x):
    """A row that is its own reverse complement shares as much with a seed as with the seed's reverse complement (S == O): the smaller d wins,
    so it stays forward whatever the seed's flip."""
    rng = np.random.default_rng(21)
    half = rng.choice(LETTERS, 150).tobytes()
    pal = half + SO.reverse_complement(half)
    assert SO.reverse_complement(pal) == pal
    x = rng.choice(LETTERS, 300)
    near = x.copy()
    near[::40] = LETTERS[(np.searchsorted(LETTERS, near[::40]) + 1) % 4]
    seqs = [x.tobytes(), pal, near.tobytes(), rng.choice(LETTERS, 300).tobytes(), pal[:280]]
    counts = G.counts_matrix(seqs, "n")
    got_t, got_d = _check_assign(seqs, counts, [0, 3], np.array([flip_x, 0], dtype=np.uint8))
    assert got_d[1] == 0
    assert got_t[2] == 0 and got_d[2] == flip_x


@pytest.mark.parametrize("ta,tb", [(3, 19), (3, 4), (3, 67), (0, 63)])
def test_two_identical_seeds_the_smaller_t_wins(gpu, ta, tb):
    """Seeds ta < tb are one text X (columns of one thread, of two lanes, of two seed tiles); tb is flipped, ta is not.  Every mutant of X has the
    same ratio with both: it goes to ta, forward.  A mutant of rc(X) goes to ta as well, reversed."""
    rng = np.random.default_rng(1000 + 100 * ta + tb)
    x = rng.choice(LETTERS, 300)
    others = [rng.choice(LETTERS, 300).tobytes() for _ in range(67)]
    mutants = []
    for i in range(20):
        m = x.copy()
        hit = rng.random(300) < 0.03
        m[hit] = rng.choice(LETTERS, int(hit.sum()))
        mutants.append(m.tobytes() if i % 2 == 0 else SO.reverse_complement(m.tobytes()))
    seqs = [x.tobytes()] + others + [x.tobytes()] + mutants      # ids: 0 = X, 1 .. 67 others, 68 = X, 69 .. 88 mutants
    seeds = list(range(1, 68))
    seeds.insert(ta, 68)
    seeds.insert(tb, 0)
    assert len(seeds) == 69 and seeds[ta] == 68 and seeds[tb] == 0
    flip = np.zeros(69, dtype=np.uint8)
    flip[tb] = 1
    counts = G.counts_matrix(seqs, "n")
    got_t, got_d = _check_assign(seqs, counts, seeds, flip)
    assert (got_t[69:] == ta).all(), got_t[69:]
    assert got_d[69:].tolist() == [i % 2 for i in range(20)]


def test_a_row_that_is_the_reverse_complement_of_a_flipped_seed(gpu):
    """Seed X lies reversed (flip 1).  rc(X) shares everything with X's opposite strand: r = 1, d = 1 XOR 1 = 0, it is forward; a copy of X shares
    everything on the same strand: r = 0, d = 1, it is turned with its seed."""
    rng = np.random.default_rng(33)
    x = rng.choice(LETTERS, 300).tobytes()
    y = rng.choice(LETTERS, 300).tobytes()
    seqs = [y, x, SO.reverse_complement(x), x, SO.reverse_complement(y)]
    counts = G.counts_matrix(seqs, "n")
    got_t, got_d = _check_assign(seqs, counts, [0, 1], np.array([0, 1], dtype=np.uint8))
    assert got_t.tolist() == [0, 1, 1, 1, 0] and got_d.tolist() == [0, 1, 0, 1, 1]


def test_the_saturated_homopolymer(gpu):
    """70 000 A: the bin AAAAAA is at 65 535 and so is TTTTTT of its reverse complement; saturation is symmetric under the permutation."""
    rng = np.random.default_rng(9)
    rnd = [rng.choice(LETTERS, 300).tobytes() for _ in range(4)]
    seqs = [b"A" * 70000, rnd[0], b"T" * 90000, rnd[1], b"A" * 100 + b"C" * 70000, rnd[2], b"T" * 500 + rnd[3], b"G" * 70000 + b"T" * 100]
    counts = G.counts_matrix(seqs, "n")
    assert counts.max() == 65535
    got_t, got_d = _check_assign(seqs, counts, [0, 1, 4], np.array([0, 1, 1], dtype=np.uint8))
    assert got_t[2] == 0 and got_d[2] == 1      # T x 90 000 is the homopolymer's reverse complement, as saturated: ratio 1 on the opposite strand
    assert got_t[7] == 2 and got_d[7] == 0      # rc(seed 4) with seed 4 flipped: forward
    _check_assign(seqs, counts, [1, 6, 3], np.array([1, 0, 1], dtype=np.uint8))


def test_the_calls_refuse_what_the_plan_refuses(gpu):
    from twilight_amd import guide, strand

    seqs, _ = _reference(_tile() + 1)
    with guide.GuideSet(seqs, "n") as gs:
        with pytest.raises(gpu.TwlError, match="seed id out of range"):
            strand.assign(gs, [0, len(seqs)], [0, 0])
        with pytest.raises(gpu.TwlError, match="the same sequence is a seed twice"):
            strand.assign(gs, [2, 2], [0, 0])
        with pytest.raises(gpu.TwlError, match="a seed's flip must be 0 or 1"):
            strand.assign(gs, [0, 1], [0, 2])
        with pytest.raises(gpu.TwlError, match="the same sequence is listed twice"):
            strand.opposite(gs, [1, 1])
        with pytest.raises(gpu.TwlError, match="id out of range"):
            strand.opposite(gs, [-1])
    with guide.GuideSet([b"MKVLEEFQIL", b"MKVLEEFQIP"], "p") as gs:
        with pytest.raises(gpu.TwlError, match="nucleotide"):
            strand.opposite(gs, [0, 1])
        with pytest.raises(gpu.TwlError, match="nucleotide"):
            strand.assign(gs, [0], [0])
