"""twl_guide_shared on the MI355X against sum_b min(c_i[b], c_j[b]) of the numpy restatement (tests/guide_oracle.py), exactly: sizes on every
edge of the tile of pairs (taken from twl_guide_describe), symmetry, the diagonal, a guard band behind the output, and a pair whose
shared count does not fit 16 bits."""
import numpy as np
import pytest

import guide_oracle as O

pytestmark = pytest.mark.gpu

VALID = {"n": b"ACGT", "p": b"AGPSTCDENQFWYHKRILMV"}
GUARD = 256


def _family(type_, n, seed):
    """n sequences of 200-400 letters: mutated pieces of three unrelated ancestors, so that the shared counts spread from 0 to w."""
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
    """(sequences, S) of the family of n sequences; computed once per size and shared, never changed."""
    if (type_, n) not in _REF:
        seqs = _family(type_, n, 100 + n)
        s = O.shared_counts(O.counts_matrix(seqs, type_))
        s.setflags(write=False)
        _REF[(type_, n)] = (seqs, s)
    return _REF[(type_, n)]


def _sizes():
    from twilight_amd import guide

    t = guide.describe()["pair_tile"]
    return [1, 2, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("which", range(6))
def test_sizes_on_every_edge_of_the_pair_tile(gpu, which):
    """N = 1, 2, one below, on and one above the tile's edge, twice the edge plus one: exact, symmetric, w on the diagonal, guard untouched."""
    from twilight_amd import guide

    n = _sizes()[which]
    seqs, want = _reference("n", n)
    flat = guide.shared(seqs, "n", guard_words=GUARD)
    assert (flat[n * n:] == 0xFFFFFFFF).all(), "the call wrote behind its n x n output"
    got = flat[: n * n].reshape(n, n)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (n, bad[:5], got[tuple(bad[0])] if len(bad) else None)
    assert (got == got.T).all()
    w = np.array([max(0, len(s) - 5) for s in seqs], dtype=np.uint32)      # all letters valid, no bin near saturation: w = windows
    assert (np.diag(got) == w).all()
    assert got.max() <= w.max() and (got <= np.minimum(w[:, None], w[None, :])).all()


def test_protein_bins_are_padded_with_zero_bins(gpu):
    """7776 bins are no multiple of the staged slice: the padding bins must add nothing.  One tile and a partial one."""
    from twilight_amd import guide

    d = guide.describe()
    assert O.BINS["p"] % d["bin_slice"] != 0 and O.BINS["n"] % d["bin_slice"] == 0
    n = d["pair_tile"] + 1
    seqs, want = _reference("p", n)
    flat = guide.shared(seqs, "p", guard_words=GUARD)
    assert (flat[n * n:] == 0xFFFFFFFF).all()
    got = flat[: n * n].reshape(n, n)
    assert (got == want).all() and (got == got.T).all()


def test_sequences_without_windows(gpu):
    """Empty and shorter than k among ordinary ones: their rows and columns are zero, the diagonal included."""
    from twilight_amd import guide

    seqs, _ = _reference("n", 2)
    seqs = [seqs[0], b"", b"ACGTA", seqs[1], b"NNNNNNNNNNNN"]
    got = guide.shared(seqs, "n")
    want = O.shared_counts(O.counts_matrix(seqs, "n"))
    assert (got == want).all()
    for i in (1, 2, 4):
        assert not got[i].any() and not got[:, i].any()


def test_a_shared_count_above_16_bits(gpu):
    """Two identical random sequences of 100 000 letters and an unrelated one: S(0, 1) = w_0 = 99 995 (no bin of a random sequence of this
    length comes near saturation), far above 65 535.  A partial sum held in 16 bits and not flushed in time gets this wrong."""
    from twilight_amd import guide

    rng = np.random.default_rng(20261019)
    a = bytes(rng.choice(list(b"ACGT"), 100000).tolist())
    c = bytes(rng.choice(list(b"ACGT"), 100000).tolist())
    seqs = [a, a, c]
    counts = O.counts_matrix(seqs, "n")
    assert counts.max() < 65535
    want = O.shared_counts(counts)
    assert want[0, 1] == 99995 and want[0, 1] > 65535
    got = guide.shared(seqs, "n")
    print("S =", got.tolist())
    assert (got == want).all()
    assert got[0, 1] == 99995 and got[0, 0] == got[1, 1] == got[2, 2] == 99995 and 65535 < got[0, 2] < 99995


def test_saturated_bins_on_both_sides(gpu):
    """Homopolymers: min(65535, 65535) in one bin, and w is the saturated sum, so d(0, 1) = 0."""
    from twilight_amd import guide

    seqs = [b"A" * 70000, b"A" * 90000, b"A" * 100 + b"C" * 70000]
    got = guide.shared(seqs, "n")
    want = O.shared_counts(O.counts_matrix(seqs, "n"))
    assert (got == want).all() and got[0, 1] == 65535 and got[0, 2] == 95
