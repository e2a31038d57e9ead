"""twl_guide_kmer_counts on the MI355X against the numpy restatement (tests/guide_oracle.py), bit for bit, for both types: lengths on every
edge of the count kernel (taken from twl_guide_describe), invalid bytes, case, U against T, a bin that saturates."""
import numpy as np
import pytest

import guide_oracle as O

pytestmark = pytest.mark.gpu

VALID = {"n": b"ACGT", "p": b"AGPSTCDENQFWYHKRILMV"}
INVALID = {"n": b"N", "p": b"X"}


def _random(rng, type_, length):
    return bytes(rng.choice(list(VALID[type_]), length).tolist()) if length else b""


def _check(guide, seqs, type_):
    got = guide.kmer_counts(seqs, type_)
    want = O.counts_matrix(seqs, type_)
    assert got.dtype == np.uint16 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (type_, [len(s) for s in seqs], bad[:5])
    return got


@pytest.mark.parametrize("type_", ["n", "p"])
def test_lengths_on_every_edge(gpu, type_):
    """0, k-1, k, k+1, the fixed list, and one below, on and one above every length at which the windows fill a thread's chunk, two chunks,
    a workgroup's round and two rounds (lengths = windows + k - 1)."""
    from twilight_amd import guide

    k, d = O.K[type_], guide.describe()
    lengths = {0, 1, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025}
    for windows in (d["count_chunk"], 2 * d["count_chunk"], d["count_round"] - d["count_chunk"], d["count_round"], 2 * d["count_round"]):
        for delta in (-1, 0, 1):
            lengths.add(windows + k - 1 + delta)
    rng = np.random.default_rng(11)
    seqs = [_random(rng, type_, L) for L in sorted(lengths)]
    got = _check(guide, seqs, type_)
    for s, row in zip(seqs, got):
        assert int(row.sum()) == max(0, len(s) - k + 1)      # every window of a sequence of valid letters lands in one bin


@pytest.mark.parametrize("type_", ["n", "p"])
def test_an_invalid_byte_removes_exactly_its_windows(gpu, type_):
    from twilight_amd import guide

    k, L = O.K[type_], 300
    rng = np.random.default_rng(12)
    base = _random(rng, type_, L)
    places = list(range(k)) + list(range(L - k, L)) + [150]
    seqs = [base] + [base[:p] + INVALID[type_] + base[p + 1:] for p in places]
    got = _check(guide, seqs, type_).astype(np.int64)
    for p, row in zip(places, got[1:]):
        lost = min(p, L - k) - max(p - k + 1, 0) + 1      # windows that start in [p - k + 1, p] and exist
        assert int(row.sum()) == L - k + 1 - lost, p
        assert (row <= got[0]).all()                      # ... and no window moved to another bin


def test_every_other_protein_byte_is_invalid(gpu):
    from twilight_amd import guide

    rng = np.random.default_rng(13)
    base = _random(rng, "p", 120)
    seqs = [base[:60] + bytes([c]) + base[61:] for c in b"BZXJUO*-.bzxjuo" + bytes([0, 10, 64, 91, 96, 123, 200, 255])]
    got = _check(guide, seqs, "p")
    assert (got.sum(axis=1) == 120 - 5 + 1 - 5).all()


@pytest.mark.parametrize("type_", ["n", "p"])
def test_lower_case_counts_as_upper_case(gpu, type_):
    from twilight_amd import guide

    rng = np.random.default_rng(14)
    s = _random(rng, type_, 777)
    mixed = bytes(c | 0x20 if i % 3 else c for i, c in enumerate(s))
    got = _check(guide, [s, s.lower(), mixed], type_)
    assert (got[0] == got[1]).all() and (got[0] == got[2]).all() and got[0].sum() == 777 - O.K[type_] + 1


def test_u_counts_as_t(gpu):
    from twilight_amd import guide

    rng = np.random.default_rng(15)
    s = _random(rng, "n", 500)
    got = _check(guide, [s, s.replace(b"T", b"U"), s.replace(b"T", b"u")], "n")
    assert (got[0] == got[1]).all() and (got[0] == got[2]).all()
    # ... while U is no letter of the protein alphabet
    assert guide.kmer_counts([b"UUUUUUUUUU"], "p").sum() == 0


def test_a_bin_saturates_at_65535(gpu):
    """A homopolymer of 70 000 letters: 69 995 windows in bin 0 (AAAAAA), kept as 65 535; a second sequence beside it is not disturbed."""
    from twilight_amd import guide

    got = _check(guide, [b"A" * 70000, b"ACGTACGTAC", b"T" * 65540 + b"G"], "n")
    assert got[0, 0] == 65535 and got[0, 1:].sum() == 0
    assert got[2, 4095] == 65535 and got[2, 4094] == 1      # 65 535 windows TTTTTT exactly (not saturated by one), then TTTTTG
    got = _check(guide, [b"W" * 70000], "p")
    assert got[0, 3 * (1296 + 216 + 36 + 6 + 1)] == 65535 and got.sum() == 65535
