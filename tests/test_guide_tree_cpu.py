"""The host clustering and text of the guide tree (twilight_amd/csrc/host/guide_upgma.hpp, through tests/guide_kats.cpp) against the naive
algorithm of tests/guide_oracle.py: the Newick text must be the same, byte for byte, ties included.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import guide_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    exe = tmp_path_factory.mktemp("guide_kats") / "guide_kats"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tests", "guide_kats.cpp")])

    def run(cases):
        """cases: [(names, matrix)] -> the text of each, from one run of the program"""
        text = []
        for names, d in cases:
            d = np.asarray(d, dtype=np.float64)
            text.append("%d\n%s\n%s\n" % (len(names), " ".join(names), " ".join(float(x).hex() for x in d.reshape(-1))))
        r = subprocess.run([str(exe)], input="".join(text), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines(keepends=True)
        assert len(lines) == len(cases)
        return lines

    return run


def _sym(rows):
    d = np.array(rows, dtype=np.float64)
    return np.triu(d, 1) + np.triu(d, 1).T


def _names(n):
    return ["s%d" % i for i in range(n)]


def test_hand_derived_trees(kats):
    """N = 2, 3, 4, worked by hand from the definition."""
    two = (["a", "b"], _sym([[0, 0.5], [0, 0]]))
    # (a, b) at 0.2 -> height 0.1; d(ab, c) = (0.6 + 0.8) / 2 = 0.7 -> height 0.35
    three = (["a", "b", "c"], _sym([[0, 0.2, 0.6], [0, 0, 0.8], [0, 0, 0]]))
    # (c, d) at 0.1 -> 0.05, slot 2; (a, b) at 0.3 -> 0.15, slot 0; d(ab, cd) = all four 0.75 -> 0.375
    four = (["a", "b", "c", "d"], _sym([[0, 0.3, 0.75, 0.75], [0, 0, 0.75, 0.75], [0, 0, 0, 0.1], [0, 0, 0, 0]]))
    got = kats([two, three, four])
    assert got[0] == "(a:0.250000,b:0.250000);\n"
    assert got[1] == "((a:0.100000,b:0.100000):0.250000,c:0.350000);\n"
    assert got[2] == "((a:0.150000,b:0.150000):0.225000,(c:0.050000,d:0.050000):0.325000);\n"
    for (names, d), text in zip([two, three, four], got):
        assert O.upgma_newick(names, d) == text


def test_every_step_a_tie(kats):
    """All distances equal: every step joins slot 0 and the smallest live slot behind it."""
    for n in (3, 7, 20):
        d = np.full((n, n), 0.625)
        np.fill_diagonal(d, 0)
        (got,) = kats([(_names(n), d)])
        assert got == O.upgma_newick(_names(n), d)
        assert got.startswith("(" * (n - 1) + "s0:0.312500,s1:0.312500)")


def test_two_exact_ties_at_different_steps(kats):
    """(0,1) and (2,3) tie at 0.25 in the first step: (0,1) goes first; then (2,3) at 0.25 against nothing; then d(01,4) = d(23,4) = 0.5 tie
    against d(01,23) = 0.75: slot 0 joins 4 before slot 2 could; the root is at (2 * 0.75 + 0.5) / 3 / 2 = 1/3."""
    d = _sym([[0, 0.25, 0.75, 0.75, 0.5], [0, 0, 0.75, 0.75, 0.5], [0, 0, 0, 0.25, 0.5], [0, 0, 0, 0, 0.5], [0, 0, 0, 0, 0]])
    (got,) = kats([(_names(5), d)])
    assert got == O.upgma_newick(_names(5), d)
    assert got == "(((s0:0.125000,s1:0.125000):0.125000,s4:0.250000):0.083333,(s2:0.125000,s3:0.125000):0.208333);\n"


def test_identical_sequences_and_a_sequence_without_windows(kats):
    """From real counts: sequences 0 and 2 are identical (d = 0), sequence 3 is shorter than k (d = 1 to all)."""
    rng = np.random.default_rng(5)
    base = bytes(rng.choice(list(b"ACGT"), 300).tolist())
    other = bytes(rng.choice(list(b"ACGT"), 280).tolist())
    seqs = [base, other, base, b"ACG", base[:150] + other[150:]]
    d = O.distances(O.shared_counts(O.counts_matrix(seqs, "n")))
    assert d[0, 2] == 0 and (d[3, [0, 1, 2, 4]] == 1).all()
    (got,) = kats([(_names(5), d)])
    assert got == O.upgma_newick(_names(5), d)
    assert "(s0:0.000000,s2:0.000000)" in got and got.endswith(",s3:0.500000);\n")


def test_seeded_random_matrices(kats):
    """50 matrices of N = 5 .. 60; half of them drawn from a few values only, so that ties are everywhere."""
    rng = np.random.default_rng(20261019)
    cases = []
    for t in range(50):
        n = int(rng.integers(5, 61))
        if t % 2:
            d = rng.choice([0.0, 0.125, 0.25, 0.3, 0.7, 1.0], size=(n, n))
        else:
            d = rng.random((n, n))
        cases.append((_names(n), _sym(d)))
    got = kats(cases)
    for (names, d), text in zip(cases, got):
        assert text == O.upgma_newick(names, d), len(names)


def test_the_host_file_is_built_without_contraction():
    import __graft_entry__ as g

    assert "-ffp-contract=off" in g.HOST_FLAGS
    assert "guide.cpp" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
