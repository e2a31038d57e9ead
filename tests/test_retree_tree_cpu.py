"""The host half of the rebuilt guide tree (guide::distancesFromCounts, guide::upgma and guide::newick of
twilight_amd/csrc/host/guide_upgma.hpp, through tests/retree_kats.cpp) against tests/retree_oracle.py: the distances bit for bit, the Newick
text byte for byte, on the hand-derived alignments and on seeded ones.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import guide_oracle as G
import retree_cases as K
import retree_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    exe = tmp_path_factory.mktemp("retree_kats") / "retree_kats"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tests", "retree_kats.cpp")])

    def run(cases):
        """cases: [(names, match, both)] -> [(distance line, tree text)] from one run of the program"""
        text = []
        for names, match, both in cases:
            text.append("%d\n%s\n%s\n%s\n" % (len(names), " ".join(names), " ".join(str(int(x)) for x in np.asarray(match).reshape(-1)),
                                              " ".join(str(int(x)) for x in np.asarray(both).reshape(-1))))
        r = subprocess.run([str(exe)], input="".join(text), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines(keepends=True)
        assert len(lines) == 2 * len(cases)
        return list(zip(lines[0::2], lines[1::2]))

    return run


def _want(names, match, both):
    d = R.distances(np.asarray(match, dtype=np.uint32), np.asarray(both, dtype=np.uint32))
    n = len(names)
    return [float(d[a, b]) for a in range(n) for b in range(a + 1, n)], G.upgma_newick(names, d)


def _check(got, names, match, both):
    dist, tree = _want(names, match, both)
    assert [float.fromhex(x) for x in got[0].split()] == dist
    assert got[1] == tree


def test_hand_derived_counts_and_trees(kats):
    cases = [(c["names"], c["match"], c["both"]) for _, c in sorted(K.HAND.items())]
    got = kats(cases)
    for g, (name, c) in zip(got, sorted(K.HAND.items())):
        _check(g, c["names"], c["match"], c["both"])
        assert g[1] == c["tree"], name


def test_both_zero_gives_distance_one(kats):
    names = ["a", "b", "c"]
    match = [[3, 0, 1], [0, 0, 0], [1, 0, 2]]
    both = [[3, 0, 2], [0, 0, 0], [2, 0, 2]]
    (dist, tree), = kats([(names, match, both)])
    assert [float.fromhex(x) for x in dist.split()] == [1.0, 0.5, 1.0]
    assert tree == "((a:0.250000,c:0.250000):0.250000,b:0.500000);\n"


@pytest.mark.parametrize("type_,n,width", [("n", 2, 5), ("n", 17, 90), ("p", 12, 60), ("n", 40, 33)])
def test_seeded_alignments(kats, type_, n, width):
    """Counts from the restatement, many ties among them (short rows): the C++ must break them the same way."""
    rows = K.seeded_rows(type_, n, width, seed=n * 1000 + width)
    match, both, _ = R.pair_counts(rows, type_, R.max_gaps(0.95, n))
    names = ["s%d" % i for i in range(n)]
    (g,) = kats([(names, match, both)])
    _check(g, names, match, both)
