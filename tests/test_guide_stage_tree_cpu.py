"""The host steps of the two-stage guide tree (twilight_amd/csrc/host/guide_stage.hpp, through tests/guide_stage_kats.cpp) against
tests/guide_stage_oracle.py on given assignments and distance matrices: the seed ids and the grafted Newick text must be the same, byte for
byte, ties and negative branch lengths included.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import guide_oracle as O
import guide_stage_oracle as G
from test_guide_stage_oracle_cpu import HAND, HAND_NAMES, HAND_TREE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    exe = tmp_path_factory.mktemp("guide_stage_kats") / "guide_stage_kats"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tests", "guide_stage_kats.cpp")])

    def run(cases):
        """cases: [(names, n_seeds, seed_of, matrix)] -> [(seed ids, text)] from one run of the program"""
        text = []
        for names, s, seed_of, d in cases:
            d = np.asarray(d, dtype=np.float64)
            text.append("%d %d\n%s\n%s\n%s\n" % (len(names), s, " ".join(names), " ".join(map(str, seed_of)), " ".join(float(x).hex() for x in d.reshape(-1))))
        r = subprocess.run([str(exe)], input="".join(text), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines(keepends=True)
        assert len(lines) == 2 * len(cases)
        return [([int(x) for x in lines[2 * i].split()], lines[2 * i + 1]) for i in range(len(cases))]

    return run


def _want(names, s, seed_of, d):
    d = np.asarray(d, dtype=np.float64)
    seeds = G.seed_ids(len(names), s)
    parts = []
    for members in G.clusters(s, seed_of):
        parts.append(G.upgma([names[i] for i in members], [0.0] * len(members), d[np.ix_(members, members)]))
    text, _ = G.upgma([p[0] for p in parts], [p[1] for p in parts], d[np.ix_(seeds, seeds)])
    return seeds, text + ";\n"


def test_hand_derived_case(kats):
    d = O.distances(O.shared_counts(O.counts_matrix(HAND, "n")))
    ((seeds, text),) = kats([(HAND_NAMES, 2, [0, 0, 0, 1, 1, 0], d)])
    assert seeds == [0, 3]
    assert text == HAND_TREE
    assert _want(HAND_NAMES, 2, [0, 0, 0, 1, 1, 0], d) == ([0, 3], HAND_TREE)


def test_a_cluster_taller_than_its_parent_gets_a_zero_branch(kats):
    """Seeds 0 and 2 are close (d = 0.1, the seeds' root at 0.05), their clusters are loose (roots at 0.4 and 0.3): both grafted branches
    would be negative and are written as 0.000000."""
    d = np.array([[0, 0.8, 0.1, 0.9], [0.8, 0, 0.9, 0.9], [0.1, 0.9, 0, 0.6], [0.9, 0.9, 0.6, 0]])
    ((seeds, text),) = kats([(["a", "b", "c", "d"], 2, [0, 0, 1, 1], d)])
    assert seeds == [0, 2]
    assert text == "((a:0.400000,b:0.400000):0.000000,(c:0.300000,d:0.300000):0.000000);\n"


def test_seeded_random_cases(kats):
    """30 cases of N = 5 .. 60 and S = 2 .. N with a random assignment (a seed in its own cluster); half of the matrices are drawn from a
    few values only, so that ties are everywhere."""
    rng = np.random.default_rng(20261019)
    cases = []
    for c in range(30):
        n = int(rng.integers(5, 61))
        s = n if c == 0 else int(rng.integers(2, n + 1))
        seeds = G.seed_ids(n, s)
        seed_of = [int(x) for x in rng.integers(0, s, n)]
        for t, i in enumerate(seeds):
            seed_of[i] = t
        d = rng.choice([0.0, 0.125, 0.25, 0.3, 0.7, 1.0], size=(n, n)) if c % 2 else rng.random((n, n))
        d = np.triu(d, 1) + np.triu(d, 1).T
        cases.append((["s%d" % i for i in range(n)], s, seed_of, d))
    got = kats(cases)
    for case, (seeds, text) in zip(cases, got):
        want_seeds, want_text = _want(*case)
        assert seeds == want_seeds and text == want_text, (len(case[0]), case[1])
    # S = N: every cluster is one sequence, the text is the one-stage tree's
    assert got[0][1] == O.upgma_newick(cases[0][0], cases[0][3])
