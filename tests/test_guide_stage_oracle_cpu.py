"""The restatement of the two-stage guide tree (tests/guide_stage_oracle.py) against a tree worked by hand from DESIGN.md section 4g, against
the one-stage oracle where the two must agree, and on the corners of the assignment rule.  The cluster sizes of the golden families are
pinned here, so that the GPU tests on them are known to cover clusters of one member and of many.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import guide_oracle as O
import guide_stage_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# eight 6-mers; joined by N a sequence has exactly these windows, one each
A, B, C, D, E, F, GG, H = "AAAAAA", "CCCCCC", "GGGGGG", "TTTTTT", "ACACAC", "CACACA", "AGAGAG", "GAGAGA"


def _seq(*kmers):
    return "N".join(kmers).encode()


HAND = [_seq(A, B, C, D), _seq(A, B, C, E), _seq(A, B, F, GG), _seq(E, F, GG, H), _seq(E, F, GG, A), _seq(C, D)]
HAND_NAMES = ["s%d" % i for i in range(6)]
HAND_TREE = "((((s0:0.000000,s5:0.000000):0.187500,s1:0.187500):0.145833,s2:0.333333):0.166667,(s3:0.125000,s4:0.125000):0.375000);\n"


def _leaves(text):
    return re.findall(r"[(,]([^(),:;]+):", text)


def test_hand_derived_tree_of_six_sequences_and_two_seeds():
    """Seeds 0 and 3.  s1: 3/4 against 1/4 -> seed 0.  s2: 2/4 against 2/4, a tie -> seed 0.  s4: 1/4 against 3/4 -> seed 1.  s5 = {c, d}:
    2/2 against 0 -> seed 0.  K_0 = (0, 1, 2, 5), K_1 = (3, 4).
    U_1: d(3, 4) = 1/4 -> height 1/8.
    U_0: d(0, 5) = 0 first; then d(05, 1) = (1/4 + 1/2) / 2 = 3/8 -> 3/16; then d(051, 2) = (2 * 3/4 + 1/2) / 3 = 2/3 -> 1/3.
    V: S(0, 3) = 0, d = 1 -> 1/2; the grafted roots stand at 1/3 and 1/8."""
    counts = O.counts_matrix(HAND, "n")
    assert [int(x) for x in counts.sum(axis=1)] == [4, 4, 4, 4, 4, 2]
    assert G.seed_ids(6, 2) == [0, 3]
    seed_of, shared = G.assign(counts, [0, 3])
    assert seed_of == [0, 0, 0, 1, 1, 0] and shared == [4, 3, 2, 4, 3, 2]
    assert G.tree_of(HAND_NAMES, HAND, "n", 2) == HAND_TREE


def test_as_many_seeds_as_sequences_is_the_one_stage_tree():
    rng = np.random.default_rng(7)
    anc = rng.choice(list(b"ACGT"), 200)
    seqs = []
    for i in range(23):
        s = anc.copy()
        hit = rng.random(200) < 0.03 * (1 + i % 5)
        s[hit] = rng.choice(list(b"ACGT"), int(hit.sum()))
        seqs.append(bytes(s.tolist()))
    names = ["q%d" % i for i in range(23)]
    assert G.tree_of(names, seqs, "n", 23) == O.tree_of(names, seqs, "n")
    names, seqs = O.read_fasta(os.path.join(GOLDEN, "sars_20.fa.gz"))
    assert G.tree_of(names, seqs, "n", len(names)) == O.tree_of(names, seqs, "n")


def test_two_identical_seeds():
    """Sequences 0, 3 and 5 are one text; the seeds of N = 6, S = 2 are 0 and 3.  Seed 3 keeps itself although seed 0 is as close and earlier;
    sequence 5 is no seed and goes to the earlier of the two."""
    rng = np.random.default_rng(11)
    same = bytes(rng.choice(list(b"ACGT"), 120).tolist())
    other = [bytes(rng.choice(list(b"ACGT"), 120).tolist()) for _ in range(3)]
    seqs = [same, other[0], other[1], same, other[2], same]
    counts = O.counts_matrix(seqs, "n")
    seed_of, shared = G.assign(counts, G.seed_ids(6, 2))
    assert seed_of[0] == 0 and seed_of[3] == 1 and seed_of[5] == 0
    assert shared[0] == shared[3] == shared[5] == 115


def test_a_sequence_without_windows_lands_on_seed_0():
    rng = np.random.default_rng(13)
    seqs = [bytes(rng.choice(list(b"ACGT"), 80).tolist()) for _ in range(9)]
    seqs[4] = b"ACGTA"      # shorter than k: w = 0
    seqs[7] = b""
    counts = O.counts_matrix(seqs, "n")
    seed_of, shared = G.assign(counts, G.seed_ids(9, 3))
    assert seed_of[4] == 0 and seed_of[7] == 0 and shared[4] == 0 and shared[7] == 0
    # ... and a seed without windows attracts nobody but itself, unless everything else is at ratio 0 too and it is the earliest
    seqs[3] = b"AC"
    counts = O.counts_matrix(seqs, "n")
    seed_of, _ = G.assign(counts, [3, 0, 6])
    assert seed_of[3] == 0 and seed_of[4] == 0 and seed_of[7] == 0      # 4 and 7 tie at 0 / 1 with every seed: the smallest t
    assert all(seed_of[i] != 0 for i in (0, 6))


def test_the_walk_over_the_candidates_is_the_total_order():
    """best_seed against every pair compared with `better` in Python integers, on ratios with many ties."""
    rng = np.random.default_rng(17)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        m = rng.integers(0, 7, n).astype(np.int64)
        s = np.minimum(rng.integers(0, 7, n), m).astype(np.int64)
        best = G.best_seed(s, m)
        cand = [(int(s[t]), int(m[t])) if m[t] > 0 else (0, 1) for t in range(n)]
        assert all(G.better(*cand[best], best, *cand[t], t) for t in range(n) if t != best)
    big = np.array([2 ** 29 - 1, 2 ** 29 - 2, 2 ** 29 - 1], dtype=np.int64)      # the largest products: no wrap
    assert G.best_seed(big, np.array([2 ** 29 - 1] * 3, dtype=np.int64)) == 0


@pytest.fixture(scope="module")
def rnasim200():
    names, seqs = O.read_fasta(os.path.join(GOLDEN, "RNASim.fa.gz"), limit=200)
    return names, seqs, O.counts_matrix(seqs, "n")


def test_every_name_is_one_leaf(rnasim200):
    names, seqs, counts = rnasim200
    text, k = G.tree_from_counts(names, counts, 8)
    assert sorted(_leaves(text)) == sorted(names)
    assert sorted(i for members in k for i in members) == list(range(200))
    assert text.count("(") == text.count(")") == 199 and text.endswith(";\n")


def test_cluster_sizes_of_the_golden_families(rnasim200):
    names, seqs, counts = rnasim200
    k8 = [len(x) for x in G.clusters(8, G.assign(counts, G.seed_ids(200, 8))[0])]
    assert min(k8) == 10 and max(k8) == 51 and sum(k8) == 200, k8
    k3 = [len(x) for x in G.clusters(3, G.assign(counts, G.seed_ids(200, 3))[0])]
    assert sorted(k3) == [49, 56, 95], k3
    names, seqs = O.read_fasta(os.path.join(GOLDEN, "sars_20.fa.gz"))
    assert G.cluster_sizes(seqs, "n", 4) == [16, 1, 1, 2]
