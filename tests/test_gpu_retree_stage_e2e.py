"""`--iterations K --retree-seeds S` on the MI355X, through the command line: the tree that run 2 is built on (--write-tree) is the two-stage
tree of the restatement (tests/retree_stage_oracle.py) of run 1's alignment, byte for byte; -t on the written tree repeats the run; as many
seeds as sequences give the run without the flag; and a family above the one-stage cap of 16 384 sequences runs to its end.  Every CLI run
has its own time limit."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import guide_oracle as O
import retree_oracle as R
import retree_stage_oracle as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu


def _cli(*args, timeout=120):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def _ok(*args, timeout=120):
    r = _cli(*args, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def _write(path, names, seqs):
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n" + s + b"\n")


def _sars():
    names, seqs = O.read_fasta(os.path.join(GOLDEN, "sars_20.fa.gz"))
    return names, seqs, "n", 4


def _rnasim200():
    names, seqs = O.read_fasta(os.path.join(GOLDEN, "RNASim.fa.gz"), limit=200)
    assert len(names) == 200
    return names, seqs, "n", 8


def _protein():
    from twilight_amd import synth

    _, leaves = synth.make_family(40, 300, P=22, seed=20261019)
    return [n for n, _ in leaves], [s.encode() for _, s in leaves], "p", 5


LARGE_N = 16400


def _large():
    """16 400 sequences of 48-64 nt: 64 unrelated founders, every sequence a founder with a tenth of its letters redrawn, cut to its length."""
    rng = np.random.default_rng(20261019)
    letters = np.array(list(b"ACGT"), dtype=np.uint8)
    founders = rng.choice(letters, (64, 64))
    which = rng.integers(0, 64, LARGE_N)
    seqs = []
    for i in range(LARGE_N):
        s = founders[which[i]].copy()
        hit = rng.random(64) < 0.1
        s[hit] = rng.choice(letters, int(hit.sum()))
        seqs.append(s[: int(rng.integers(48, 65))].tobytes())
    return ["x%d" % i for i in range(LARGE_N)], seqs, "n", 256


FAMILIES = {"sars_20": _sars, "rnasim_200": _rnasim200, "protein_40x300": _protein, "large": _large}
_CACHE = {}


def _aligned(path, names, seqs):
    """The rows of an alignment file in input order, after checking that it is one: one width, every row degapped is its input."""
    got_names, rows = O.read_fasta(path)
    assert got_names == names
    assert len({len(r) for r in rows}) == 1
    for n, s, r in zip(names, seqs, rows):
        assert r.replace(b"-", b"") == s, n
    return rows


def _family(name, tmp_path_factory, first=()):
    """(fasta path, names, sequences, type, seeds, the rows of run 1): made once per family and shared.  `first` are the flags that choose the
    first tree; run 1 is the run with them and --iterations 1."""
    if name not in _CACHE:
        d = tmp_path_factory.mktemp("retree_stage_" + name)
        names, seqs, type_, s = FAMILIES[name]()
        fa = str(d / "s.fa")
        _write(fa, names, seqs)
        a1 = str(d / "a1.aln")
        _ok("-i", fa, "-o", a1, "--iterations", "1", "--type", type_, *first, timeout=300)
        _CACHE[name] = (fa, names, seqs, type_, s, _aligned(a1, names, seqs))
    return _CACHE[name]


def _leaves(text):
    return re.findall(r"[(,]([^(),:;]+):", text)


def _line(stderr, iteration):
    m = re.search(r"Guide tree rebuilt in two stages from the alignment of iteration %d: kept (\d+) of (\d+) columns, (\d+) sequences, (\d+) seeds \(ms\): upload [\d.e+-]+, gaps [\d.e+-]+, "
                  r"pack [\d.e+-]+, assign [\d.e+-]+, groups [\d.e+-]+, download [\d.e+-]+, UPGMA [\d.e+-]+, text [\d.e+-]+; clusters: smallest (\d+), median (\d+), largest (\d+)" % iteration, stderr)
    assert m, stderr[-2000:]
    return [int(x) for x in m.groups()]


def _two_iterations(tmp_path, fa, names, seqs, type_, s, rows1, T=None, first=(), timeout=120):
    a2, b2, t2 = str(tmp_path / "a2.aln"), str(tmp_path / "b2.aln"), str(tmp_path / "t2.nwk")
    mask = () if T is None else ("--mask-gappy", str(T))
    T = 0.95 if T is None else T
    r = _ok("-i", fa, "-o", a2, "--iterations", "2", "--retree-seeds", str(s), "--write-tree", t2, "--type", type_, "-v", *mask, *first, timeout=timeout)
    want, k = RS.tree_of(names, rows1, type_, s, T)
    got = open(t2).read()
    assert got == want, (got[:300], want[:300])
    sizes = sorted(len(x) for x in k)
    want_kept = int(R.kept_columns(rows1, R.max_gaps(T, len(rows1))).sum())
    assert _line(r.stderr, 1) == [want_kept, len(rows1[0]), len(names), s, sizes[0], sizes[len(sizes) // 2], sizes[-1]]
    _ok("-t", t2, "-i", fa, "-o", b2, "--type", type_, timeout=timeout)
    assert _md5(a2) == _md5(b2)
    _aligned(a2, names, seqs)
    return got, want_kept


@pytest.mark.parametrize("name", ["protein_40x300", "rnasim_200", "sars_20"])
def test_the_second_tree_is_the_oracles_and_reproduces_the_run(gpu, tmp_path, tmp_path_factory, name):
    fa, names, seqs, type_, s, rows1 = _family(name, tmp_path_factory)
    got, _ = _two_iterations(tmp_path, fa, names, seqs, type_, s, rows1)
    assert sorted(_leaves(got)) == sorted(names)


def test_as_many_seeds_as_sequences_is_the_run_without_the_flag(gpu, tmp_path, tmp_path_factory):
    fa, names, seqs, type_, _, rows1 = _family("rnasim_200", tmp_path_factory)
    a, b, ta, tb = str(tmp_path / "a.aln"), str(tmp_path / "b.aln"), str(tmp_path / "a.nwk"), str(tmp_path / "b.nwk")
    _ok("-i", fa, "-o", a, "--iterations", "2", "--retree-seeds", "200", "--write-tree", ta, "--type", type_)
    _ok("-i", fa, "-o", b, "--iterations", "2", "--write-tree", tb, "--type", type_)
    assert _md5(ta) == _md5(tb) and _md5(a) == _md5(b)
    assert open(ta).read() == R.tree_of(names, rows1, type_)


def test_three_iterations_chain_one_step_further(gpu, tmp_path, tmp_path_factory):
    """sars_20: the tree of run 3 is the restatement's two-stage tree of run 2's alignment."""
    fa, names, seqs, type_, s, rows1 = _family("sars_20", tmp_path_factory)
    a2, a3, b3, t3 = str(tmp_path / "a2.aln"), str(tmp_path / "a3.aln"), str(tmp_path / "b3.aln"), str(tmp_path / "t3.nwk")
    _ok("-i", fa, "-o", a2, "--iterations", "2", "--retree-seeds", str(s), "--type", type_)
    rows2 = _aligned(a2, names, seqs)
    r = _ok("-i", fa, "-o", a3, "--iterations", "3", "--retree-seeds", str(s), "--write-tree", t3, "--type", type_, "-v")
    assert open(t3).read() == RS.tree_of(names, rows2, type_, s)[0]
    assert _line(r.stderr, 1)[1] == len(rows1[0]) and _line(r.stderr, 2)[1] == len(rows2[0])
    _ok("-t", t3, "-i", fa, "-o", b3, "--type", type_)
    assert _md5(a3) == _md5(b3)
    _aligned(a3, names, seqs)


def test_a_stricter_mask(gpu, tmp_path, tmp_path_factory):
    """--mask-gappy 0.5 on the 200 RNASim records: fewer columns are kept than by default, and the tree is the restatement's for that mask."""
    fa, names, seqs, type_, s, rows1 = _family("rnasim_200", tmp_path_factory)
    _, kept = _two_iterations(tmp_path, fa, names, seqs, type_, s, rows1, T=0.5)
    assert kept < int(R.kept_columns(rows1, R.max_gaps(0.95, len(rows1))).sum())


def test_iterations_from_a_given_tree(gpu, tmp_path, tmp_path_factory):
    """sars_20 with -t: run 2 is -t on the restatement's two-stage tree of the plain -t run."""
    fa, names, seqs, type_, s, _ = _family("sars_20", tmp_path_factory)
    nwk = os.path.join(GOLDEN, "sars_20.nwk")
    c1, c2, d2, t = str(tmp_path / "c1.aln"), str(tmp_path / "c2.aln"), str(tmp_path / "d2.aln"), str(tmp_path / "t.nwk")
    _ok("-t", nwk, "-i", fa, "-o", c1, "--type", type_)
    with open(t, "w") as f:
        f.write(RS.tree_of(names, _aligned(c1, names, seqs), type_, s)[0])
    _ok("-t", nwk, "-i", fa, "-o", c2, "--iterations", "2", "--retree-seeds", str(s), "--type", type_)
    _ok("-t", t, "-i", fa, "-o", d2, "--type", type_)
    assert _md5(c2) == _md5(d2)
    _aligned(c2, names, seqs)


def test_a_family_above_the_one_stage_cap(gpu, tmp_path, tmp_path_factory):
    """16 400 sequences: --iterations 2 is refused without --retree-seeds; with --tree-seeds 256 --retree-seeds 256 it runs to its end, the
    second tree is the oracle's, every name is one leaf, every row degapped is its input, and -t on the written tree repeats the run."""
    first = ("--tree-seeds", "256")
    fa, names, seqs, type_, s, rows1 = _family("large", tmp_path_factory, first)
    r = _cli("-i", fa, "-o", str(tmp_path / "no.aln"), "--type", type_, "--iterations", "2", *first)
    assert r.returncode == 1 and "16400 sequences" in r.stderr and "at most 16384" in r.stderr and "--retree-seeds" in r.stderr
    assert not os.path.exists(str(tmp_path / "no.aln"))
    got, _ = _two_iterations(tmp_path, fa, names, seqs, type_, s, rows1, first=first, timeout=300)
    assert sorted(_leaves(got)) == sorted(names)
