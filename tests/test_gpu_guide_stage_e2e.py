"""A run with `--tree-seeds S` on the MI355X, through the command line: the tree it builds and writes is the tree of the restatement
(tests/guide_stage_oracle.py) byte for byte, as many seeds as sequences give the run without the flag, -t on the written tree repeats the
run, -m composes, and a family above the one-stage cap of 16 384 sequences runs to its end.  Every CLI run has its own time limit."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import guide_oracle as O
import guide_stage_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu


def _cli(*args, timeout=120):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


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


LARGE_N = 16400
FAMILIES = {"sars_20": _sars, "rnasim_200": _rnasim200, "protein_40x300": _protein, "large": _large}
_CACHE = {}


def _family(name, tmp_path_factory):
    """(fasta path, names, sequences, type, seeds, the oracle's tree): made once per family and shared."""
    if name not in _CACHE:
        d = tmp_path_factory.mktemp("guide_stage_" + name)
        names, seqs, type_, s = FAMILIES[name]()
        fa = str(d / "s.fa")
        _write(fa, names, seqs)
        text, k = G.tree_from_counts(names, O.counts_matrix(seqs, type_), s)
        assert max(len(x) for x in k) <= 16384
        _CACHE[name] = (fa, names, seqs, type_, s, text)
    return _CACHE[name]


def _rows(path):
    names, rows = O.read_fasta(path)
    return dict(zip(names, rows))


def _leaves(text):
    return re.findall(r"[(,]([^(),:;]+):", text)


def _check_rows(path, names, seqs):
    rows = _rows(path)
    assert set(rows) == set(names) and len(rows) == len(names)
    assert len({len(v) for v in rows.values()}) == 1
    for n, s in zip(names, seqs):
        assert rows[n].replace(b"-", b"") == s, n


@pytest.mark.parametrize("name", ["protein_40x300", "rnasim_200", "sars_20"])
def test_the_written_tree_is_the_oracles_and_reproduces_the_run(gpu, tmp_path, tmp_path_factory, name):
    fa, names, seqs, type_, s, want_tree = _family(name, tmp_path_factory)
    a, b, t = str(tmp_path / "a.aln"), str(tmp_path / "b.aln"), str(tmp_path / "t.nwk")
    r = _cli("-i", fa, "-o", a, "--write-tree", t, "--tree-seeds", str(s), "--type", type_, "-v")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Guide tree of %d sequences in two stages, %d seeds (ms): upload + count" % (len(names), s) in r.stderr
    assert re.search(r"clusters: smallest \d+, median \d+, largest \d+", r.stderr)
    got_tree = open(t).read()
    assert got_tree == want_tree, (got_tree[:300], want_tree[:300])
    r = _cli("-t", t, "-i", fa, "-o", b, "--type", type_)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _md5(a) == _md5(b)
    _check_rows(a, names, seqs)


def test_as_many_seeds_as_sequences_is_the_run_without_the_flag(gpu, tmp_path, tmp_path_factory):
    fa, names, seqs, type_, _, _ = _family("rnasim_200", tmp_path_factory)
    a, b, ta, tb = str(tmp_path / "a.aln"), str(tmp_path / "b.aln"), str(tmp_path / "a.nwk"), str(tmp_path / "b.nwk")
    r = _cli("-i", fa, "-o", a, "--write-tree", ta, "--tree-seeds", "200")
    assert r.returncode == 0, r.stderr[-2000:]
    r = _cli("-i", fa, "-o", b, "--write-tree", tb)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _md5(ta) == _md5(tb) and _md5(a) == _md5(b)
    assert open(ta).read() == O.tree_of(names, seqs, type_)


def test_subtrees_of_the_two_stage_tree(gpu, tmp_path, tmp_path_factory):
    """-m 50 with --tree-seeds 8 against -t on the written tree with -m 50."""
    fa, names, seqs, type_, s, want_tree = _family("rnasim_200", tmp_path_factory)
    a, b, t = str(tmp_path / "a.aln"), str(tmp_path / "b.aln"), str(tmp_path / "t.nwk")
    r = _cli("-i", fa, "-o", a, "--write-tree", t, "--tree-seeds", str(s), "-m", "50")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(t).read() == want_tree
    assert "subtrees" in r.stderr
    r = _cli("-t", t, "-i", fa, "-o", b, "-m", "50")
    assert r.returncode == 0, r.stderr[-2000:]
    assert _md5(a) == _md5(b)
    _check_rows(a, names, seqs)


def test_a_family_above_the_one_stage_cap(gpu, tmp_path, tmp_path_factory):
    """16 400 sequences: refused without the flag, aligned with --tree-seeds 256; the tree is the oracle's, every name is one leaf, every row
    degapped is its input, and -t on the written tree repeats the run."""
    fa, names, seqs, type_, s, want_tree = _family("large", tmp_path_factory)
    a, b, t = str(tmp_path / "a.aln"), str(tmp_path / "b.aln"), str(tmp_path / "t.nwk")
    r = _cli("-i", fa, "-o", a, "--type", type_)
    assert r.returncode == 1 and "at most 16384" in r.stderr and "--tree-seeds" in r.stderr
    r = _cli("-i", fa, "-o", a, "--write-tree", t, "--tree-seeds", str(s), "--type", type_, "-v", timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got_tree = open(t).read()
    assert sorted(_leaves(got_tree)) == sorted(names)
    assert got_tree == want_tree, (got_tree[:300], want_tree[:300])
    _check_rows(a, names, seqs)
    r = _cli("-t", t, "-i", fa, "-o", b, "--type", type_, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _md5(a) == _md5(b)
