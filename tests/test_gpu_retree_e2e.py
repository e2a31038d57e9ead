"""--iterations on the MI355X, through the command line: the tree that run 2 is built on (--write-tree) is the tree of the numpy restatement
(tests/retree_oracle.py) of run 1's alignment, byte for byte, and -t on the written tree repeats the run byte for byte.  Every CLI run has
its own time limit."""
import hashlib
import os
import re
import subprocess

import pytest

import guide_oracle as O
import retree_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu


def _cli(*args, timeout=120):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def _ok(*args):
    r = _cli(*args)
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
    return names, seqs, "n"


def _rnasim200():
    names, seqs = O.read_fasta(os.path.join(GOLDEN, "RNASim.fa.gz"), limit=200)
    assert len(names) == 200
    return names, seqs, "n"


def _protein():
    from twilight_amd import synth

    _, leaves = synth.make_family(40, 300, P=22, seed=20261019)
    return [n for n, _ in leaves], [s.encode() for _, s in leaves], "p"


FAMILIES = {"sars_20": _sars, "rnasim_200": _rnasim200, "protein_40x300": _protein}
_CACHE = {}


def _aligned(path, names, seqs):
    """The rows of an alignment file in input order, after checking that it is one: one width, every row degapped is its input."""
    got_names, rows = O.read_fasta(path)
    assert got_names == names
    assert len({len(r) for r in rows}) == 1
    for n, s, r in zip(names, seqs, rows):
        assert r.replace(b"-", b"") == s, n
    return rows


def _family(name, tmp_path_factory):
    """(directory, fasta path, names, sequences, type, the rows of run (a): --iterations 1): made once per family and shared."""
    if name not in _CACHE:
        d = tmp_path_factory.mktemp("retree_" + name)
        names, seqs, type_ = FAMILIES[name]()
        fa = str(d / "s.fa")
        _write(fa, names, seqs)
        a1 = str(d / "a1.aln")
        _ok("-i", fa, "-o", a1, "--iterations", "1", "--type", type_)
        _CACHE[name] = (d, fa, names, seqs, type_, _aligned(a1, names, seqs))
    return _CACHE[name]


def _kept(stderr, iteration):
    m = re.search(r"Guide tree rebuilt from the alignment of iteration %d: kept (\d+) of (\d+) columns" % iteration, stderr)
    assert m, stderr[-2000:]
    return int(m.group(1)), int(m.group(2))


def _two_iterations(tmp_path, fa, names, seqs, type_, rows1, T=None):
    a2, b2, t2 = str(tmp_path / "a2.aln"), str(tmp_path / "b2.aln"), str(tmp_path / "t2.nwk")
    mask = () if T is None else ("--mask-gappy", str(T))
    T = 0.95 if T is None else T
    r = _ok("-i", fa, "-o", a2, "--iterations", "2", "--write-tree", t2, "--type", type_, "-v", *mask)
    want = R.tree_of(names, rows1, type_, T)
    got = open(t2).read()
    assert got == want, (got[:300], want[:300])
    want_kept = int(R.kept_columns(rows1, R.max_gaps(T, len(rows1))).sum())
    assert _kept(r.stderr, 1) == (want_kept, len(rows1[0]))
    _ok("-t", t2, "-i", fa, "-o", b2, "--type", type_)
    assert _md5(a2) == _md5(b2)
    return _aligned(a2, names, seqs), want_kept


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_second_tree_is_the_oracles_and_reproduces_the_run(gpu, tmp_path, tmp_path_factory, name):
    _, fa, names, seqs, type_, rows1 = _family(name, tmp_path_factory)
    _two_iterations(tmp_path, fa, names, seqs, type_, rows1)


def test_one_iteration_is_the_run_without_the_flag(gpu, tmp_path, tmp_path_factory):
    d, fa, names, seqs, type_, _ = _family("protein_40x300", tmp_path_factory)
    plain, t0, t1 = str(tmp_path / "plain.aln"), str(tmp_path / "t0.nwk"), str(tmp_path / "t1.nwk")
    _ok("-i", fa, "-o", plain, "--type", type_, "--write-tree", t0)
    assert _md5(plain) == _md5(str(d / "a1.aln"))
    _ok("-i", fa, "-o", plain, "--type", type_, "--write-tree", t1, "--iterations", "1")
    assert open(t0).read() == open(t1).read() == O.tree_of(names, seqs, type_)


def test_the_first_tree_may_be_the_two_stage_tree(gpu, tmp_path, tmp_path_factory):
    """--tree-seeds 20 with --iterations 2 on the 200 RNASim records: the first tree is the two-stage one, the second the restatement's tree of
    the alignment that tree gave."""
    _, fa, names, seqs, type_, _ = _family("rnasim_200", tmp_path_factory)
    s1, s2, b2, t2 = str(tmp_path / "s1.aln"), str(tmp_path / "s2.aln"), str(tmp_path / "b2.aln"), str(tmp_path / "t2.nwk")
    _ok("-i", fa, "-o", s1, "--tree-seeds", "20", "--type", type_)
    _ok("-i", fa, "-o", s2, "--tree-seeds", "20", "--iterations", "2", "--write-tree", t2, "--type", type_)
    assert open(t2).read() == R.tree_of(names, _aligned(s1, names, seqs), type_)
    _ok("-t", t2, "-i", fa, "-o", b2, "--type", type_)
    assert _md5(s2) == _md5(b2)


def test_a_stricter_mask(gpu, tmp_path, tmp_path_factory):
    """--mask-gappy 0.5 on the 200 RNASim records: fewer columns are kept than by default, and the tree is the restatement's for that mask."""
    _, fa, names, seqs, type_, rows1 = _family("rnasim_200", tmp_path_factory)
    _, kept = _two_iterations(tmp_path, fa, names, seqs, type_, rows1, T=0.5)
    assert kept < int(R.kept_columns(rows1, R.max_gaps(0.95, len(rows1))).sum())


def test_three_iterations_chain_one_step_further(gpu, tmp_path, tmp_path_factory):
    """sars_20: the tree of run 3 is the restatement's tree of run 2's alignment."""
    _, fa, names, seqs, type_, rows1 = _family("sars_20", tmp_path_factory)
    a2, a3, b3, t3 = str(tmp_path / "a2.aln"), str(tmp_path / "a3.aln"), str(tmp_path / "b3.aln"), str(tmp_path / "t3.nwk")
    _ok("-i", fa, "-o", a2, "--iterations", "2", "--type", type_)
    rows2 = _aligned(a2, names, seqs)
    r = _ok("-i", fa, "-o", a3, "--iterations", "3", "--write-tree", t3, "--type", type_, "-v")
    assert open(t3).read() == R.tree_of(names, rows2, type_)
    assert _kept(r.stderr, 1)[1] == len(rows1[0]) and _kept(r.stderr, 2)[1] == len(rows2[0])
    _ok("-t", t3, "-i", fa, "-o", b3, "--type", type_)
    assert _md5(a3) == _md5(b3)
    _aligned(a3, names, seqs)


def test_iterations_from_a_given_tree(gpu, tmp_path, tmp_path_factory):
    """sars_20 with -t: run 2 is -t on the restatement's tree of the plain -t run."""
    _, fa, names, seqs, type_, _ = _family("sars_20", tmp_path_factory)
    nwk = os.path.join(GOLDEN, "sars_20.nwk")
    c1, c2, d2, t = str(tmp_path / "c1.aln"), str(tmp_path / "c2.aln"), str(tmp_path / "d2.aln"), str(tmp_path / "t.nwk")
    _ok("-t", nwk, "-i", fa, "-o", c1, "--type", type_)
    with open(t, "w") as f:
        f.write(R.tree_of(names, _aligned(c1, names, seqs), type_))
    _ok("-t", nwk, "-i", fa, "-o", c2, "--iterations", "2", "--type", type_)
    _ok("-t", t, "-i", fa, "-o", d2, "--type", type_)
    assert _md5(c2) == _md5(d2)
    _aligned(c2, names, seqs)
