"""A run without -t on the MI355X, through the command line: the tree it builds and writes (--write-tree) is the tree of the numpy restatement
(tests/guide_oracle.py) byte for byte, and -t on the written tree repeats the run byte for byte, -m included.  Every CLI run has its own
time limit."""
import gzip
import hashlib
import os
import subprocess

import pytest

import guide_oracle as O

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


def _sars(tmp):
    names, seqs = O.read_fasta(os.path.join(GOLDEN, "sars_20.fa.gz"))
    return names, seqs, "n"


def _rnasim200(tmp):
    names, seqs = O.read_fasta(os.path.join(GOLDEN, "RNASim.fa.gz"), limit=200)
    assert len(names) == 200
    return names, seqs, "n"


def _protein(tmp):
    from twilight_amd import synth

    _, leaves = synth.make_family(40, 300, P=22, seed=20261019)
    return [n for n, _ in leaves], [s.encode() for _, s in leaves], "p"


FAMILIES = {"sars_20": _sars, "rnasim_200": _rnasim200, "protein_40x300": _protein}
_CACHE = {}


def _family(name, tmp_path_factory):
    """(fasta path, names, sequences, type, the oracle's tree): made once per family and shared."""
    if name not in _CACHE:
        d = tmp_path_factory.mktemp("guide_" + name)
        names, seqs, type_ = FAMILIES[name](d)
        fa = str(d / "s.fa")
        _write(fa, names, seqs)
        _CACHE[name] = (fa, names, seqs, type_, O.tree_of(names, seqs, type_))
    return _CACHE[name]


def _rows(path):
    names, rows = O.read_fasta(path)
    return dict(zip(names, rows))


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_written_tree_is_the_oracles_and_reproduces_the_run(gpu, tmp_path, tmp_path_factory, name):
    fa, names, seqs, type_, want_tree = _family(name, tmp_path_factory)
    a, b, t = str(tmp_path / "a.aln"), str(tmp_path / "b.aln"), str(tmp_path / "t.nwk")
    r = _cli("-i", fa, "-o", a, "--write-tree", t, "--type", type_, "-v")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Guide tree of %d sequences (ms): upload + count" % len(names) in r.stderr
    got_tree = open(t).read()
    assert got_tree == want_tree, (got_tree[:300], want_tree[:300])
    r = _cli("-t", t, "-i", fa, "-o", b, "--type", type_)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _md5(a) == _md5(b)
    rows = _rows(a)
    assert set(rows) == set(names)
    assert len({len(v) for v in rows.values()}) == 1
    for n, s in zip(names, seqs):
        assert rows[n].replace(b"-", b"") == s, n


def test_subtrees_of_the_built_tree(gpu, tmp_path, tmp_path_factory):
    """-m 50 without -t against -t on the written tree with -m 50."""
    fa, names, seqs, type_, want_tree = _family("rnasim_200", tmp_path_factory)
    a, b, t = str(tmp_path / "a.aln"), str(tmp_path / "b.aln"), str(tmp_path / "t.nwk")
    r = _cli("-i", fa, "-o", a, "--write-tree", t, "-m", "50")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(t).read() == want_tree
    assert "subtrees" in r.stderr
    r = _cli("-t", t, "-i", fa, "-o", b, "-m", "50")
    assert r.returncode == 0, r.stderr[-2000:]
    assert _md5(a) == _md5(b)
    rows = _rows(a)
    assert len({len(v) for v in rows.values()}) == 1
    for n, s in zip(names, seqs):
        assert rows[n].replace(b"-", b"") == s, n
