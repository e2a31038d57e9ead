"""The command line of --iterations and --mask-gappy where it needs no device: everything it refuses, with the text, before a device is
opened; the checker's build of the same sources, which carries neither flag; and --iterations 1, which is today's run.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(*args, timeout=60):
    exe = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def _fasta(path, records):
    path.write_text("".join(">%s\n%s\n" % r for r in records))
    return str(path)


def _refused(r, *words):
    assert r.returncode == 1, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "twl_init" not in r.stderr and "usage:" not in r.stderr, r.stderr


def test_usage_names_the_new_form(built):
    r = _cli()
    assert r.returncode == 1 and "--iterations K [--mask-gappy 0.95]" in r.stderr
    assert "usage: twilight-mi355x -t <tree.nwk> -i <sequences.fa[.gz]> -o <out.aln>" in r.stderr and "[--write-tree <tree.nwk>] [--tree-seeds S]" in r.stderr


@pytest.mark.parametrize("value", ["0", "6", "-1", "two", "2x", "", "1.5"])
def test_refuses_a_count_that_is_not_1_to_5(built, tmp_path, value):
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", value)
    _refused(r, "--iterations needs a number of runs from 1 to 5", "(got %s)" % value)


@pytest.mark.parametrize("value", ["0", "-0.5", "1.0001", "2", "abc", "0.5x", "nan", ""])
def test_refuses_a_mask_outside_0_1(built, tmp_path, value):
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", "2", "--mask-gappy", value)
    _refused(r, "--mask-gappy needs a value in (0, 1]", "(got %s)" % value)


def test_refuses_a_mask_without_iterations(built, tmp_path):
    for extra in ((), ("--iterations", "1")):
        r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--mask-gappy", "0.9", *extra)
        _refused(r, "--mask-gappy applies to the trees that --iterations 2 or more rebuilds")


@pytest.mark.parametrize("extra", [("-a", "x.aln"), ("-f", "dir"), ("-m", "50"), ("-t", "x.nwk", "-m", "50"), ("-t", "x.nwk", "-a", "x.aln")])
def test_refuses_the_other_modes(built, tmp_path, extra):
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", "2", *extra)
    _refused(r, "--iterations cannot be combined with -a, -f or -m")


def test_refuses_filter_and_host_staged(built, tmp_path):
    for tree in ((), ("-t", "x.nwk")):
        r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", "3", "--filter", *tree)
        _refused(r, "--iterations cannot be combined with --filter", "would lack the excluded sequences")
        r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", "3", "--host-staged", *tree)
        _refused(r, "--host-staged is not available with --iterations")


def test_refuses_several_gpus_at_parse_time(built, tmp_path):
    """Before any file is opened: none of them exists."""
    for tree in ((), ("-t", str(tmp_path / "none.nwk"))):
        for extra in (("--gpu-index", "0,1"), ("-G", "2")):
            r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", "2", *tree, *extra)
            _refused(r, "--iterations runs on one GPU")
            assert "open" not in r.stderr


def test_write_tree_stays_refused_with_a_tree(built, tmp_path):
    r = _cli("-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--iterations", "2", "--write-tree", str(tmp_path / "t.nwk"))
    _refused(r, "--write-tree cannot be combined with -t")


@pytest.mark.parametrize("tree", [False, True])
def test_refuses_what_the_records_rule_out(built, tmp_path, tree):
    """Fewer than 2 sequences, more than 16384, a name no tree can hold: after one pass over the records, before the tree is read (it does
    not exist) and before a device is opened."""
    t = ("-t", str(tmp_path / "none.nwk")) if tree else ()
    out = str(tmp_path / "o.aln")
    one = _fasta(tmp_path / "one.fa", [("a", "ACGTACGTAC"), ("a", "ACGTACGTAA")])      # a duplicate name keeps its first record: one sequence
    _refused(_cli("-i", one, "-o", out, "--iterations", "2", *t), "at least 2 sequences", "holds 1")
    many = _fasta(tmp_path / "many.fa", [("s%d" % i, "ACGTACGT") for i in range(16385)])
    _refused(_cli("-i", many, "-o", out, "--iterations", "2", "--type", "n", *t), "16385 sequences", "at most 16384")
    if not tree:
        _refused(_cli("-i", many, "-o", out, "--iterations", "2", "--type", "n", "--tree-seeds", "256"), "16385 sequences", "at most 16384", "--tree-seeds")
    for name, words in (("a(b", ("cannot be written into a Newick tree",)), ("node_7", ('begins with "node"',)), ("", ("without a name",))):
        fa = _fasta(tmp_path / "s.fa", [("ok", "ACGTACGTAC"), (name, "ACGTACGTAA"), ("fine", "ACGTACGTCC")])
        _refused(_cli("-i", fa, "-o", out, "--iterations", "2", "--type", "n", *t), *words)
    assert not os.path.exists(out)


def test_checker_binary_knows_neither_flag(built, tmp_path):
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    for flag, value in (("--iterations", "2"), ("--iterations", "1"), ("--mask-gappy", "0.9")):
        r = subprocess.run([exe, "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), flag, value], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "unsupported option %s" % flag in r.stderr


@pytest.mark.parametrize("args", [("-t", "none.nwk", "-i", "none.fa", "-o", "o.aln"), ("-a", "x.aln", "-t", "x.nwk", "-i", "x.fa", "-o", "o.aln"), ("-i", "none.fa"),
                                  ("-f", "no_such_dir", "-o", "o.aln"), ("-a", "none.aln", "-i", "none.fa", "-o", "o.aln"),
                                  ("-t", "none.nwk", "-i", "none.fa", "-o", "o.aln", "-m", "50"), ("-i", "none.fa", "-o", "o.aln", "--gpu-index", "0,1"),
                                  ("-t", "x.nwk", "-i", "x.fa", "-o", "o.aln", "--write-tree", "t.nwk")])
def test_iterations_1_is_todays_run(built, tmp_path, args):
    """--iterations 1 parses wherever the run parses without it and changes nothing: the same exit code and the same messages, in every mode
    (none of the files exists, so every run ends where it opens its first file, or in its own refusal)."""
    a = subprocess.run([os.path.join(ROOT, "twilight_amd", "twilight-mi355x"), *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    b = subprocess.run([os.path.join(ROOT, "twilight_amd", "twilight-mi355x"), *args, "--iterations", "1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert a.returncode == b.returncode != 0 and a.stderr == b.stderr and a.stdout == b.stdout
    assert "--iterations" not in b.stderr or "usage:" in b.stderr
