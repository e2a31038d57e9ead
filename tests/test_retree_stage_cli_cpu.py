"""The command line of `--retree-seeds S` (the guide tree rebuilt in two stages) where it needs no device: what it refuses, at parse time or
after reading the records, the cap that it lifts, the usage text, and the checker's build of the same main.cpp, which carries no such option.
These tests fail on a build that does not know the option.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(*args, timeout=60):
    exe = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def _refused(r, *words):
    assert r.returncode == 1, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "twl_init" not in r.stderr and "usage:" not in r.stderr and "unsupported option" not in r.stderr, r.stderr


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    fa = tmp_path_factory.mktemp("retree_stage_cli") / "many.fa"
    fa.write_text("".join(">s%d\nACGTACGT\n" % i for i in range(16385)))
    return str(fa)


def test_usage_names_the_flag(built):
    r = _cli()
    assert r.returncode == 1 and "--iterations K [--mask-gappy 0.95] [--retree-seeds S]" in r.stderr
    assert "[--write-tree <tree.nwk>] [--tree-seeds S]" in r.stderr
    assert "--retree-seeds S computes those trees in two stages" in r.stderr


@pytest.mark.parametrize("value", ["1", "0", "x", "16385", "-4", "12x", "", "2.5"])
def test_refuses_a_bad_number_of_seeds_at_parse_time(built, tmp_path, value):
    """Before the file is even opened: it does not exist."""
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", "2", "--retree-seeds", value)
    _refused(r, "--retree-seeds needs a number of seeds from 2 to 16384", "(got %s)" % value)
    assert "open" not in r.stderr


def test_refuses_a_missing_value(built, tmp_path):
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", "2", "--retree-seeds")
    assert r.returncode == 1 and "missing value for --retree-seeds" in r.stderr


@pytest.mark.parametrize("tree", [False, True])
def test_refused_without_two_iterations(built, tmp_path, tree):
    t = ("-t", str(tmp_path / "none.nwk")) if tree else ()
    for extra in ((), ("--iterations", "1")):
        r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--retree-seeds", "8", *t, *extra)
        _refused(r, "--retree-seeds applies to the trees that --iterations 2 or more rebuilds")
        assert "open" not in r.stderr


@pytest.mark.parametrize("extra,words", [(("-m", "50"), "--iterations cannot be combined with -a, -f or -m"), (("-a", "x.aln"), "--iterations cannot be combined with -a, -f or -m"),
                                         (("-f", "dir"), "--iterations cannot be combined with -a, -f or -m"), (("--filter",), "--iterations cannot be combined with --filter"),
                                         (("--host-staged",), "--host-staged is not available with --iterations"), (("--gpu-index", "0,1"), "--iterations runs on one GPU")])
def test_the_rules_of_iterations_stay(built, tmp_path, extra, words):
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--iterations", "2", "--retree-seeds", "8", *extra)
    _refused(r, words)


@pytest.mark.parametrize("tree", [False, True])
def test_refuses_more_seeds_than_sequences_after_reading(built, tmp_path, tree):
    """After the one pass over the records, before the tree is read (it does not exist) and before a device is opened."""
    fa = tmp_path / "s.fa"
    fa.write_text("".join(">s%d\nACGTACGTAC\n" % i for i in range(5)) + ">s0\nACGTACGTAA\n")      # the second s0 is dropped: 5 sequences
    t = ("-t", str(tmp_path / "none.nwk")) if tree else ()
    r = _cli("-i", str(fa), "-o", str(tmp_path / "o.aln"), "--type", "n", "--iterations", "2", "--retree-seeds", "6", *t)
    _refused(r, "--retree-seeds 6 is more than the 5 sequences")
    assert "none.nwk" not in r.stderr and not (tmp_path / "o.aln").exists()


def test_the_name_checks_come_first(built, tmp_path):
    fa = tmp_path / "s.fa"
    fa.write_text(">ok\nACGTACGTAC\n>a(b\nACGTACGTAA\n>fine\nACGTACGTCC\n")
    r = _cli("-i", str(fa), "-o", str(tmp_path / "o.aln"), "--type", "n", "--iterations", "2", "--retree-seeds", "4")
    _refused(r, "cannot be written into a Newick tree")


def test_the_one_stage_refusal_points_at_the_flag(built, tmp_path, many):
    """Its words stay (tests/test_retree_cli_cpu.py); a line is appended."""
    for extra in ((), ("--tree-seeds", "256")):
        r = _cli("-i", many, "-o", str(tmp_path / "o.aln"), "--type", "n", "--iterations", "2", *extra)
        _refused(r, "16385 sequences", "at most 16384", "--tree-seeds", "--retree-seeds S")


def test_the_flag_lifts_the_cap(built, tmp_path, many):
    """16 385 sequences with the flag and -t on a file that does not exist: the run gets past the cap and ends where it opens the tree."""
    missing = str(tmp_path / "none.nwk")
    r = _cli("-t", missing, "-i", many, "-o", str(tmp_path / "o.aln"), "--type", "n", "--iterations", "2", "--retree-seeds", "256")
    assert r.returncode != 0
    assert "at most 16384" not in r.stderr and "16385 sequences" not in r.stderr and "--retree-seeds" not in r.stderr, r.stderr
    assert missing in r.stderr, r.stderr
    assert not (tmp_path / "o.aln").exists()


def test_without_a_tree_the_first_tree_needs_its_own_flag(built, tmp_path, many):
    """No -t above 16 384 sequences: the first tree is the k-mer tree, whose own refusal names --tree-seeds."""
    r = _cli("-i", many, "-o", str(tmp_path / "o.aln"), "--type", "n", "--iterations", "2", "--retree-seeds", "256")
    _refused(r, "16385 sequences", "a guide tree is built for at most 16384", "--tree-seeds S")


def test_checker_binary_rejects_the_option(built, tmp_path):
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = subprocess.run([exe, "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--iterations", "2", "--retree-seeds", "8"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and ("unsupported option --iterations" in r.stderr or "unsupported option --retree-seeds" in r.stderr)
    r = subprocess.run([exe, "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--retree-seeds", "8"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option --retree-seeds" in r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--retree-seeds" not in r.stderr
