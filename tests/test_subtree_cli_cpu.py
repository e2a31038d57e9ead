"""The command line of the subtree mode (-m / --max-subtree) where it needs no device: what it refuses at parse time, and the checker's build of
the same main.cpp, which carries no subtree mode.  These tests fail on a build that does not know -m.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _cli(*args, timeout=60):
    exe = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def test_cli_refuses_a_subtree_size_below_one(built, tmp_path):
    for bad in ("0", "-3", "x", "2.5"):
        r = _cli("-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "-m", bad)
        assert r.returncode == 1 and "--max-subtree needs a number of leaves >= 1" in r.stderr, (bad, r.stderr)
        assert "unsupported option" not in r.stderr


def test_cli_refuses_subtrees_with_merge_or_placement(built, tmp_path):
    r = _cli("-f", str(tmp_path), "-o", str(tmp_path / "o.aln"), "-m", "5")
    assert r.returncode == 1 and "-m (alignment in subtrees) cannot be combined with -a or -f" in r.stderr
    r = _cli("-a", "x.aln", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--max-subtree", "5")
    assert r.returncode == 1 and "-m (alignment in subtrees) cannot be combined with -a or -f" in r.stderr


def test_cli_refuses_several_gpus_and_host_staged_at_parse_time(built, tmp_path):
    """Before any device is opened and before the processes of a sharded run are forked: the tree file does not even exist."""
    r = _cli("-t", str(tmp_path / "none.nwk"), "-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "-m", "2", "--gpu-index", "0,1", "--type", "n")
    assert r.returncode == 1 and "one GPU" in r.stderr and "twl_init" not in r.stderr and "Failed to open" not in r.stderr
    r = _cli("-t", str(tmp_path / "none.nwk"), "-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "-m", "2", "--host-staged", "--type", "n")
    assert r.returncode == 1 and "--host-staged is not available with -m" in r.stderr


def test_cli_usage_names_the_mode(built):
    r = _cli()
    assert r.returncode == 1 and "-m <max. leaves per subtree>" in r.stderr


def test_cli_refuses_a_tree_that_cannot_be_cut(built, tmp_path):
    """A star at -m below its size: the best cut is the root, the partition records nothing; the run ends before a device is opened."""
    (tmp_path / "t.nwk").write_text("(a,b,c,d,e);\n")
    (tmp_path / "s.fa").write_text("".join(f">{n}\nACGTACGT\n" for n in "abcde"))
    r = _cli("-t", str(tmp_path / "t.nwk"), "-i", str(tmp_path / "s.fa"), "-o", str(tmp_path / "o.aln"), "-m", "3")
    assert r.returncode == 1 and "cannot be cut into subtrees of at most 3 leaves" in r.stderr and "twl_init" not in r.stderr


def test_cli_refuses_a_subtree_of_one_leaf(built, tmp_path):
    (tmp_path / "t.nwk").write_text("((((((a,b),c),d),e),f),g);\n")
    (tmp_path / "s.fa").write_text("".join(f">{n}\nACGTACGT\n" for n in "abcdefg"))
    r = _cli("-t", str(tmp_path / "t.nwk"), "-i", str(tmp_path / "s.fa"), "-o", str(tmp_path / "o.aln"), "-m", "2")
    assert r.returncode == 1 and "leaves subtree 1 with 1 leaf" in r.stderr and "twl_init" not in r.stderr


def test_checker_binaries_keep_refusing_m(built):
    """The CPU-check build of the same main.cpp carries no subtree mode: -m stays an unsupported option there."""
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = subprocess.run([exe, "-m", "5", "-t", os.path.join(GOLDEN, "sars_20.nwk"), "-i", "x.fa", "-o", "o.aln"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option -m" in r.stderr
