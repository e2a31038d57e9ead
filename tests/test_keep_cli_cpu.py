"""`--keep-length` and `--write-insertions` on the command line, before a file is read or a device opened: every refusal by exit code and
message; the CPU checker's build of the same parser knows neither flag; a placement without the flag is what it was.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")


def _cli(*args, env=None, exe=EXE):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, env=env)


# none of the named files exists: a refusal that came after a read would say so instead
REFUSALS = {
    "keep_length_without_a": (("-i", "none.fa", "-o", "o.aln", "--keep-length"), "--keep-length applies to placement into a backbone alignment: give it with -a"),
    "keep_length_with_a_tree_and_no_a": (("-t", "none.nwk", "-i", "none.fa", "-o", "o.aln", "--keep-length"), "--keep-length applies to placement into a backbone alignment: give it with -a"),
    "keep_length_with_place_on_tree": (("-a", "none.aln", "-t", "none.nwk", "-i", "none.fa", "-o", "o.aln", "--place-on-tree", "--keep-length"),
                                       "--keep-length is not available with --place-on-tree"),
    "keep_length_with_f": (("-f", "nonedir", "-o", "o.aln", "--keep-length"), "--keep-length cannot be combined with -f"),
    "keep_length_with_f_and_a": (("-f", "nonedir", "-a", "none.aln", "-i", "none.fa", "-o", "o.aln", "--keep-length"), "--keep-length cannot be combined with -f"),
    "write_insertions_without_keep_length": (("-a", "none.aln", "-i", "none.fa", "-o", "o.aln", "--write-insertions", "ins.tsv"),
                                             "--write-insertions applies to a run with --keep-length"),
    "write_insertions_without_keep_length_or_a": (("-t", "none.nwk", "-i", "none.fa", "-o", "o.aln", "--write-insertions", "ins.tsv"),
                                                  "--write-insertions applies to a run with --keep-length"),
    "write_insertions_names_the_output": (("-a", "none.aln", "-i", "none.fa", "-o", "o.aln", "--keep-length", "--write-insertions", "o.aln"),
                                          "--write-insertions names the same file as -o"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals(built, tmp_path, case):
    args, message = REFUSALS[case]
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "ERROR: " + message in r.stderr, r.stderr
    assert "cant open" not in r.stderr and "twl_init" not in r.stderr and "Backbone" not in r.stderr
    assert os.listdir(tmp_path) == []


def test_each_refusal_has_its_own_message():
    texts = [m for _, m in REFUSALS.values()]
    assert len(set(texts)) == 5
    assert all("--keep-length" in m or "--write-insertions" in m for m in texts)


def test_write_insertions_needs_a_value(built):
    r = _cli("-a", "none.aln", "-i", "none.fa", "-o", "o.aln", "--keep-length", "--write-insertions")
    assert r.returncode == 1 and "missing value for --write-insertions" in r.stderr


def test_what_placement_refused_before_is_refused_with_the_same_text(built, tmp_path):
    out = str(tmp_path / "o.aln")
    r = _cli("-a", "x.aln", "-t", "x.nwk", "-i", "x.fa", "-o", out, "--keep-length")
    assert r.returncode == 1 and "not supported yet" in r.stderr and "--keep-length" not in r.stderr
    r = _cli("-a", "x.aln", "-i", "x.fa", "-o", out, "--host-staged", "--keep-length")
    assert r.returncode == 1 and "--host-staged is not available in placement mode (-a)" in r.stderr
    r = _cli("-a", "x.aln", "-i", "x.fa", "-o", out, "--gpu-index", "0,1", "--keep-length")
    assert r.returncode == 1 and "placement mode (-a) runs on one GPU" in r.stderr


def test_the_usage_text_names_both_flags(built):
    r = _cli("-h")
    assert r.returncode == 1 and "--keep-length [--write-insertions <file>]" in r.stderr


def test_checker_binary_keeps_calling_the_flags_unsupported(built):
    """The CPU-check build of the same driver.cpp carries no placement: both flags stay unsupported options there."""
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = _cli("--keep-length", "-a", "x.aln", "-i", "x.fa", "-o", "o.aln", exe=exe)
    assert r.returncode == 1 and "unsupported option --keep-length" in r.stderr
    r = _cli("--write-insertions", "f", exe=exe)
    assert r.returncode == 1 and "unsupported option --write-insertions" in r.stderr


def test_placement_without_a_device_fails_as_before(built, tmp_path):
    """With no device visible to the process, -a reads its inputs and then fails at twl_init, with the flag and without it: the flag adds
    no step in front of the device, writes no file and says nothing of its own."""
    bb, new = tmp_path / "bb.aln", tmp_path / "new.fa"
    bb.write_bytes(b">a\nACGT\n>b\nAC-T\n")
    new.write_bytes(b">n\nACGGT\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    got = []
    for flags in ((), ("--keep-length", "--write-insertions", str(tmp_path / "ins.tsv"))):
        r = _cli("-a", str(bb), "-i", str(new), "-o", str(tmp_path / "o.aln"), *flags, env=env)
        assert r.returncode == 1, r.stderr
        assert "ERROR: twl_init failed" in r.stderr and "Low-quality sequences (not placed): 0" in r.stderr
        assert "Kept the backbone's length" not in r.stderr
        got.append((r.stdout, r.stderr))
    assert got[0] == got[1]
    assert sorted(os.listdir(tmp_path)) == ["bb.aln", "new.fa"]
