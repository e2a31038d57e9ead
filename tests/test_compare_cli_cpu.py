"""`--compare`, `--write-compare` and `--evaluate` on the command line, before a file is read or a device opened: every refusal by exit code
and message; the CPU checker's build of the same parser knows none of the three flags; a run without them is what it was.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")


def _cli(*args, env=None, exe=EXE, cwd=None):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, env=env, cwd=cwd)


BASE = ("-t", "none.nwk", "-i", "none.fa", "-o", "o.aln")
CMP = ("--compare", "none_ref.aln")
EVAL = ("--evaluate", "none_est.aln") + CMP
# none of the named files exists: a refusal that came after a read would say so instead
REFUSALS = {
    "with_adjust_direction": (BASE + CMP + ("--adjust-direction",), "--compare cannot be combined with --adjust-direction"),
    "with_keep_length": (("-a", "none.aln", "-i", "none.fa", "-o", "o.aln", "--keep-length") + CMP, "--compare cannot be combined with --keep-length"),
    "with_trim_gappy": (BASE + ("--trim-gappy", "0.9") + CMP, "--compare cannot be combined with --trim-gappy or --trim-to"),
    "with_trim_to": (BASE + CMP + ("--trim-to", "x"), "--compare cannot be combined with --trim-gappy or --trim-to"),
    "host_staged": (BASE + ("--host-staged",) + CMP, "--host-staged is not available with --compare"),
    "two_gpus": (BASE + CMP + ("--gpu-index", "0,1"), "--compare runs on one GPU"),
    "two_gpus_by_count": (BASE + ("-G", "2") + CMP, "--compare runs on one GPU"),
    "write_compare_alone": (BASE + ("--write-compare", "c.tsv"), "--write-compare applies to a run with --compare"),
    "write_compare_names_the_output": (BASE + CMP + ("--write-compare", "o.aln"), "--write-compare names the same file as -o"),
    "evaluate_alone": (("--evaluate", "none_est.aln"), "--evaluate needs --compare"),
    "evaluate_with_t": (EVAL + ("-t", "none.nwk"), "--evaluate compares two files and runs nothing"),
    "evaluate_with_i": (EVAL + ("-i", "none.fa"), "--evaluate compares two files and runs nothing"),
    "evaluate_with_a": (EVAL + ("-a", "none.aln"), "--evaluate compares two files and runs nothing"),
    "evaluate_with_f": (EVAL + ("-f", "nonedir"), "--evaluate compares two files and runs nothing"),
    "evaluate_with_o": (EVAL + ("-o", "o.aln"), "--evaluate compares two files and runs nothing"),
    "evaluate_with_m": (EVAL + ("-m", "100"), "--evaluate compares two files and runs nothing"),
    "evaluate_with_iterations": (EVAL + ("--iterations", "2"), "--evaluate compares two files and runs nothing"),
    "evaluate_with_one_iteration": (EVAL + ("--iterations", "1"), "--evaluate compares two files and runs nothing"),
    "in_merge_mode_two_gpus": (("-f", "nonedir", "-o", "o.aln", "--gpu-index", "0,1") + CMP, "--compare runs on one GPU"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals(built, tmp_path, case):
    args, message = REFUSALS[case]
    r = _cli(*args, cwd=tmp_path)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "ERROR: " + message in r.stderr, r.stderr
    assert "cant open" not in r.stderr and "twl_init" not in r.stderr and "Failed to open" not in r.stderr
    assert os.listdir(tmp_path) == []


def test_each_refusal_has_its_own_message():
    texts = {m for _, m in REFUSALS.values()}
    assert len(texts) == 9      # --adjust-direction, --keep-length, the trim, --host-staged, GPUs, --write-compare twice, --evaluate twice


@pytest.mark.parametrize("flag", ["--compare", "--write-compare", "--evaluate"])
def test_the_flags_need_a_value(built, flag):
    r = _cli(*BASE, flag)
    assert r.returncode == 1 and "missing value for " + flag in r.stderr


def test_the_flags_pass_the_parser(built, tmp_path):
    """Accepted; the reference must be readable before anything runs (a mistyped path does not cost the run), then the run goes on to its
    first file, which is not there; --evaluate asks for its own file first."""
    r = _cli(*BASE, *CMP, "--write-compare", "c.tsv", cwd=tmp_path)
    assert r.returncode == 1 and "unsupported option" not in r.stderr and "ERROR: --compare: cant open file: none_ref.aln" in r.stderr
    r = _cli(*EVAL, "--write-compare", "c.tsv", cwd=tmp_path)
    assert r.returncode == 1 and "ERROR: --evaluate: cant open file: none_est.aln" in r.stderr
    assert os.listdir(tmp_path) == []
    (tmp_path / "none_ref.aln").write_bytes(b">a\nAC\n>b\nAC\n")
    r = _cli(*BASE, *CMP, "--write-compare", "c.tsv", cwd=tmp_path)
    assert r.returncode != 0 and "--compare" not in r.stderr and "none_ref.aln" not in r.stderr, "the run goes on to its own inputs"
    assert os.listdir(tmp_path) == ["none_ref.aln"]


def test_evaluate_reads_both_files_before_it_opens_a_device(built, tmp_path):
    """Rows of unequal length inside a file, fewer than 2 common names: refused from the files alone, nothing written."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    est, ref, ragged, other = tmp_path / "e.aln", tmp_path / "r.aln", tmp_path / "ragged.aln", tmp_path / "other.aln"
    est.write_bytes(b">a\nAC-G\n>b\nA-CG\n>c\nACG-\n")
    ref.write_bytes(b">a x\nACG-\n>b\nACG-\n>d\nACG-\n")
    ragged.write_bytes(b">a\nAC-G\n>b\nA-C\n")
    other.write_bytes(b">a\nACG\n>x\nACG\n>y\nACG\n")
    r = _cli("--evaluate", str(ragged), "--compare", str(ref), env=env)
    assert r.returncode == 1 and "ERROR: --evaluate: the rows of " + str(ragged) + " differ in length" in r.stderr
    r = _cli("--evaluate", str(est), "--compare", str(ragged), env=env)
    assert r.returncode == 1 and "ERROR: --compare: the rows of " + str(ragged) + " differ in length" in r.stderr
    r = _cli("--evaluate", str(est), "--compare", str(other), "--write-compare", str(tmp_path / "c.tsv"), env=env)
    assert r.returncode == 1 and "have 1 name(s) in common; a comparison needs at least 2 (2 only in the output, 2 only in the reference)" in r.stderr
    assert "twl_init" not in r.stderr
    r = _cli("--evaluate", str(est), "--compare", str(ref), "--write-compare", str(tmp_path / "c.tsv"), env=env)
    assert r.returncode == 1 and "twl_init failed" in r.stderr, "two common names: the comparison goes on to the device, which is not there"
    assert sorted(os.listdir(tmp_path)) == ["e.aln", "other.aln", "r.aln", "ragged.aln"]


def test_the_usage_text_names_the_flags(built):
    r = _cli("-h")
    assert r.returncode == 1 and "--compare <reference.aln[.gz]> [--write-compare <file>]" in r.stderr
    assert "--evaluate <alignment.aln[.gz]> --compare <reference.aln[.gz]>" in r.stderr


@pytest.mark.parametrize("flag", ["--compare", "--write-compare", "--evaluate"])
def test_checker_binary_keeps_calling_the_flags_unsupported(built, flag):
    """The CPU-check build of the same driver.cpp carries no comparison: the three flags stay unsupported options there."""
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = _cli(*BASE, flag, "x.aln", exe=exe)
    assert r.returncode == 1 and "unsupported option " + flag in r.stderr


def test_the_library_entry_knows_none_of_the_flags(built):
    """twl_msa_open parses its arguments with a fresh Option: allowCompare stays false there."""
    src = open(os.path.join(ROOT, "twilight_amd", "csrc", "host", "capi.cpp")).read()
    assert "allowCompare" not in src and "compareWritten" not in src
    hdr = open(os.path.join(ROOT, "twilight_amd", "csrc", "host", "twl_host.hpp")).read()
    assert "bool allowCompare = false;" in hdr


def test_a_run_without_a_device_fails_as_before(built, tmp_path):
    """With no device visible a default run reads its inputs and fails at twl_init, with --compare and without it: the flag adds no step in
    front of the run but the check that its file can be read, writes no file and says nothing of its own."""
    tree, seqs = tmp_path / "t.nwk", tmp_path / "s.fa"
    tree.write_bytes(b"((a:0.1,b:0.1):0.1,c:0.2);\n")
    seqs.write_bytes(b">a\nACGTACGT\n>b\nACGACGT\n>c\nACGTACG\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    got = []
    ref = tmp_path / "ref.aln"
    ref.write_bytes(b">a\nACGTACGT\n>b\nACG-ACGT\n")
    for flags in ((), ("--compare", str(ref), "--write-compare", str(tmp_path / "c.tsv"))):
        r = _cli("-t", str(tree), "-i", str(seqs), "-o", str(tmp_path / "o.aln"), *flags, env=env)
        assert r.returncode == 1, r.stderr
        assert "twl_init failed" in r.stderr and "compare:" not in r.stderr
        got.append((r.stdout, r.stderr))
    assert got[0] == got[1]
    assert sorted(os.listdir(tmp_path)) == ["ref.aln", "s.fa", "t.nwk"]
