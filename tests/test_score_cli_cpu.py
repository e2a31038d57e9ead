"""`--score`, `--write-score` and `--score-alignment` on the command line, before a file is read or a device opened: every refusal by exit
code and message, nothing written; the CPU checker's build of the same parser knows none of the three flags; a run without them is what it
was.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")


def _cli(*args, env=None, exe=EXE, cwd=None):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, env=env, cwd=cwd)


BASE = ("-t", "none.nwk", "-i", "none.fa", "-o", "o.aln")
SA = ("--score-alignment", "none_est.aln")
NOTHING_RUNS = "--score-alignment scores a file and runs nothing"
# none of the named files exists: a refusal that came after a read would say so instead
REFUSALS = {
    "with_keep_length": (("-a", "none.aln", "-i", "none.fa", "-o", "o.aln", "--keep-length", "--score"), "--score cannot be combined with --keep-length"),
    "with_trim_gappy": (BASE + ("--trim-gappy", "0.9", "--score"), "--score cannot be combined with --trim-gappy or --trim-to"),
    "with_trim_to": (BASE + ("--score", "--trim-to", "x"), "--score cannot be combined with --trim-gappy or --trim-to"),
    "host_staged": (BASE + ("--host-staged", "--score"), "--host-staged is not available with --score"),
    "two_gpus": (BASE + ("--score", "--gpu-index", "0,1"), "--score runs on one GPU"),
    "two_gpus_by_count": (BASE + ("-G", "2", "--score"), "--score runs on one GPU"),
    "in_merge_mode_two_gpus": (("-f", "nonedir", "-o", "o.aln", "--gpu-index", "0,1", "--score"), "--score runs on one GPU"),
    "write_score_alone": (BASE + ("--write-score", "s.tsv"), "--write-score applies to a run with --score or --score-alignment"),
    "write_score_names_the_output": (BASE + ("--score", "--write-score", "o.aln"), "--write-score names the same file as -o"),
    "score_alignment_with_t": (SA + ("-t", "none.nwk"), NOTHING_RUNS),
    "score_alignment_with_i": (SA + ("-i", "none.fa"), NOTHING_RUNS),
    "score_alignment_with_a": (SA + ("-a", "none.aln"), NOTHING_RUNS),
    "score_alignment_with_f": (SA + ("-f", "nonedir"), NOTHING_RUNS),
    "score_alignment_with_o": (SA + ("-o", "o.aln"), NOTHING_RUNS),
    "score_alignment_with_m": (SA + ("-m", "100"), NOTHING_RUNS),
    "score_alignment_with_iterations": (SA + ("--iterations", "2"), NOTHING_RUNS),
    "score_alignment_with_evaluate": (SA + ("--evaluate", "none2.aln"), NOTHING_RUNS),
    "score_alignment_with_evaluate_and_compare": (SA + ("--evaluate", "none2.aln", "--compare", "none3.aln"), NOTHING_RUNS),
    "score_alignment_with_score": (SA + ("--score",), "--score-alignment cannot be combined with --score"),
    "score_alignment_two_gpus": (SA + ("--gpu-index", "0,1"), "--score-alignment runs on one GPU"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals(built, tmp_path, case):
    args, message = REFUSALS[case]
    r = _cli(*args, cwd=tmp_path)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "ERROR: " + message in r.stderr, r.stderr
    assert "cant open" not in r.stderr and "twl_init" not in r.stderr and "Failed to open" not in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("flag", ["--write-score", "--score-alignment"])
def test_the_flags_need_a_value(built, flag):
    r = _cli(*BASE, flag)
    assert r.returncode == 1 and "missing value for " + flag in r.stderr


def test_the_flags_pass_the_parser(built, tmp_path):
    """Accepted: the run goes on to its first file, which is not there; --score-alignment asks for its file before anything else."""
    r = _cli(*BASE, "--score", "--write-score", "s.tsv", cwd=tmp_path)
    assert r.returncode != 0 and "unsupported option" not in r.stderr and "--score" not in r.stderr
    r = _cli(*SA, "--write-score", "s.tsv", cwd=tmp_path)
    assert r.returncode == 1 and "ERROR: --score-alignment: cant open file: none_est.aln" in r.stderr
    assert os.listdir(tmp_path) == []


def test_score_alignment_reads_its_file_before_it_opens_a_device(built, tmp_path):
    """Rows of unequal length, a single row: refused from the file alone, nothing written."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    ragged, single, good = tmp_path / "ragged.aln", tmp_path / "single.aln", tmp_path / "good.aln"
    ragged.write_bytes(b">a\nAC-G\n>b\nA-C\n")
    single.write_bytes(b">a\nAC-G\n")
    good.write_bytes(b">a\nAC-G\n>b\nA-CG\n")
    r = _cli("--score-alignment", str(ragged), env=env)
    assert r.returncode == 1 and "ERROR: --score-alignment: the rows of " + str(ragged) + " differ in length" in r.stderr
    r = _cli("--score-alignment", str(single), "--write-score", str(tmp_path / "s.tsv"), env=env)
    assert r.returncode == 1 and "ERROR: --score-alignment: 1 row(s); a sum-of-pairs score needs at least 2." in r.stderr and "twl_init" not in r.stderr
    r = _cli("--score-alignment", str(good), "--write-score", str(tmp_path / "s.tsv"), env=env)
    assert r.returncode == 1 and "twl_init failed" in r.stderr, "two rows: the score goes on to the device, which is not there"
    assert sorted(os.listdir(tmp_path)) == ["good.aln", "ragged.aln", "single.aln"]


def test_the_usage_text_names_the_flags(built):
    r = _cli("-h")
    assert r.returncode == 1 and "--score [--write-score <file>]" in r.stderr
    assert "--score-alignment <alignment.aln[.gz]>" in r.stderr and "scores 0, with -w too" in r.stderr


@pytest.mark.parametrize("flag", ["--score", "--write-score", "--score-alignment"])
def test_checker_binary_keeps_calling_the_flags_unsupported(built, flag):
    """The CPU-check build of the same driver.cpp carries no score: the three flags stay unsupported options there."""
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = _cli(*BASE, flag, "x.aln", exe=exe)
    assert r.returncode == 1 and "unsupported option " + flag in r.stderr


def test_the_library_entry_knows_none_of_the_flags(built):
    """twl_msa_open parses its arguments with a fresh Option: allowScore stays false there."""
    src = open(os.path.join(ROOT, "twilight_amd", "csrc", "host", "capi.cpp")).read()
    assert "allowScore" not in src and "scoreWritten" not in src
    hdr = open(os.path.join(ROOT, "twilight_amd", "csrc", "host", "twl_host.hpp")).read()
    assert "bool allowScore = false;" in hdr


def test_a_run_without_a_device_fails_as_before(built, tmp_path):
    """With no device visible a default run reads its inputs and fails at twl_init, with --score and without it: the flag adds no step in front
    of the run, writes no file and says nothing of its own."""
    tree, seqs = tmp_path / "t.nwk", tmp_path / "s.fa"
    tree.write_bytes(b"((a:0.1,b:0.1):0.1,c:0.2);\n")
    seqs.write_bytes(b">a\nACGTACGT\n>b\nACGACGT\n>c\nACGTACG\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    got = []
    for flags in ((), ("--score", "--write-score", str(tmp_path / "s.tsv"))):
        r = _cli("-t", str(tree), "-i", str(seqs), "-o", str(tmp_path / "o.aln"), *flags, env=env)
        assert r.returncode == 1, r.stderr
        assert "twl_init failed" in r.stderr and "score:" not in r.stderr
        got.append((r.stdout, r.stderr))
    assert got[0] == got[1]
    assert sorted(os.listdir(tmp_path)) == ["s.fa", "t.nwk"]
