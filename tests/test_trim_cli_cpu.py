"""`--trim-gappy`, `--trim-to` and `--write-columns` on the command line, before a file is read or a device opened: every refusal by exit
code and message; the CPU checker's build of the same parser knows none of the three flags; a run without them is what it was.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")


def _cli(*args, env=None, exe=EXE, cwd=None):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, env=env, cwd=cwd)


BASE = ("-t", "none.nwk", "-i", "none.fa", "-o", "o.aln")
# none of the named files exists: a refusal that came after a read would say so instead
REFUSALS = {
    "both_rules": (BASE + ("--trim-gappy", "0.9", "--trim-to", "x"), "--trim-gappy and --trim-to cannot be combined"),
    "both_rules_in_merge_mode": (("-f", "nonedir", "-o", "o.aln", "--trim-to", "x", "--trim-gappy", "0.9"), "--trim-gappy and --trim-to cannot be combined"),
    "T_not_a_number": (BASE + ("--trim-gappy", "many"), "--trim-gappy needs a value in [0, 1] (got many)"),
    "T_with_a_tail": (BASE + ("--trim-gappy", "0.5x"), "--trim-gappy needs a value in [0, 1] (got 0.5x)"),
    "T_negative": (BASE + ("--trim-gappy", "-0.1"), "--trim-gappy needs a value in [0, 1] (got -0.1)"),
    "T_above_1": (BASE + ("--trim-gappy", "1.01"), "--trim-gappy needs a value in [0, 1] (got 1.01)"),
    "T_nan": (BASE + ("--trim-gappy", "nan"), "--trim-gappy needs a value in [0, 1] (got nan)"),
    "write_columns_without_a_rule": (BASE + ("--write-columns", "cols.tsv"), "--write-columns applies to a run with --trim-gappy or --trim-to"),
    "write_columns_names_the_output": (BASE + ("--trim-gappy", "0.9", "--write-columns", "o.aln"), "--write-columns names the same file as -o"),
    "trim_gappy_with_keep_length": (("-a", "none.aln", "-i", "none.fa", "-o", "o.aln", "--keep-length", "--trim-gappy", "0.9"),
                                    "--trim-gappy and --trim-to cannot be combined with --keep-length"),
    "trim_to_with_keep_length": (("-a", "none.aln", "-i", "none.fa", "-o", "o.aln", "--trim-to", "x", "--keep-length"),
                                 "--trim-gappy and --trim-to cannot be combined with --keep-length"),
    "trim_gappy_host_staged": (BASE + ("--host-staged", "--trim-gappy", "0.9"), "--host-staged is not available with --trim-gappy or --trim-to"),
    "trim_to_host_staged": (BASE + ("--trim-to", "x", "--host-staged"), "--host-staged is not available with --trim-gappy or --trim-to"),
    "trim_gappy_two_gpus": (BASE + ("--gpu-index", "0,1", "--trim-gappy", "0.9"), "--trim-gappy and --trim-to run on one GPU"),
    "trim_to_two_gpus": (BASE + ("-G", "2", "--trim-to", "x"), "--trim-gappy and --trim-to run on one GPU"),
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
    texts = {m.split(" (got")[0] for _, m in REFUSALS.values()}
    assert len(texts) == 7      # both rules, T, --write-columns without a rule, ... naming -o, --keep-length, --host-staged, more than one GPU


@pytest.mark.parametrize("flag", ["--trim-gappy", "--trim-to", "--write-columns"])
def test_the_flags_need_a_value(built, flag):
    r = _cli(*BASE, flag)
    assert r.returncode == 1 and "missing value for " + flag in r.stderr


@pytest.mark.parametrize("T", ["0", "1", "0.95", "1e-3", "0x1p-1"])
def test_the_ends_of_the_range_pass_the_parser(built, tmp_path, T):
    """T = 0 and T = 1 are values: the run goes on to its first file, which is not there."""
    r = _cli(*BASE, "--trim-gappy", T, cwd=tmp_path)
    assert r.returncode != 0 and "--trim-gappy needs" not in r.stderr and "unsupported option" not in r.stderr
    assert os.listdir(tmp_path) == []


def test_the_usage_text_names_the_flags(built):
    r = _cli("-h")
    assert r.returncode == 1 and "[--trim-gappy T | --trim-to NAME] [--write-columns <file>]" in r.stderr


@pytest.mark.parametrize("flag", ["--trim-gappy", "--trim-to", "--write-columns"])
def test_checker_binary_keeps_calling_the_flags_unsupported(built, flag):
    """The CPU-check build of the same driver.cpp carries no trim: the three flags stay unsupported options there."""
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = _cli(*BASE, flag, "0.5", exe=exe)
    assert r.returncode == 1 and "unsupported option " + flag in r.stderr


def test_the_library_entry_knows_none_of_the_flags(built):
    """twl_msa_open parses its arguments without the trim: a library caller has twl_store_trim_columns itself."""
    src = open(os.path.join(ROOT, "twilight_amd", "csrc", "host", "capi.cpp")).read()
    assert src.count("parseCommandLine(") == 1
    assert "parseCommandLine((int)av.size(), av.data(), m->option))" in src, "twl_msa_open passes no allow switch: every one defaults to false"
    hdr = open(os.path.join(ROOT, "twilight_amd", "csrc", "host", "twl_host.hpp")).read()
    assert "bool allowTrim = false);" in hdr


def test_a_run_without_a_device_fails_as_before(built, tmp_path):
    """With no device visible to the process a default run reads its inputs and fails at twl_init, with the flags and without them: the
    flags add no step in front of the device, write no file and say nothing of their own."""
    tree, seqs = tmp_path / "t.nwk", tmp_path / "s.fa"
    tree.write_bytes(b"((a:0.1,b:0.1):0.1,c:0.2);\n")
    seqs.write_bytes(b">a\nACGTACGT\n>b\nACGACGT\n>c\nACGTACG\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    got = []
    for flags in ((), ("--trim-gappy", "0.5", "--write-columns", str(tmp_path / "cols.tsv")), ("--trim-to", "a")):
        r = _cli("-t", str(tree), "-i", str(seqs), "-o", str(tmp_path / "o.aln"), *flags, env=env)
        assert r.returncode == 1, r.stderr
        assert "twl_init failed" in r.stderr
        assert "Trimmed" not in r.stderr
        got.append((r.stdout, r.stderr))
    assert got[0] == got[1] == got[2]
    assert sorted(os.listdir(tmp_path)) == ["s.fa", "t.nwk"]
