"""The pure host decisions of the retree calls (twilight_amd/csrc/twl_retree_plan.inc.hip) against their known answers
(tests/retree_plan_kats.cpp), compiled by g++ alone; retree_max_gaps against the restatement's math.floor(float(T) * n); header, binding and
library name the same symbols.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import retree_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    exe = tmp_path_factory.mktemp("retree_plan") / "retree_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "retree_plan_kats.cpp")])
    return str(exe)


def test_retree_plan_known_answers(kats):
    r = subprocess.run([kats], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == 41


def test_max_gaps_is_the_restatements(kats):
    """floor(T * n) in double: the exact cases of the definition, the default, and values of T whose product with n lands next to an integer."""
    cases = [(1.0, 1), (1.0, 7), (1.0, 16384), (0.5, 4), (0.25, 3), (0.95, 20), (0.95, 200), (0.95, 16384), (0.1, 10), (0.1, 30), (0.7, 10), (0.3, 10), (0.29, 100), (0.57, 100),
             (1e-9, 5), (float(np.nextafter(1.0, 0.0)), 16384), (float(np.nextafter(0.5, 0.0)), 4), (float(np.nextafter(0.5, 1.0)), 4)]
    rng = np.random.default_rng(4)
    cases += [(float(rng.random()) or 0.5, int(rng.integers(1, 16385))) for _ in range(200)]
    text = "".join("%s %d\n" % (float(t).hex(), n) for t, n in cases)
    r = subprocess.run([kats, "maxgaps"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert got == [R.max_gaps(t, n) for t, n in cases]
    assert got[1] == 7 and got[3] == 2 and got[4] == 0


def test_every_refusal_is_written_in_the_plan_file():
    """twl_retree.inc.hip allocates, uploads, launches and downloads; what the calls reject is decided in the pure file alone."""
    host = open(os.path.join(CSRC, "twl_retree.inc.hip")).read()
    plan = open(os.path.join(CSRC, "twl_retree_plan.inc.hip")).read()
    for message in ("no rows", "more than 16384 rows", "the rows have no columns", "max_gaps must lie in 0 .. n", "the type must be 'n' or 'p'"):
        assert message in plan and message not in host, message
    assert "hip" not in re.sub(r"//.*", "", plan).lower(), "the plan file makes no HIP call"


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_retree_header_matches_binding_and_library(built):
    import twilight_amd as twl
    from twilight_amd import retree

    assert set(_declared("twl_retree.h")) == {"twl_retree_describe", "twl_retree_column_gaps", "twl_retree_pair_counts", "twl_retree_timing"}
    assert set(_declared("twl_retree.h")) == set(retree.exported_symbols())
    lib = twl.load_library()
    for name in _declared("twl_retree.h"):
        assert getattr(lib, name) is not None, name
    import __graft_entry__ as g

    for f in ("twl_retree.inc.hip", "twl_retree_plan.inc.hip", "retree_kernels.hip.h"):
        assert f in g.KERNEL_SOURCES
    assert retree.MAX_SEQS == 16384 and "#define TWL_RETREE_MAX_SEQS 16384" in open(os.path.join(ROOT, "include", "twl_retree.h")).read()


def test_the_calls_refuse_before_any_device_work(built):
    """On a machine without a device, and without twl_init: the refusals of the plan file come first, then the missing initialisation."""
    import twilight_amd as twl
    from twilight_amd import retree

    rows = [b"AC-T", b"A-GT", b"acgu"]
    with pytest.raises(twl.TwlError, match="no rows"):
        retree.pair_counts([], "n", 0)
    with pytest.raises(twl.TwlError, match="no rows"):
        retree.column_gaps([])
    with pytest.raises(twl.TwlError, match="the rows have no columns"):
        retree.pair_counts([b"", b""], "n", 0)
    with pytest.raises(twl.TwlError, match="the type must be 'n' or 'p'"):
        retree.pair_counts(rows, "x", 1)
    for mg in (-1, 4):
        with pytest.raises(twl.TwlError, match="max_gaps must lie in 0 .. n"):
            retree.pair_counts(rows, "n", mg)
    d = retree.describe()
    assert d["word_columns"] == 64 and d["pair_tile"] > 0 and d["slice_words"] > 0 and d["gap_rows"] > 0
