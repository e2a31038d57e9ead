"""The pure host decisions of the twl_retree_set_* calls (twilight_amd/csrc/twl_retree_set_plan.inc.hip) against their known answers
(tests/retree_set_plan_kats.cpp), compiled by g++ alone; header, binding and library name the same symbols; and the calls themselves where
they refuse before any device work.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")
NEW_FILES = ("retree_stage_kernels.hip.h", "twl_retree_set.inc.hip", "twl_retree_set_plan.inc.hip")
REFUSALS = ("more than 1048576 rows in a set", "seed id out of range", "the same row is a seed twice", "no groups", "an empty group", "the group offsets decrease",
            "the first group must start at 0", "a group of more than 16384 rows", "more than 2^28 entries", "row id out of range",
            "the number of seeds must be between 1 and 16384", "no rows", "the rows have no columns", "max_gaps must lie in 0 .. n", "the type must be 'n' or 'p'")


def test_retree_set_plan_known_answers(tmp_path):
    exe = tmp_path / "retree_set_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "retree_set_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == 64
    for name in ("slabs_of_65535_rows", "slabs_of_65536_rows", "slabs_of_131071_rows", "plan_group_of_1", "plan_group_of_2", "plan_group_of_63", "plan_group_of_64",
                 "plan_group_of_65", "plan_group_of_130"):
        assert "OK " + name in lines, name


def test_every_refusal_is_written_in_the_plan_file():
    """twl_retree_set.inc.hip allocates, uploads, launches and downloads, and twl_retree.inc.hip gains nothing: what the calls reject is
    decided in the pure file alone, which makes no HIP call and holds no global."""
    host = open(os.path.join(CSRC, "twl_retree_set.inc.hip")).read()
    old_host = open(os.path.join(CSRC, "twl_retree.inc.hip")).read()
    plan = open(os.path.join(CSRC, "twl_retree_set_plan.inc.hip")).read() + open(os.path.join(CSRC, "twl_retree_plan.inc.hip")).read()
    for message in REFUSALS:
        assert message in plan and message not in host and message not in old_host, message
    code = re.sub(r"//.*", "", open(os.path.join(CSRC, "twl_retree_set_plan.inc.hip")).read())
    code = re.sub(r'#include "[^"]*"', "", code)      # (the two pure plan files it includes carry .inc.hip in their names)
    assert "hip" not in code.lower(), "the plan file makes no HIP call"
    assert "g_err" not in code and "g_init" not in code and not re.search(r"^\s*static\s", code, flags=re.M), "the plan file reads and writes no global"
    for line in code.splitlines():      # at file scope: only includes, constexpr constants, and inline functions
        if line and not line[0].isspace() and line[0] not in "{}#":
            assert line.startswith(("inline ", "constexpr ")), line


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_header_matches_binding_and_library(built):
    import twilight_amd as twl
    from twilight_amd import retree_set

    want = {"twl_retree_set_describe", "twl_retree_set_create", "twl_retree_set_destroy", "twl_retree_set_letters", "twl_retree_set_assign",
            "twl_retree_set_pair_groups", "twl_retree_set_timing"}
    assert set(_declared("twl_retree_set.h")) == want == set(retree_set.exported_symbols())
    lib = twl.load_library()
    for name in want:
        assert getattr(lib, name) is not None, name
    assert retree_set.SET_MAX_SEQS == 1048576 and "#define TWL_RETREE_SET_MAX_SEQS 1048576" in open(os.path.join(ROOT, "include", "twl_retree_set.h")).read()
    d = retree_set.describe()
    assert d == {"assign_rows": 64, "assign_seeds": 64, "group_tile": 64, "pack_rows": 65535}


def test_the_new_files_are_kernel_sources():
    import __graft_entry__ as g

    for f in NEW_FILES:
        assert f in g.KERNEL_SOURCES
    text = open(os.path.join(CSRC, "twl_align.hip")).read()
    assert '#include "twl_retree_set.inc.hip"' in text and '#include "../../include/twl_retree_set.h"' in text
    assert text.index('#include "retree_kernels.hip.h"') < text.index('#include "retree_stage_kernels.hip.h"')
    assert "twl_retree_set.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_the_calls_refuse_before_any_device_work(built):
    """On a machine without a device, and without twl_init: the refusals of the plan file come first."""
    import twilight_amd as twl
    from twilight_amd import retree_set

    rows = [b"AC-T", b"A-GT", b"acgu"]
    with pytest.raises(twl.TwlError, match="no rows"):
        retree_set.RetreeSet([], "n", 0)
    with pytest.raises(twl.TwlError, match="the rows have no columns"):
        retree_set.RetreeSet([b"", b""], "n", 0)
    with pytest.raises(twl.TwlError, match="the type must be 'n' or 'p'"):
        retree_set.RetreeSet(rows, "x", 1)
    for mg in (-1, 4):
        with pytest.raises(twl.TwlError, match="max_gaps must lie in 0 .. n"):
            retree_set.RetreeSet(rows, "n", mg)
    lib = retree_set._lib()
    out = np.zeros(4, dtype=np.int32)
    ids = np.zeros(4, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for rc in (lib.twl_retree_set_assign(None, C.c_int32(1), p(ids), p(out), None, None), lib.twl_retree_set_pair_groups(None, C.c_int32(1), p(ids), p(ids), p(out), p(out)),
               lib.twl_retree_set_letters(None, p(out)), lib.twl_retree_set_timing(None, None, None, None, None, None, None), lib.twl_retree_set_describe(None)):
        with pytest.raises(twl.TwlError, match="bad argument"):
            twl.api._check(rc)
    assert lib.twl_retree_set_destroy(None) == 0
