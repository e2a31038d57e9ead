"""The pure host decisions of the twl_guide_set_* calls (twilight_amd/csrc/twl_guide_set_plan.inc.hip) against their known answers
(tests/guide_set_plan_kats.cpp), compiled by g++ alone; and the calls themselves where they refuse before any device work.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")


def test_guide_set_plan_known_answers(tmp_path):
    exe = tmp_path / "guide_set_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "guide_set_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == 47


def test_every_refusal_is_written_in_the_plan_file():
    """twl_guide_set.inc.hip allocates, uploads, launches and downloads; what the calls reject is decided in the pure file alone."""
    host = open(os.path.join(CSRC, "twl_guide_set.inc.hip")).read()
    plan = open(os.path.join(CSRC, "twl_guide_set_plan.inc.hip")).read()
    for message in ("more than 1048576 sequences in a set", "seed id out of range", "the same sequence is a seed twice", "an empty group", "the group offsets decrease",
                    "a group of more than 16384 sequences", "more than 2^28 entries", "sequence id out of range", "the number of seeds must be between 1 and 16384"):
        assert message in plan and message not in host, message
    for call in ("hipMalloc", "hipMemcpy", "hipLaunch", "<<<"):
        assert call not in plan, call


def test_the_calls_refuse_before_any_device_work(built):
    """On a machine without a device, and without twl_init: the refusals of the check functions come first, then the missing initialisation."""
    import twilight_amd as twl
    from twilight_amd import guide

    with pytest.raises(twl.TwlError, match="no sequences"):
        guide.GuideSet([], "n")
    with pytest.raises(twl.TwlError, match="the type must be 'n' or 'p'"):
        guide.GuideSet([b"ACGTACGT"], "x")
    lib = guide._lib()
    out = np.zeros(4, dtype=np.int32)
    ids = np.zeros(4, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for rc in (lib.twl_guide_set_assign(None, C.c_int32(1), p(ids), p(out), None), lib.twl_guide_set_shared_groups(None, C.c_int32(1), p(ids), p(ids), p(out)),
               lib.twl_guide_set_weights(None, p(out)), lib.twl_guide_set_timing(None, None, None, None, None)):
        with pytest.raises(twl.TwlError, match="bad argument"):
            twl.api._check(rc)
    assert lib.twl_guide_set_destroy(None) == 0
    assert guide.SET_MAX_SEQS == 1048576 and "#define TWL_GUIDE_SET_MAX_SEQS 1048576" in open(os.path.join(ROOT, "include", "twl_guide.h")).read()
    assert guide.MAX_SEQS == 16384


def test_the_new_files_are_kernel_sources():
    import __graft_entry__ as g

    for f in ("guide_stage_kernels.hip.h", "twl_guide_set.inc.hip", "twl_guide_set_plan.inc.hip"):
        assert f in g.KERNEL_SOURCES
    text = open(os.path.join(CSRC, "twl_align.hip")).read()
    assert '#include "twl_guide_set.inc.hip"' in text
