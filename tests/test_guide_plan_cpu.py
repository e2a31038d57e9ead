"""The pure host decisions of the guide calls (twilight_amd/csrc/twl_guide_plan.inc.hip) against their known answers
(tests/guide_plan_kats.cpp), compiled by g++ alone.  No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")


def test_guide_plan_known_answers(tmp_path):
    exe = tmp_path / "guide_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "guide_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == 26


def test_every_refusal_is_written_in_the_plan_file():
    """twl_guide.inc.hip allocates, uploads, launches and downloads; what the calls reject is decided in the pure file alone."""
    host = open(os.path.join(CSRC, "twl_guide.inc.hip")).read()
    plan = open(os.path.join(CSRC, "twl_guide_plan.inc.hip")).read()
    for message in ("no sequences", "more than 16384 sequences", "negative sequence length"):
        assert message in plan and message not in host, message
    assert "hip" not in re.sub(r"//.*", "", plan).lower(), "the plan file makes no HIP call"


def test_the_calls_refuse_before_any_device_work(built):
    """On a machine without a device, and without twl_init: the refusals of check_guide come first, then the missing initialisation."""
    import ctypes as C

    import numpy as np
    import pytest

    import twilight_amd as twl
    from twilight_amd import guide

    with pytest.raises(twl.TwlError, match="no sequences"):
        guide.shared([], "n")
    with pytest.raises(twl.TwlError, match="the type must be 'n' or 'p'"):
        lib = guide._lib()
        out = np.zeros(4, dtype=np.uint32)
        ptrs = (C.c_char_p * 1)(b"ACGT")
        lens = np.array([4], dtype=np.int32)
        twl.api._check(lib.twl_guide_shared(C.c_int(0), C.c_char(b"x"), C.c_int32(1), ptrs, lens.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_uint32))))
    with pytest.raises(twl.TwlError, match="the type must be"):
        guide.bins("q")
    assert guide.bins("n") == 4096 and guide.bins("p") == 7776
    d = guide.describe()
    assert d["count_round"] % d["count_chunk"] == 0 and d["pair_tile"] > 0 and d["bin_slice"] > 0
