"""The pure host decisions of the keep-length finish (twilight_amd/csrc/twl_keep_plan.inc.hip) against their known answers
(tests/keep_plan_kats.cpp), compiled by g++ alone; the ABI's symbol list, header against binding against library; the build lists.
No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")


def test_keep_plans_known_answers(tmp_path):
    exe = tmp_path / "keep_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "keep_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 43
    names = {l.split()[1] for l in lines}
    # what the issue lists: finish_keep twice, either finish after the other, dropped_* before finish_keep, an id that was not collected,
    # an id listed twice, a run_off that is not the scan of the counts, n = 0
    for must in ("finish_keep_rejects_second_call", "finish_rejects_after_finish_keep", "finish_keep_rejects_after_finish", "counts_rejects_before_finish_keep",
                 "runs_rejects_before_finish_keep", "counts_rejects_uncollected_sequence", "runs_rejects_uncollected_sequence", "counts_rejects_id_twice",
                 "runs_rejects_id_twice", "runs_rejects_run_off_of_other_counts", "counts_accepts_n_0", "runs_accepts_n_0"):
        assert must in names, must


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_keep_header_matches_binding():
    from twilight_amd import keep

    assert set(_declared("twl_keep.h")) == set(keep.exported_symbols())
    for name in ("twl_place_finish_keep", "twl_place_dropped_counts", "twl_place_dropped_runs"):
        assert name in keep.exported_symbols()


def test_place_header_and_binding_keep_their_symbols():
    from twilight_amd import keep, place

    assert set(_declared("twl_place.h")) == set(place.exported_symbols())
    assert not set(place.exported_symbols()) & set(keep.exported_symbols())


def test_keep_symbols_are_exported(built):
    import twilight_amd as twl

    lib = twl.load_library()
    for name in _declared("twl_keep.h"):
        assert getattr(lib, name) is not None, name


def test_the_calls_refuse_a_null_placement_before_any_device_work(built):
    import twilight_amd as twl
    from twilight_amd import keep

    lib = keep._lib()
    for rc in (lib.twl_place_finish_keep(None, None, None), lib.twl_place_dropped_counts(None, C.c_int32(0), None, None, None),
               lib.twl_place_dropped_runs(None, C.c_int32(0), None, None, None, None, None), lib.twl_place_keep_timing(None, None, None)):
        with pytest.raises(twl.TwlError, match="bad argument"):
            twl.api._check(rc)


def test_the_new_files_are_kernel_sources_and_built():
    import __graft_entry__ as g

    for f in ("keep_kernels.hip.h", "twl_keep.inc.hip", "twl_keep_plan.inc.hip"):
        assert f in g.KERNEL_SOURCES
        assert os.path.exists(os.path.join(CSRC, f))
    unit = open(os.path.join(CSRC, "twl_align.hip")).read()
    assert unit.index('#include "twl_keep.inc.hip"') > unit.index('#include "twl_place.inc.hip"')
    assert '#include "keep_kernels.hip.h"' in unit
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry.count('"twl_keep.h"') == 2          # the library's and the host library's header lists


def test_the_placement_kernels_are_untouched():
    """The keep kernels sit in a file of their own; the placement kernels' file carries no word of them."""
    assert "keep" not in open(os.path.join(CSRC, "place_kernels.hip.h")).read()
