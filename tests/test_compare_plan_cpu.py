"""The pure host decisions of the comparison (twilight_amd/csrc/twl_compare_plan.inc.hip) against their known answers
(tests/compare_plan_kats.cpp), compiled by g++ alone, plain and under the address and undefined-behaviour sanitizers; the ABI's symbol list,
header against binding against library; the build lists; the kernels' constants.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")

MUST = ("rejects_null_estimate", "rejects_null_reference", "rejects_null_object", "rejects_null_bad_row", "rejects_one_row", "rejects_one_row_too_many",
        "rejects_a_negative_estimate_width", "rejects_a_negative_reference_width", "rejects_one_estimate_column_more", "rejects_one_reference_column_more",
        "accepts_the_widest_estimate", "ten_thousand_by_hundred_thousand", "its_last_cell_lies_past_2_to_the_31_bytes", "hundred_thousand_by_38524",
        "its_row_offsets_pass_2_to_the_31", "the_largest_object_does_not_wrap")


@pytest.mark.parametrize("flags", [("-O1",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_compare_plans_known_answers(tmp_path, flags):
    exe = tmp_path / "compare_plan_kats"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "compare_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 30
    names = {l.split()[1] for l in lines}
    for must in MUST:
        assert must in names, must


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_compare_header_matches_binding():
    from twilight_amd import compare, trim

    assert set(_declared("twl_compare.h")) == set(compare.exported_symbols())
    assert set(compare.exported_symbols()) == {"twl_compare_create", "twl_compare_columns", "twl_compare_timing", "twl_compare_describe", "twl_compare_destroy"}
    assert set(_declared("twl_trim.h")) == set(trim.exported_symbols()) and not set(trim.exported_symbols()) & set(compare.exported_symbols())


def test_compare_symbols_are_exported(built):
    import twilight_amd as twl

    lib = twl.load_library()
    for name in _declared("twl_compare.h"):
        assert getattr(lib, name) is not None, name


def test_the_constants_need_no_device(built):
    """twl_compare_describe answers before twl_init.  Two workgroups of the column kernel share a CU's 160 KiB: T counters of 4 bytes for each
    column of a tile are at most 72 KiB, which leaves 8 KiB for the reduction tables of each; a lane per column of the tile; a scan round is a
    whole number of tiles."""
    from twilight_amd import compare

    T, TILE, STEP, CHUNK = compare.describe()
    assert T & (T - 1) == 0 and T >= 64
    assert TILE == 64
    assert T * TILE * 4 <= 72 * 1024
    assert STEP % 4 == 0 and 4 <= STEP <= 256
    assert CHUNK % TILE == 0 and CHUNK == 256 * 4


def test_the_calls_refuse_null_arguments_before_any_device_work(built):
    import twilight_amd as twl
    from twilight_amd import compare

    lib = compare._lib()
    h = C.c_void_p(None)
    bad = C.c_int32(7)
    rows = (C.c_void_p * 2)()
    for rc in (lib.twl_compare_create(C.c_int(0), C.c_int32(2), C.c_int32(3), None, C.c_int32(3), rows, C.byref(h), C.byref(bad)),
               lib.twl_compare_create(C.c_int(0), C.c_int32(2), C.c_int32(3), rows, C.c_int32(3), rows, C.byref(h), C.byref(bad)),      # null rows
               lib.twl_compare_columns(None, None, None, None, None, None), lib.twl_compare_timing(None, None, None, None, None), lib.twl_compare_describe(None)):
        with pytest.raises(twl.TwlError, match="bad argument"):
            twl.api._check(rc)
    assert bad.value == -1 and not h.value
    assert lib.twl_compare_destroy(None) == 0
    for n, why in ((1, "at least 2 rows"), ((1 << 20) + 1, "too many rows")):
        with pytest.raises(twl.TwlError, match=why):
            twl.api._check(lib.twl_compare_create(C.c_int(0), C.c_int32(n), C.c_int32(3), rows, C.c_int32(3), rows, C.byref(h), C.byref(bad)))
    with pytest.raises(twl.TwlError, match="negative width"):
        twl.api._check(lib.twl_compare_create(C.c_int(0), C.c_int32(2), C.c_int32(-1), rows, C.c_int32(3), rows, C.byref(h), C.byref(bad)))
    with pytest.raises(twl.TwlError, match="rows too long"):
        twl.api._check(lib.twl_compare_create(C.c_int(0), C.c_int32(2), C.c_int32(2 ** 31 - 1), rows, C.c_int32(3), rows, C.byref(h), C.byref(bad)))


def test_the_new_files_are_kernel_sources_and_built():
    import __graft_entry__ as g

    for f in ("compare_kernels.hip.h", "twl_compare.inc.hip", "twl_compare_plan.inc.hip"):
        assert f in g.KERNEL_SOURCES
        assert os.path.exists(os.path.join(CSRC, f))
    unit = open(os.path.join(CSRC, "twl_align.hip")).read()
    assert unit.index('#include "twl_compare.inc.hip"') > unit.index('#include "twl_trim.inc.hip"')
    assert '#include "compare_kernels.hip.h"' in unit
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry.count('"twl_compare.h"') == 2          # the library's and the host library's header lists
    assert '"compare.cpp"' in entry and '"-DTWL_COMPARE"' in entry


def test_the_plan_file_makes_no_hip_call():
    text = open(os.path.join(CSRC, "twl_compare_plan.inc.hip")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()


def test_the_kernels_use_no_floating_point():
    text = re.sub(r"//.*", "", open(os.path.join(CSRC, "compare_kernels.hip.h")).read())
    assert not re.search(r"\b(float|double|half)\b", text)
    assert "unsigned long long" in text, "the C(k, 2) products and their sums are 64-bit"
