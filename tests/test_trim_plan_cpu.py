"""The pure host decisions of the column trim (twilight_amd/csrc/twl_trim_plan.inc.hip) against their known answers (tests/trim_plan_kats.cpp),
compiled by g++ alone, plain and under the address and undefined-behaviour sanitizers; the ABI's symbol list, header against binding against
library; the build lists; the kernels' constants.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")

MUST = ("rejects_null_store", "rejects_null_ids", "rejects_null_output", "rejects_no_rows", "rejects_id_8_of_8", "rejects_a_negative_id", "rejects_an_id_twice",
        "rejects_two_lengths", "rejects_a_prepared_level", "rejects_rule_2", "rejects_a_negative_limit", "rejects_a_limit_above_n", "rejects_a_reference_outside_ids",
        "rejects_one_column_more", "accepts_the_widest_row", "one_past_each", "rows_spill_into_z", "the_widest_row_does_not_wrap")


@pytest.mark.parametrize("flags", [("-O1",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_trim_plans_known_answers(tmp_path, flags):
    exe = tmp_path / "trim_plan_kats"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "trim_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 40
    names = {l.split()[1] for l in lines}
    for must in MUST:
        assert must in names, must


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_trim_header_matches_binding():
    from twilight_amd import trim

    assert set(_declared("twl_trim.h")) == set(trim.exported_symbols())
    assert set(trim.exported_symbols()) == {"twl_store_trim_columns", "twl_store_trim_read", "twl_store_trim_timing", "twl_trim_describe"}


def test_backbone_header_and_binding_keep_their_symbols():
    from twilight_amd import backbone, trim

    assert set(_declared("twl_backbone.h")) == set(backbone.exported_symbols())
    assert not set(backbone.exported_symbols()) & set(trim.exported_symbols())


def test_trim_symbols_are_exported(built):
    import twilight_amd as twl

    lib = twl.load_library()
    for name in _declared("twl_trim.h"):
        assert getattr(lib, name) is not None, name


def test_the_constants_need_no_device(built):
    """twl_trim_describe answers before twl_init: a tile is 256 threads of 16 columns, a scan round 256 words of 32, the byte counters are
    flushed before they can wrap, in whole steps of the row loop."""
    from twilight_amd import trim

    T, R, Cc, F = trim.describe()
    assert T == 256 * 16 and Cc == 256 * 32
    assert 4 <= F <= 255 and F % 4 == 0
    assert R > F, "a slice longer than a flush period, or the flush never runs"


def test_the_calls_refuse_null_arguments_before_any_device_work(built):
    import twilight_amd as twl
    from twilight_amd import trim

    lib = trim._lib()
    kept = C.c_int32(0)
    ids = (C.c_int32 * 1)(0)
    for rc in (lib.twl_store_trim_columns(None, C.c_int32(1), ids, C.c_int32(0), C.c_int32(0), C.byref(kept)), lib.twl_store_trim_read(None, None, None),
               lib.twl_store_trim_timing(None, None), lib.twl_trim_describe(None)):
        with pytest.raises(twl.TwlError, match="bad argument"):
            twl.api._check(rc)


def test_the_new_files_are_kernel_sources_and_built():
    import __graft_entry__ as g

    for f in ("trim_kernels.hip.h", "twl_trim.inc.hip", "twl_trim_plan.inc.hip"):
        assert f in g.KERNEL_SOURCES
        assert os.path.exists(os.path.join(CSRC, f))
    unit = open(os.path.join(CSRC, "twl_align.hip")).read()
    assert unit.index('#include "twl_trim.inc.hip"') > unit.index('#include "twl_backbone.inc.hip"') > unit.index('#include "twl_store.inc.hip"')
    assert '#include "trim_kernels.hip.h"' in unit
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry.count('"twl_trim.h"') == 2          # the library's and the host library's header lists
    assert '"trim.cpp"' in entry


def test_the_plan_file_makes_no_hip_call():
    text = open(os.path.join(CSRC, "twl_trim_plan.inc.hip")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()


def test_the_squeeze_kernels_are_untouched():
    """The trim kernels sit in a file of their own; the squeeze kernels' file carries no word of them."""
    assert "trim" not in open(os.path.join(CSRC, "backbone_kernels.hip.h")).read()
