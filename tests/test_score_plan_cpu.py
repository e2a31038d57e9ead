"""The pure host decisions of the sum-of-pairs score (twilight_amd/csrc/twl_score_plan.inc.hip) against their known answers
(tests/score_plan_kats.cpp), compiled by g++ alone, plain and under the address and undefined-behaviour sanitizers; the terminal runs of the
plan against the oracle on every directed case; the ABI's symbol list, header against binding against library; the build lists; the kernels'
constants.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import score_cases as SC
import score_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")

MUST = ("rejects_null_store", "rejects_null_ids", "rejects_null_sub", "rejects_null_runs", "rejects_null_totals", "rejects_one_row", "rejects_2_20_rows_and_one",
        "rejects_id_8_of_8", "rejects_an_id_twice", "rejects_two_lengths", "rejects_a_prepared_level", "rejects_type_x", "rejects_no_column", "rejects_one_column_more",
        "rejects_totals_of_2_63", "accepts_totals_below_2_63", "one_past_each", "six_tile_pairs", "sub_rows_one_after_the_other", "a_row_without_letters", "one_end_each")


@pytest.mark.parametrize("flags", [("-O1",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_score_plans_known_answers(tmp_path, flags):
    exe = tmp_path / "score_plan_kats"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "score_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 40
    names = {l.split()[1] for l in lines}
    for must in MUST:
        assert must in names, must


TERMINALS_MAIN = r"""
#include <cstdio>
#include "%s"
int main()
{
    int n, W;
    while (scanf("%%d %%d", &n, &W) == 2) {
        std::vector<uint32_t> let((size_t)W);
        std::vector<int32_t> first((size_t)n), last((size_t)n);
        for (auto &v : let) if (scanf("%%u", &v) != 1) return 2;
        for (auto &v : first) if (scanf("%%d", &v) != 1) return 2;
        for (auto &v : last) if (scanf("%%d", &v) != 1) return 2;
        uint64_t RT = 0, GT = 0;
        score_terminals(n, W, let.data(), first.data(), last.data(), RT, GT);
        printf("%%llu %%llu\n", (unsigned long long)RT, (unsigned long long)GT);
    }
    return 0;
}
"""


def test_the_plans_terminal_runs_agree_with_the_walk(tmp_path):
    """score_terminals on let, first and last of every directed case (the walk where it is affordable, the column statement elsewhere)."""
    src = tmp_path / "terminals.cpp"
    src.write_text(TERMINALS_MAIN % os.path.join(CSRC, "twl_score_plan.inc.hip"))
    exe = tmp_path / "terminals"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    cases = SC.all_cases(16, 64, 512, 252)
    text, want = [], []
    for c in cases:
        p = SO.present(c.rows)
        n, W = p.shape
        first = [int(np.argmax(r)) if r.any() else W for r in p]
        last = [W - 1 - int(np.argmax(r[::-1])) if r.any() else -1 for r in p]
        text.append(" ".join(map(str, [n, W, *p.sum(axis=0).tolist(), *first, *last])))
        tot = SO.walk_all(c.rows)[1] if n <= 70 else SO.column_totals(c.rows)
        want.append(f"{tot['RT']} {tot['GT']}")
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:-1] == want


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_score_header_matches_binding():
    from twilight_amd import score

    assert set(_declared("twl_score.h")) == set(score.exported_symbols()) == {"twl_store_score_rows", "twl_store_score_timing", "twl_score_describe"}


def test_score_symbols_are_exported(built):
    import twilight_amd as twl

    lib = twl.load_library()
    for name in _declared("twl_score.h"):
        assert getattr(lib, name) is not None, name


def test_the_constants_need_no_device(built):
    """twl_score_describe answers before twl_init; the oracle's CPU tests and the directed cases stand on these values."""
    from twilight_amd import score

    S, T, R, F = score.describe()
    assert (S, T, R, F) == (16, 64, 512, 252)
    assert S % 2 == 0, "the staged pitch S + 1 is odd"
    assert 4 <= F <= 255 and F % 4 == 0 and R > F, "a byte counter is flushed before it wraps, and a slice is longer than a flush period"
    assert score.sub_index(4, 0, 0) == 0 and score.sub_index(4, 4, 4) == 14 and score.sub_index(20, 20, 20) == 230 and score.sub_index(4, 1, 1) == 5


def test_the_calls_refuse_null_arguments_before_any_device_work(built):
    import twilight_amd as twl
    from twilight_amd import score

    lib = score._lib()
    ids = (C.c_int32 * 2)(0, 1)
    out = (C.c_uint64 * 231)()
    for rc in (lib.twl_store_score_rows(None, C.c_int32(2), ids, C.c_char(b"n"), out, out, out), lib.twl_store_score_timing(None, None, None, None), lib.twl_score_describe(None)):
        with pytest.raises(twl.TwlError, match="bad argument"):
            twl.api._check(rc)


def test_the_new_files_are_kernel_sources_and_built():
    import __graft_entry__ as g

    for f in ("score_kernels.hip.h", "twl_score.inc.hip", "twl_score_plan.inc.hip"):
        assert f in g.KERNEL_SOURCES
        assert os.path.exists(os.path.join(CSRC, f))
    unit = open(os.path.join(CSRC, "twl_align.hip")).read()
    assert unit.index('#include "twl_score.inc.hip"') > unit.index('#include "twl_trim.inc.hip"') > unit.index('#include "twl_store.inc.hip"')
    assert '#include "score_kernels.hip.h"' in unit
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry.count('"twl_score.h"') == 2          # the library's and the host library's header lists
    assert '"score.cpp"' in entry and '"-DTWL_SCORE"' in entry


def test_the_plan_file_makes_no_hip_call():
    text = open(os.path.join(CSRC, "twl_score_plan.inc.hip")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()


def test_the_retree_kernels_are_untouched():
    """The score kernels sit in a file of their own; the retree kernels' file carries no word of them."""
    assert "score" not in open(os.path.join(CSRC, "retree_kernels.hip.h")).read()
