"""The layout of the path blocks ranks exchange (twilight_amd/csrc/host/exchange_plan.hpp) and what the two block calls refuse before a launch
(check_block_rows, twilight_amd/csrc/twl_level_plan.inc.hip) against their known answers (tests/exchange_plan_kats.cpp), compiled by g++ alone;
and the restatement the GPU tests expect their blocks from (tests/exchange_cases.py) against a dump of the C++ functions on the same cases,
the levels and ownerships of tests/test_gpu_level_exchange.py among them.  No GPU needed."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exchange_cases as EC  # noqa: E402


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    exe = tmp_path_factory.mktemp("exchange_plan") / "exchange_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "exchange_plan_kats.cpp")])
    return str(exe)


def test_exchange_plan_known_answers(kats):
    r = subprocess.run([kats], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 42


def _level_layout_cases():
    """The ownerships of the GPU levels as layout cases: bound = both sides' columns, lengths made up below the bound (0 among them)."""
    out = []
    for lv in (EC.main_level("n"), EC.main_level("p", small=True)):
        bound = [len(p.case.sides[0].rows[0]) + len(p.case.sides[1].rows[0]) for p in lv.pairs]
        for own in lv.ownerships:
            lens = [0 if (i % 7 == 3 or not lv.takes_part[i]) else max(1, bound[i] - i % 5) for i in range(len(bound))]
            out.append(dict(name=f"{lv.seq_type}_{own.name}", world=own.world, owner=own.owner, takes=lv.takes_part, bound=bound, lens=lens,
                            errs=[(5 if n == 0 else 0) for n in lens]))
    return out


def test_restatement_equals_the_host_function(kats):
    cases = EC.layout_cases() + _level_layout_cases()
    r = subprocess.run([kats, "--dump"], input=EC.case_stdin(cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = [" ".join(l.split()) for l in r.stdout.splitlines()]
    want = [" ".join(l.split()) for c in cases for l in EC.dump_case(c)]
    assert len(got) == len(want) and len(want) >= 3 * len(cases)
    for g, w in zip(got, want):
        assert g == w, f"host: {g[:300]}\nrestatement: {w[:300]}"


def test_restatement_on_a_block_small_enough_to_read():
    """block_bytes itself: header, rows at their offsets, the fill byte in the pads and behind the last row; a descending rank."""
    pl = EC.plan([0, 1, 0, 1], [1, 1, 1, 1], [9, 3, 8, 2], 2, descending=(1,))
    assert pl.mine == [[0, 2], [3, 1]] and pl.hdr == [48, 48] and pl.block_max == 256
    off, end = EC.row_offsets(pl, 1, [2, 3])
    assert (off, end) == ([48, 56], 64)
    blk = EC.block_bytes(pl, 1, (1, 2, 0.0, 3), [2, 3], [0, 0], [[1, 2], [0, 0, 1]])
    assert len(blk) == 256 and blk[24:32] == bytes([3, 0, 0, 0, 0x44, 0x4C, 0x57, 0x54]) and blk[32:48] == bytes([2, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0])
    assert blk[48:64] == bytes([1, 2] + [0xEE] * 6 + [0, 0, 1] + [0xEE] * 5) and set(blk[64:]) == {0xEE}
