"""The pure host decisions of placement (twilight_amd/csrc/twl_place_plan.inc.hip and the path source it shares with the merge,
twl_path_source.inc.hip) against their known answers (tests/place_plan_kats.cpp), compiled by g++ alone.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_place_plans_known_answers(tmp_path):
    exe = tmp_path / "place_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "place_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 63


def test_path_source_refusals_are_written_once():
    """-a and -f decode one convention: its messages exist in one file of the library."""
    csrc = os.path.join(ROOT, "twilight_amd", "csrc")
    for message in ("from_dp must be 0, 1 or 2", "from_dp 1 without a DP output of that length", "from_dp 2: twl_level_restore first, with this row pitch",
                    "host rows missing", "from_dp needs the prepared and aligned level of these pairs"):
        holders = [f for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f)) and message in open(os.path.join(csrc, f), errors="replace").read()]
        assert holders == ["twl_path_source.inc.hip"], (message, holders)
