"""Known-answer tests of what a level call decides on the host (check_sides, plan_prepare, plan_align, check_commit, plan_commit) -- pure functions of
twilight_amd/csrc/twl_level_plan.inc.hip, compiled by g++ into a small program (tests/level_plan_kats.cpp); runs without a GPU and without the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_plans_known_answers(tmp_path):
    exe = tmp_path / "level_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "level_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 85
