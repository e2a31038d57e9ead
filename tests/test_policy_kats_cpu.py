"""Known-answer tests of the re-run ladder (next_rung), of the pass memory (PassMemory) and of a tile-parallel level's plan (plan_tile_level) -- pure functions of twilight_amd/csrc/twl_policy.inc.hip,
compiled by g++ into a small program (tests/policy_kats.cpp); runs without a GPU and without the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ladder_and_pass_memory_known_answers(tmp_path):
    exe = tmp_path / "policy_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "policy_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 78
