"""The pure host decisions of the subtree profile (twilight_amd/csrc/twl_subtree_plan.inc.hip) against their known answers
(tests/subtree_plan_kats.cpp), compiled by g++ alone; the header, its binding and the built library name the same symbols.  No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")


def test_subtree_plan_known_answers(tmp_path):
    exe = tmp_path / "subtree_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "subtree_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == 21


def test_every_refusal_is_written_in_the_plan_file():
    """twl_subtree.inc.hip allocates, uploads and launches; what the call rejects is decided in the pure file alone."""
    host = open(os.path.join(CSRC, "twl_subtree.inc.hip")).read()
    plan = open(os.path.join(CSRC, "twl_subtree_plan.inc.hip")).read()
    for message in ("cache id in use", "sequence id out of range", "sequence id given twice", "the rows of the profile differ in length",
                    "the rows of the profile are empty"):
        assert message in plan and message not in host, message
    assert "hip" not in re.sub(r"//.*", "", plan).lower(), "the plan file makes no HIP call"


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_subtree_header_matches_binding():
    from twilight_amd import subtree

    assert _declared("twl_subtree.h") == ["twl_store_weighted_columns"]
    assert set(_declared("twl_subtree.h")) == set(subtree.exported_symbols())


def test_subtree_symbols_are_exported(built):
    import twilight_amd as twl

    lib = twl.load_library()
    for name in _declared("twl_subtree.h"):
        assert getattr(lib, name) is not None, name
    # the sources of the new call are part of the library's source stamp
    import __graft_entry__ as g

    for f in ("twl_subtree.inc.hip", "twl_subtree_plan.inc.hip", "subtree_kernels.hip.h"):
        assert f in g.KERNEL_SOURCES
