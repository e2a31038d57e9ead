"""Placement without a tree (-a, include/twl_place.h) on the CPU: the oracle's merge of insertions on hand-derived cases, the ABI's symbol
list, the command line's refusals.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import place_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _merge(backbone, new):
    """Items 6-7 of the contract on given paths: (longest, output rows)."""
    L = len(backbone[0])
    paths = [np.asarray(p, dtype=np.int8) for _, p in new]
    longest = PO.merge_insertions(L, paths)
    rows = [PO.expand_backbone(r, longest) for r in backbone] + [PO.expand_placed(s, p, longest) for (s, _), p in zip(new, paths)]
    return longest, rows


def test_hand_derived_example():
    backbone = [b"AC-G", b"A-TG"]
    new = [(b"AXYCTG", [0, 1, 1, 0, 0, 0]), (b"ZACTG", [1, 0, 0, 0, 0]), (b"ACG", [0, 0, 2, 0]), (b"ACTGWW", [0, 0, 0, 0, 1, 1])]
    longest, rows = _merge(backbone, new)
    assert longest.tolist() == [1, 2, 0, 0, 2]
    assert len(backbone[0]) + int(longest.sum()) == 9
    assert rows == [b".A..C-G..", b".A..-TG..", b".AXYCTG..", b"ZA..CTG..", b".A..C-G..", b".A..CTGWW"]


def test_no_insertion_is_identity():
    backbone = [b"ac-gT", b"A-tgT", b"-----"]
    new = [(b"ACGT", [0, 0, 2, 0, 0]), (b"", [2, 2, 2, 2, 2]), (b"acgtt", [0, 0, 0, 0, 0])]
    longest, rows = _merge(backbone, new)
    assert not longest.any()
    assert rows[:3] == backbone
    assert rows[3:] == [b"AC-GT", b"-----", b"acgtt"]


def test_insertions_at_slot_zero_and_slot_L():
    backbone = [b"ACG"]
    new = [(b"xxACG", [1, 1, 0, 0, 0]), (b"ACGyyy", [0, 0, 0, 1, 1, 1]), (b"zACGw", [1, 0, 0, 0, 1])]
    longest, rows = _merge(backbone, new)
    assert longest.tolist() == [2, 0, 0, 3]
    assert rows == [b"..ACG...", b"xxACG...", b"..ACGyyy", b"z.ACGw.."]
    for r in rows:
        assert len(r) == 8


def test_oracle_end_to_end_invariants():
    """place() on a small family: all rows one width; the backbone comes back when the placed rows and the all-'.' columns go; every placed
    row without '-' and '.' is its input; low-quality sequences are absent."""
    rng = np.random.default_rng(5)
    core = rng.choice(list(b"ACGT"), 120).astype(np.uint8).tobytes()
    backbone = [(b"b%d" % k, bytes(c if rng.random() > 0.05 else ord("-") for c in core)) for k in range(6)]
    new = []
    for k in range(5):
        s = bytearray(core)
        at = int(rng.integers(0, len(s)))
        s[at:at] = rng.choice(list(b"ACGT"), int(rng.integers(1, 6))).astype(np.uint8).tobytes()
        new.append((b"n%d" % k, bytes(s)))
    new.append((b"bad", b"N" * 60 + core[:60]))
    out, longest, _ = PO.place(backbone, new)
    names = [n for n, _ in out]
    assert b"bad" not in names and len(out) == 6 + 5
    W = len(out[0][1])
    assert W == len(core) + int(longest.sum()) and all(len(r) == W for _, r in out)
    keep = [j for j in range(W) if not all(r[j] == ord(".") for _, r in out[:6])]
    for (_, r), (_, b) in zip(out[:6], backbone):
        assert bytes(r[j] for j in keep) == b
    for (_, r), (_, s) in zip(out[6:], new[:5]):
        assert r.replace(b"-", b"").replace(b".", b"") == s


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_place_header_matches_binding():
    from twilight_amd import place

    assert set(_declared("twl_place.h")) == set(place.exported_symbols())


def test_place_symbols_are_exported(built):
    import twilight_amd as twl
    from twilight_amd import place

    lib = twl.load_library()
    for name in _declared("twl_place.h"):
        assert getattr(lib, name) is not None, name


def _cli(*args, timeout=60):
    exe = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def test_cli_refuses_placement_with_a_tree(built, tmp_path):
    r = _cli("-a", "x.aln", "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"))
    assert r.returncode == 1 and "not supported yet" in r.stderr


def test_cli_refuses_host_staged_and_several_gpus_in_placement(built, tmp_path):
    r = _cli("-a", "x.aln", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--host-staged")
    assert r.returncode == 1 and "--host-staged" in r.stderr
    r = _cli("-a", "x.aln", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--gpu-index", "0,1")
    assert r.returncode == 1 and "one GPU" in r.stderr


def test_checker_binaries_keep_refusing_a(built):
    """The CPU-check build of the same main.cpp carries no placement: -a stays an unsupported option there."""
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = subprocess.run([exe, "-a", "x.aln", "-i", "x.fa", "-o", "o.aln"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option -a" in r.stderr
