"""The directed placement inputs (tests/place_cases.py) reach the branches they are listed for, and tests/place_oracle.py, the reference of
tests/test_gpu_place_edges.py, obeys the closed forms that hold on such inputs.  No GPU needed."""
import numpy as np
import pytest

import place_cases as PC
import place_oracle as PO

GROUPS = sorted({s.group for s in PC.PLACE_SPECS})


@pytest.mark.parametrize("spec", PC.PLACE_SPECS, ids=lambda s: s.name)
def test_spec_reaches_its_branches(spec):
    got = PC.classify(spec.path(), spec.L)
    assert spec.reach, "a spec must name what it is for"
    assert {k: got[k] for k in spec.reach} == spec.reach


def test_every_branch_is_reached_by_some_spec():
    seen = [PC.classify(s.path(), s.L) for s in PC.PLACE_SPECS]
    for key in ("run_ends_on_tile_end", "run_crosses_tile", "run_covers_whole_tile", "leading_run_crosses_tile", "run_crosses_thread_chunk",
                "run_ends_path_on_tile_end", "ends_in_run"):
        assert any(c[key] for c in seen) and not all(c[key] for c in seen), key
    assert {4095, 4096, 4097} <= {len(s.path()) for s in PC.PLACE_SPECS}
    assert {c["tiles"] for c in seen} >= {1, 2, 3, 4}
    assert {1, 4, 4095, 4096} <= {c["last_tile_codes"] for c in seen}


def test_make_path_and_make_seq():
    p = PC.make_path(4, {0: 2, 2: 1, 4: 3}, (1,))
    assert p.dtype == np.int8 and p.tolist() == [1, 1, 0, 2, 1, 0, 0, 1, 1, 1]
    s = PC.make_seq(np.random.default_rng(0), p)
    assert len(s) == 9 and s != s.upper() and s != s.lower()
    assert PC.runs_of(p) == [(0, 1), (4, 4), (7, 9)]


def _closed_forms(backbone, seqs, paths, runs_list):
    L = len(backbone[0])
    longest = PO.merge_insertions(L, paths)
    assert np.array_equal(longest, PC.slot_max(L, runs_list))
    W = L + int(longest.sum())
    ins = np.arange(L + 1) + np.concatenate([[0], np.cumsum(longest)[:-1]])
    for r in backbone:
        out = PO.expand_backbone(r, longest)
        assert len(out) == W and out.replace(b".", b"") == r
    for s, p, runs in zip(seqs, paths, runs_list):
        row = PO.expand_placed(s, p, longest)
        assert len(row) == W and row.replace(b".", b"").replace(b"-", b"") == s
        letters_before = np.concatenate([[0], np.cumsum(p != 2)])
        starts = [a for a, _ in PC.runs_of(p)]          # one run per non-empty slot, in slot order: a column lies between two slots
        assert len(starts) == len([n for n in runs.values() if n])
        for (k, n), st in zip(sorted((k, n) for k, n in runs.items() if n), starts):
            q = int(letters_before[st])
            assert row[ins[k]: ins[k] + n] == s[q: q + n], f"slot {k}: the run's letters, left-aligned"
            assert row[ins[k] + n: ins[k] + int(longest[k])] == b"." * (int(longest[k]) - n), f"slot {k}: padding"
    return longest, W


@pytest.mark.parametrize("name", GROUPS)
def test_oracle_closed_forms_on_spec_groups(name):
    backbone, seqs, paths = PC.group_inputs(name)
    longest, W = _closed_forms(backbone, seqs, paths, [s.runs for s in PC.group(name)])
    if name == "tiles":
        assert W == 24250
    if name == "chunks":
        assert longest[40] == 5      # runs of 3 and 5 share the slot: the shorter one is padded (checked above)


@pytest.mark.parametrize("L", sorted(PC.ROUND_CASES))
def test_scan_round_cases(L):
    backbone, seqs, paths, runs = PC.round_inputs(L)
    longest, W = _closed_forms(backbone, seqs, paths, runs)
    for k in PC.round_slots(L):
        assert longest[k] > 0
    for base in range(0, L + 1, PC.ROUND):
        assert longest[base: base + PC.ROUND].sum() > 0, "a round without insertions: the carry would not matter"
    total, big = PC.ROUND_CASES[L]
    if total is not None:
        assert W == L + total
    if big:
        pitch = (max(len(x) for x in backbone + seqs) + 1 + 255) // 256 * 256      # the least pitch the store can start with
        assert W + 1 > pitch and W > 2 * L + 256 and longest[L] < W // 4
    assert {PC.ROUND_CASES[1][0] + 1, PC.ROUND_CASES[255][0] + 255} == {256, 257}
