"""tests/place_cases.py -- directed inputs for the placement kernels (twilight_amd/csrc/place_kernels.hip.h): paths with insertion runs placed
on the edges of scan_path's tiles and thread chunks and of place_scan_kernel's rounds.  TEST INFRASTRUCTURE ONLY, plain numpy, no GPU.

The kernels' constants are restated here on purpose (a tile of 4096 codes, 16 codes per thread, scan rounds of 256 slots): classify() says
which branches a path reaches from the path alone, so a change of the product's constants shows as a spec that no longer reaches its branch
(tests/test_place_edge_inputs_cpu.py) and not as a test that quietly stops aiming at anything."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np

TILE = 4096          # kPlTile: codes per tile of scan_path
CHUNK = 16           # kPlItems: consecutive codes per thread
ROUND = 256          # kPlThreads: slots per round of place_scan_kernel, columns per workgroup of the colsrc / backbone kernels
NUC = list(b"ACGTNacgtn")
AA = list(b"ACDEFGHIKLMNPQRSTVWYXacdefghiklmnpqrstvwyx")


def make_path(L, runs, deletions=()):
    """A path over L backbone columns as int8: runs = {slot: length} puts an insertion run (code 1) of that length in front of column `slot`
    (slot L: after the last column); the columns in `deletions` get code 2, the others code 0."""
    ins = np.zeros(L + 1, dtype=np.int64)
    for k, n in runs.items():
        assert 0 <= k <= L and n >= 0
        ins[k] = n
    cols = np.zeros(L, dtype=np.int8)
    if len(deletions):
        cols[np.asarray(sorted(deletions), dtype=np.int64)] = 2
    path = np.ones(L + int(ins.sum()), dtype=np.int8)
    at = np.arange(L) + np.cumsum(ins)[:L]          # column c follows every run up to and including its own
    path[at] = cols
    return path


def make_seq(rng, path, letters=NUC) -> bytes:
    """As many letters (upper and lower case mixed) as the path has codes != 2."""
    return rng.choice(letters, int(np.count_nonzero(np.asarray(path) != 2))).astype(np.uint8).tobytes()


def runs_of(path):
    """(start, end) positions, both inclusive, of every maximal run of code 1."""
    one = np.concatenate([[0], (np.asarray(path) == 1).astype(np.int8), [0]])
    d = np.diff(one)
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


def classify(path, L) -> Dict[str, object]:
    """Which branches of scan_path this path reaches, from the path alone."""
    path = np.asarray(path)
    n = len(path)
    assert int(np.count_nonzero(path != 1)) == L
    tiles = (n + TILE - 1) // TILE
    runs = runs_of(path)

    def whole_tile(s, e):
        t = (s + TILE - 1) // TILE                  # first tile that starts inside the run
        return t < tiles and min(n, (t + 1) * TILE) - 1 <= e

    return {
        "tiles": tiles,
        "last_tile_codes": n - (tiles - 1) * TILE if n else 0,
        "run_ends_on_tile_end": any(e % TILE == TILE - 1 and e + 1 < n for s, e in runs),      # path[e + 1] is the next tile's first code
        "run_crosses_tile": any(s // TILE != e // TILE for s, e in runs),
        "run_covers_whole_tile": any(whole_tile(s, e) for s, e in runs),                        # the tile's own `last` stays -1
        "leading_run_crosses_tile": bool(runs) and runs[0][0] == 0 and runs[0][1] >= TILE,      # last = -1 carried over a tile
        "run_crosses_thread_chunk": any(s + (CHUNK - 1 - s % CHUNK) + 1 <= e for s, e in runs),
        "run_ends_path_on_tile_end": bool(runs) and runs[-1][1] == n - 1 and n % TILE == 0,     # p + 1 == n on a tile's last code
        "ends_in_run": n > 0 and path[-1] == 1,
    }


@dataclass
class Spec:
    name: str
    group: str                       # the specs of one group share a backbone and a placement
    L: int
    runs: Dict[int, int]
    deletions: Tuple[int, ...] = ()
    reach: Dict[str, object] = field(default_factory=dict)      # what classify() must say for this spec

    def path(self):
        return make_path(self.L, self.runs, self.deletions)


_LT = 4100      # group "tiles": two tiles, the second of 4 codes when nothing is inserted

PLACE_SPECS = [
    # ---- group tiles (the issue's eight, in its order) ----
    Spec("no_insertion", "tiles", _LT, {}, (5, 4095, 4096), dict(tiles=2, last_tile_codes=4, ends_in_run=False, run_crosses_tile=False)),
    Spec("run6_ends_tile0", "tiles", _LT, {4090: 6}, (), dict(tiles=2, run_ends_on_tile_end=True, run_crosses_tile=False, last_tile_codes=10)),
    Spec("run7_crosses_by_one", "tiles", _LT, {4090: 7}, (4090,), dict(tiles=2, run_crosses_tile=True, run_ends_on_tile_end=False, last_tile_codes=11)),
    Spec("run4096_leading", "tiles", _LT, {0: 4096}, (), dict(tiles=3, run_covers_whole_tile=True, leading_run_crosses_tile=False, run_ends_on_tile_end=True)),
    Spec("run5000_slot_L", "tiles", _LT, {_LT: 5000}, (_LT - 1,), dict(tiles=3, ends_in_run=True, run_crosses_tile=True, run_covers_whole_tile=True)),
    Spec("run9000_two_whole_tiles", "tiles", _LT, {10: 9000}, (), dict(tiles=4, run_covers_whole_tile=True, run_crosses_tile=True)),
    Spec("run1_every_even_column", "tiles", _LT, {k: 1 for k in range(0, _LT, 2)}, (), dict(tiles=2, run_crosses_thread_chunk=False, last_tile_codes=_LT + _LT // 2 - TILE)),
    Spec("empty_sequence", "tiles", _LT, {}, tuple(range(_LT)), dict(tiles=2, last_tile_codes=4)),
    # a leading run that goes on into tile 1: last = -1 is carried over a tile and used there
    Spec("run4100_leading", "tiles2", _LT, {0: 4100}, (0,), dict(tiles=3, leading_run_crosses_tile=True, run_covers_whole_tile=True)),
    Spec("run2_leading", "tiles2", _LT, {0: 2, 4093: 3}, (), dict(tiles=2, run_crosses_tile=True)),
    # ---- group chunks: runs on positions 14..17 of a thread's chunk, two sequences sharing slot 40 ----
    Spec("pos14_17", "chunks", 64, {14: 4}, (), dict(tiles=1, run_crosses_thread_chunk=True)),
    Spec("pos14_15", "chunks", 64, {14: 2}, (3,), dict(run_crosses_thread_chunk=False)),
    Spec("pos15_16", "chunks", 64, {15: 2}, (), dict(run_crosses_thread_chunk=True)),
    Spec("pos16_17", "chunks", 64, {16: 2}, (16,), dict(run_crosses_thread_chunk=False)),
    Spec("pos15", "chunks", 64, {15: 1, 64: 1}, (), dict(run_crosses_thread_chunk=False, ends_in_run=True)),
    Spec("slot40_run3", "chunks", 64, {40: 3}, (), dict(tiles=1)),
    Spec("slot40_run5", "chunks", 64, {40: 5}, (39, 40), dict(tiles=1, run_crosses_thread_chunk=False)),
    # ---- one placement each: a path of exactly 4095, 4096 (a run as its last codes) and 4097 codes ----
    Spec("len4095", "len4095", 4000, {2000: 95}, (1999,), dict(tiles=1, last_tile_codes=4095)),
    Spec("len4095_plain", "len4095", 4000, {}, (0, 3999), dict(tiles=1)),
    Spec("len4096", "len4096", 4000, {4000: 96}, (), dict(tiles=1, last_tile_codes=4096, ends_in_run=True, run_ends_path_on_tile_end=True)),
    Spec("len4096_plain", "len4096", 4000, {4000: 1}, (7,), dict(tiles=1)),
    Spec("len4097", "len4097", 4000, {0: 97}, (), dict(tiles=2, last_tile_codes=1, ends_in_run=False)),
    Spec("len4097_run_last", "len4097", 4000, {3990: 90, 4000: 7}, (), dict(tiles=2, last_tile_codes=1, ends_in_run=True, run_crosses_tile=True)),
]


def group(name):
    return [s for s in PLACE_SPECS if s.group == name]


def group_inputs(name, n_backbone=2, seed=0):
    """(backbone rows, sequences, paths) of one group of PLACE_SPECS; the backbone holds letters and '-' (no '.')."""
    specs = group(name)
    rng = np.random.default_rng(seed + len(name))
    L = specs[0].L
    backbone = [rng.choice(list(b"ACGTacgt-"), L).astype(np.uint8).tobytes() for _ in range(n_backbone)]
    paths = [s.path() for s in specs]
    seqs = [make_seq(rng, p) for p in paths]
    return backbone, seqs, paths


# ---- place_scan_kernel's rounds and the final width ----

def round_slots(L):
    """Slot 0, the last slot of every round of 256 and the first of the next, slot L."""
    s = {0, L}
    for k in range(ROUND, L + 1, ROUND):
        s |= {k - 1, k}
    return sorted(s)


# L -> (total insertion or None, length of one long run per sequence or 0)
ROUND_CASES = {1: (255, 0), 255: (2, 0), 256: (None, 0), 257: (None, 400), 511: (None, 0), 512: (None, 0), 513: (None, 0), 1024: (None, 0)}


def round_runs(L, n_seq=4):
    """runs dicts of n_seq sequences over L columns: every slot of round_slots(L) gets an insertion from two of them at least, of different
    lengths, so every scan round has a non-zero sum.  total: W - L is made exactly that; big: sequence s carries one run of big + s codes
    (not in slot L), which makes W exceed the pitch of a store that started at the pitch its sequences need."""
    total, big = ROUND_CASES[L]
    slots = round_slots(L)
    runs = [dict() for _ in range(n_seq)]
    for i, k in enumerate(slots):
        for s in range(n_seq):
            n = (i + 2 * s) % 4
            if total is not None:
                n = min(n, 1)
            if n:
                runs[s][k] = n
    for s in range(n_seq if big else 0):
        runs[s][slots[s % (len(slots) - 1)]] = big + s
    if total is not None:
        rest = sum(max(r.get(k, 0) for r in runs) for k in slots if k != 0)
        for r in runs:
            r.pop(0, None)
        assert total > rest
        runs[n_seq - 1][0] = total - rest
    return runs


def round_inputs(L, n_backbone=3, n_seq=4):
    """(backbone rows, sequences, paths, runs) of the scan-round case of L columns."""
    rng = np.random.default_rng(1000 + L)
    backbone = [rng.choice(list(b"ACGTacgt-"), L).astype(np.uint8).tobytes() for _ in range(n_backbone)]
    runs = round_runs(L, n_seq)
    paths = [make_path(L, r, tuple(range(s, L, 5)) if s % 2 else ()) for s, r in enumerate(runs)]
    seqs = [make_seq(rng, p) for p in paths]
    return backbone, seqs, paths, runs


def slot_max(L, runs_list):
    """The closed form of merge_insertions on make_path inputs: the longest run per slot."""
    out = np.zeros(L + 1, dtype=np.int64)
    for r in runs_list:
        for k, n in r.items():
            out[k] = max(out[k], n)
    return out
