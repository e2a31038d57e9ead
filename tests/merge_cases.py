"""tests/merge_cases.py -- directed inputs for the merge of alignments (twilight_amd/csrc/merge_kernels.hip.h, twl_merge.inc.hip,
twl_path_source.inc.hip): families whose merges run from the level's own buffers, rows on both planes of the store, and host paths placed
on the edges of the merge kernels.  TEST INFRASTRUCTURE ONLY, plain numpy, no GPU.

The kernels' constants are restated here on purpose (256 threads, waves of 64, tiles of 4096 codes, 16 rows and 16 columns per thread of
the rewrite, a row pitch that is a multiple of 256): tests/test_merge_edge_inputs_cpu.py holds every case to what it is listed for, so a
case that was edited away from its edge fails there and does not quietly stop aiming at anything.

(A) FAMILIES / RUNS: the levels of tests/test_gpu_merge_edges.py as host/merge.cpp's mergeProfileLevel drives them.  The expected final path
of every pair is tests/golden/merge_edge_paths.json: merge_oracle.merge_pair over the families below, run length encoded.  The CPU file
recomputes all of them (oracle_paths) and compares, so the GPU file reads the JSON and runs no DP oracle.
(B) plane_case: rows on both planes of the store, and a finish that has to re-pitch the planes.
(C) rank_case, three_pairs_case, column_tile_case, rewrite_width_case, lone_column_case: host paths."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

import merge_oracle as MO

LO, PO, F = MO.LO, MO.PO, MO.F

THREADS, WAVE, TILE = 256, 64, 4096      # kPlThreads, the wave of the rank kernel's ballot, kPlTile
ROWS_PER_WG, COLS = 16, 16               # kMgRows, kMgCols
PITCH_UNIT = 256                         # grow_rows rounds the row pitch up to a multiple of this
ALPHABET = list(b"ACGTacgtNn-.")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_edge_paths.json")


# ---- (A) families ----

@dataclass
class GroupSpec:
    rows: int
    start: int               # the group's rows are variants of ancestor[start:stop]
    stop: int
    empty: Tuple[int, ...]   # columns that hold '-' in every row: removed at -r 0.95, kept at -r 1
    cut: Tuple[int, int] = (0, 0)      # (position, letters) taken out of the slice
    add: Tuple[int, int] = (0, 0)      # (position, letters) of the group's own put in, after the cut

    @property
    def len(self):
        return self.stop - self.start - self.cut[1] + self.add[1]


@dataclass
class Family:
    seq_type: str
    seed: int
    groups: List[GroupSpec]
    levels: List[List[Tuple[int, int]]]      # per level its pairs (reference node, query node); a node is named by its lowest group


# Lengths differ between the pairs of a level, so the level's seq_len and the pitch refLen + qryLen exceed most pairs' own lengths.
FAMILIES: Dict[str, Family] = {
    "nuc6": Family("n", 601, [GroupSpec(5, 0, 300, (0, 50, 51, 52, 120, 299), (80, 9), (200, 9)), GroupSpec(9, 10, 330, (7, 200, 201), (150, 12), (40, 12)),
                              GroupSpec(3, 60, 210, (30, 31), (100, 5), (20, 5)), GroupSpec(4, 50, 220, (), (60, 7), (120, 7)),
                              GroupSpec(7, 100, 330, (), (30, 11), (180, 11)), GroupSpec(6, 90, 295, (100, 204), (150, 6), (60, 6))],
                   [[(0, 1), (2, 3), (4, 5)], [(0, 2)], [(0, 4)]]),
    "prot4": Family("p", 402, [GroupSpec(4, 0, 260, (3, 90, 91), (120, 8), (40, 8)), GroupSpec(7, 30, 245, (), (50, 6), (160, 6)),
                               GroupSpec(5, 70, 250, (10,), (90, 4), (30, 4)), GroupSpec(3, 10, 250, (100, 101, 102), (200, 10), (60, 10))],
                    [[(0, 1), (2, 3)], [(0, 2)]]),
}


def family_rows(name: str) -> List[List[bytes]]:
    """The rows of every group: a slice of one ancestor less a cut, with letters of the group's own put in, with point changes (8 %), gaps
    (4 %), lowercase letters (3 %) and the group's all-gap columns."""
    fam = FAMILIES[name]
    rng = np.random.default_rng(fam.seed)
    letters = list(b"ACGT") if fam.seq_type == "n" else list(b"ACDEFGHIKLMNPQRSTVWY")
    anc = rng.choice(letters, 340).astype(np.uint8)
    out = []
    for g in fam.groups:
        base = anc[g.start: g.stop]
        base = np.concatenate([base[: g.cut[0]], base[g.cut[0] + g.cut[1]:]])
        base = np.concatenate([base[: g.add[0]], rng.choice(letters, g.add[1]).astype(np.uint8), base[g.add[0]:]])
        rows = []
        for _ in range(g.rows):
            r = base.copy()
            hit = rng.random(len(r)) < 0.08
            r[hit] = rng.choice(letters, int(hit.sum())).astype(np.uint8)
            gap = rng.random(len(r)) < 0.04
            r[gap] = ord("-")
            low = (rng.random(len(r)) < 0.03) & ~gap
            r[low] |= 0x20
            r[list(g.empty)] = ord("-")
            rows.append(r.tobytes())
        out.append(rows)
    return out


def matrix_of(seq_type):
    from twilight_amd import synth

    return synth.nucleotide_matrix() if seq_type == "n" else synth.protein_matrix()


@dataclass
class OraclePair:
    path: np.ndarray            # merge_oracle.merge_pair's final path
    retries: int                # DP runs that ended with an error before the one that passed
    lens: Tuple[int, int]       # the sides' lengths before the merge
    runs: Tuple[list, list]     # the (start, length) runs of columns each side loses at this threshold


def oracle_paths(name: str, thr: float) -> Dict[Tuple[int, int], OraclePair]:
    """Every pair of the family's schedule through merge_oracle.merge_pair and level_oracle.update_frequency, level by level."""
    fam = FAMILIES[name]
    rows = family_rows(name)
    M = matrix_of(fam.seq_type)
    freq = {k: PO.backbone_profile(r, fam.seq_type) for k, r in enumerate(rows)}
    num = {k: len(r) for k, r in enumerate(rows)}
    weight = {k: F(len(r)) for k, r in enumerate(rows)}
    out = {}
    for level in fam.levels:
        for r, q in level:
            retries = []
            path = MO.merge_pair(freq[r], num[r], weight[r], freq[q], num[q], weight[q], fam.seq_type, M, thr=thr, log=lambda x, f: retries.append((x, f)))
            runs = tuple(LO.prepare_side(LO.profile_from_cache(freq[k], weight[k], num[k]), num[k], thr, -50.0, -5.0, fam.seq_type)[2] if thr != 1.0 else []
                         for k in (r, q))
            out[(r, q)] = OraclePair(path, len(retries), (freq[r].shape[0], freq[q].shape[0]), runs)
            freq[r] = LO.update_frequency(freq[r], freq[q], path, weight[r], weight[q])
            num[r], weight[r] = num[r] + num[q], F(weight[r] + weight[q])
            del freq[q]
    return out


def rle(path) -> str:
    p = np.asarray(path, dtype=np.int8)
    cut = np.flatnonzero(np.diff(p)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(p)]])
    return " ".join(f"{int(p[s])}x{int(e - s)}" for s, e in zip(starts, ends))


def unrle(text: str) -> np.ndarray:
    parts = [t.split("x") for t in text.split()]
    return np.concatenate([np.full(int(n), int(c), dtype=np.int8) for c, n in parts]) if parts else np.zeros(0, np.int8)


def golden_key(name: str, thr: float) -> str:
    return f"{name}@{thr:g}"


def golden_paths(name: str, thr: float) -> Dict[Tuple[int, int], np.ndarray]:
    """The committed final paths of the family at this threshold, keyed like oracle_paths."""
    with open(GOLDEN) as f:
        data = json.load(f)[golden_key(name, thr)]
    return {tuple(int(x) for x in k.split("+")): unrle(v) for k, v in data.items()}


GOLDEN_KEYS = (("nuc6", 1.0), ("nuc6", 0.95), ("prot4", 1.0))


@dataclass
class LevelStep:
    pairs: List[Tuple[int, int]]
    restore: List[int]                    # indices into `pairs` handed to twl_level_restore before the apply
    source: List[Optional[int]]           # per pair: from_dp 1 / 2, 0 = downloaded and handed back as a host row, None = skipped (path_len 0)


@dataclass
class Run:
    family: str
    thr: float
    steps: List[LevelStep]


def _steps(fam, first: LevelStep, later_source: List[int], extra: Optional[LevelStep] = None) -> List[LevelStep]:
    out = [first] + ([extra] if extra else [])
    for level, src in zip(FAMILIES[fam].levels[1:], later_source):
        out.append(LevelStep(level, [i for i in range(len(level)) if src == 2], [src] * len(level)))
    return out


_N6 = FAMILIES["nuc6"].levels[0]
# A skipped pair is committed with path_len 0 (include/twl_level.h: "path_len[i] == 0 leaves pair i untouched (deferred pair)"), and the commit
# ends the level: the pair's DP output is gone with it.  So the skipped pair is PREPARED AGAIN, as a level of its own, and applied there.
RUNS: Dict[str, Run] = {
    "thr1_dp_output": Run("prot4", 1.0, _steps("prot4", LevelStep(FAMILIES["prot4"].levels[0], [], [1, 1]), [1])),
    "thr1_dp_output_and_path_buffer": Run("nuc6", 1.0, _steps("nuc6", LevelStep(_N6, [0, 2], [2, 1, 2]), [1, 2])),
    "thr095_path_buffer": Run("nuc6", 0.95, _steps("nuc6", LevelStep(_N6, [0, 1, 2], [2, 2, 2]), [2, 2])),
    "skipped_middle_pair": Run("nuc6", 1.0, _steps("nuc6", LevelStep(_N6, [2], [1, None, 2]), [2, 1], extra=LevelStep([_N6[1]], [], [1]))),
    "host_row_among_level_rows": Run("nuc6", 1.0, _steps("nuc6", LevelStep(_N6, [0], [2, 0, 1]), [1, 1])),
}


def level_pitches(lens: Dict[int, int], pairs) -> Tuple[int, int, int]:
    """(seq_len, the DP output's row pitch 2 * seq_len, the path buffer's pitch max(refLen + qryLen)) of a level, as mergeProfileLevel sets them."""
    seq_len = max(max(lens[r], lens[q]) for r, q in pairs)
    return seq_len, 2 * seq_len, max(lens[r] + lens[q] for r, q in pairs)


# ---- host paths ----

def random_rows(rng, n, L, alphabet=ALPHABET) -> List[bytes]:
    return [rng.choice(alphabet, L).astype(np.uint8).tobytes() for _ in range(n)]


def mixed_path(rng, wr, wq, n0, lead1=0, tail2=0):
    """A path with exactly wr codes != 1 and wq codes != 2, n0 of them code 0: lead1 codes 1 first, tail2 codes 2 last, the rest shuffled."""
    n1, n2 = wq - n0 - lead1, wr - n0 - tail2
    assert n1 >= 0 and n2 >= 0
    mid = np.array([0] * n0 + [1] * n1 + [2] * n2, dtype=np.int8)
    rng.shuffle(mid)
    return np.concatenate([np.ones(lead1, np.int8), mid, np.full(tail2, 2, np.int8)])


@dataclass
class MergeCase:
    """Groups of rows and the calls of a merge with host paths: per call (ref_groups, qry_groups, paths)."""
    name: str
    files: List[List[bytes]]
    calls: List[Tuple[list, list, list]]
    W: int
    note: dict = field(default_factory=dict)


# ---- (C) merge_ranks_kernel: one exceptional code on a lane, wave, round or tile edge ----

RANK_LEN = TILE + 304                                            # a whole tile and a partial one whose last round is partial as well
RANK_INDICES = (0, WAVE - 1, WAVE, THREADS - 1, THREADS, TILE - 1, TILE, RANK_LEN - 1)


def rank_case(code: int, at: int) -> MergeCase:
    """A path of RANK_LEN codes 0 but for one code `code` (1 or 2) at position `at`: wr + wq - n0 = RANK_LEN with n0 = RANK_LEN - 1."""
    assert code in (1, 2) and 0 <= at < RANK_LEN
    rng = np.random.default_rng(1000 * code + at)
    path = np.zeros(RANK_LEN, np.int8)
    path[at] = code
    wr, wq = RANK_LEN - (code == 1), RANK_LEN - (code == 2)
    return MergeCase(f"code{code}_at{at}", [random_rows(rng, 2, wr), random_rows(rng, 1, wq)], [([[0]], [[1]], [path])], RANK_LEN, {"code": code, "at": at})


def round_case(n: int) -> MergeCase:
    """A shuffled path of exactly n codes (256: one whole round, 257: a round and one code)."""
    rng = np.random.default_rng(n)
    wr, wq = n - 60, n - 45
    return MergeCase(f"len{n}", [random_rows(rng, 2, wr), random_rows(rng, 2, wq)], [([[0]], [[1]], [mixed_path(rng, wr, wq, wr + wq - n)])], n)


# ---- (C) three pairs of very different sizes in one call ----

def three_pairs_case() -> MergeCase:
    """Ten groups.  Call 1 merges inside the sides (four pairs), call 2 is the call under test: pairs of 300, 5000 and 40 codes in that
    order, with sides of {0,1}/{2}, {3}/{4,5} and {6,7}/{8,9} -- every two-group side has been composed once, the rank tables start at
    0, 180, 380, 3280, 5880, 5904 ints, and the compose table has ten jobs.  Calls 3 and 4 bring everything to one width."""
    rng = np.random.default_rng(333)
    L = [150, 140, 200, 2900, 2000, 2100, 20, 18, 15, 17]
    files = [random_rows(rng, 1 + k % 2, l) for k, l in enumerate(L)]
    c1 = ([[0], [4], [6], [8]], [[1], [5], [7], [9]],
          [mixed_path(rng, 150, 140, 110), mixed_path(rng, 2000, 2100, 1500), mixed_path(rng, 20, 18, 14), mixed_path(rng, 15, 17, 10)])
    c2 = ([[0, 1], [3], [6, 7]], [[2], [4, 5], [8, 9]],
          [mixed_path(rng, 180, 200, 80), mixed_path(rng, 2900, 2600, 500, lead1=3), mixed_path(rng, 24, 22, 6, tail2=2)])
    c3 = ([[3, 4, 5]], [[0, 1, 2]], [mixed_path(rng, 5000, 300, 250)])
    c4 = ([[6, 7, 8, 9]], [[0, 1, 2, 3, 4, 5]], [mixed_path(rng, 40, 5050, 30)])
    return MergeCase("three_pairs", files, [c1, c2, c3, c4], 5060, {"sizes": [300, 5000, 40], "rank_off": [0, 180, 380, 3280, 5880, 5904]})


# ---- (C) merge_iota / merge_compose / merge_inverse: grid.y = ceil(maxL / 256) ----

COLUMN_TILE_LENS = (257, 1, 513, 255, 256)


def column_tile_case() -> MergeCase:
    """Groups of 1, 255, 256, 257 and 513 columns merged as a star over four levels: every launch has grid.y = 3 and groups that end
    inside the first, on the edge of the first, just inside the second and just inside the third block of 256 columns."""
    rng = np.random.default_rng(513)
    files = [random_rows(rng, 2, l) for l in COLUMN_TILE_LENS]
    calls, w, under = [], COLUMN_TILE_LENS[0], [0]
    for k in range(1, len(files)):
        n0 = min(w, COLUMN_TILE_LENS[k]) * 2 // 3
        calls.append(([list(under)], [[k]], [mixed_path(rng, w, COLUMN_TILE_LENS[k], n0, lead1=int(k == 2), tail2=int(k == 3))]))
        w += COLUMN_TILE_LENS[k] - n0
        under.append(k)
    return MergeCase("column_tiles", files, calls, w)


# ---- (C) merge_rewrite_kernel: the last, partial chunk of 16 columns ----

REWRITE_WIDTHS = (16, 48, 49, 63, 303, 304, 305)      # W % 16 = 0, 1, 15 below 64 and near 300, and one chunk exactly


def rewrite_width_case(W: int) -> MergeCase:
    rng = np.random.default_rng(W)
    L0, L1 = 2 * W // 3, W // 2
    n0 = L0 + L1 - W
    return MergeCase(f"W{W}", [random_rows(rng, ROWS_PER_WG + 1, L0), random_rows(rng, 2, L1)], [([[0]], [[1]], [mixed_path(rng, L0, L1, n0)])], W)


def lone_column_case() -> MergeCase:
    """A group of ONE column in the middle of 400: every other entry of its inverse map is -1."""
    rng = np.random.default_rng(400)
    path = np.concatenate([np.full(200, 2, np.int8), np.ones(1, np.int8), np.full(199, 2, np.int8)])
    return MergeCase("lone_column", [random_rows(rng, 3, 399), random_rows(rng, ROWS_PER_WG + 1, 1, alphabet=list(b"ACGTacgt"))], [([[0]], [[1]], [path])], 400, {"at": 200})


# ---- (B) rows on both planes ----

PLANE_LENS = (100, 120, 140)               # columns of the three groups
PLANE_EXTRA_LEN = 90                       # two rows that are in no group: one per plane
PLANE_WIDTHS = {"within_the_pitch": 255, "beyond_the_pitch": 256}


def least_pitch(max_len: int) -> int:
    """The row pitch of a store that starts at the pitch its rows need (twl_store_create through grow_rows when the generous allocation
    fails): need = max_len + 1 bytes, rounded up to PITCH_UNIT.  twl_merge_finish asks grow_rows for W + 1 bytes, so the planes are
    reallocated when W + 1 > pitch: the smallest such W is the pitch itself."""
    return (max_len + 1 + PITCH_UNIT - 1) // PITCH_UNIT * PITCH_UNIT


@dataclass
class PlaneCase:
    name: str
    groups: List[List[int]]       # store ids of the three groups
    extra: List[int]              # store ids of the rows outside the merge
    plane: List[int]              # per store id: the plane its live row sits on when the merge finishes
    stale: List[bytes]            # per store id: what the other plane holds
    live: List[bytes]             # per store id: the row
    calls: List[Tuple[list, list, list]]
    W: int


def plane_case(name: str) -> PlaneCase:
    """Group 0 (3 rows) wholly on plane 1, group 1 (4 rows) wholly on plane 0, group 2 (2 * 16 + 5 rows) alternating, so each of its three
    slices of the rewrite (the partial last one included) reads both planes; the two other rows sit on plane 0 and plane 1.  The stale copy
    of every row differs from the live one at every column."""
    W = PLANE_WIDTHS[name]
    rng = np.random.default_rng(77)
    sizes = (3, 4, 2 * ROWS_PER_WG + 5)
    groups, plane, lens, at = [], [], [], 0
    for k, n in enumerate(sizes):
        groups.append(list(range(at, at + n)))
        plane += [1] * n if k == 0 else [0] * n if k == 1 else [(j + 1) % 2 for j in range(n)]
        lens += [PLANE_LENS[k]] * n
        at += n
    extra = [at, at + 1]
    plane += [0, 1]
    lens += [PLANE_EXTRA_LEN] * 2
    live = [rng.choice(ALPHABET, l).astype(np.uint8) for l in lens]
    stale = []
    for v in live:                                        # another letter of the alphabet at every column
        shift = rng.integers(1, len(ALPHABET), len(v))
        idx = np.array([ALPHABET.index(int(c)) for c in v])
        stale.append(np.array(ALPHABET, dtype=np.uint8)[(idx + shift) % len(ALPHABET)].tobytes())
    live = [v.tobytes() for v in live]
    w01 = PLANE_LENS[2]
    n0a = PLANE_LENS[0] + PLANE_LENS[1] - w01
    n0b = w01 + PLANE_LENS[2] - W
    calls = [([[0]], [[1]], [mixed_path(rng, PLANE_LENS[0], PLANE_LENS[1], n0a)]), ([[0, 1]], [[2]], [mixed_path(rng, w01, PLANE_LENS[2], n0b, lead1=1)])]
    return PlaneCase(name, groups, extra, plane, stale, live, calls, W)
