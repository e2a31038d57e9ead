"""tests/keep_cases.py -- directed inputs for the kernels of the placement finish that keeps the backbone's length
(twilight_amd/csrc/keep_kernels.hip.h), beside those of tests/place_cases.py, which both kernels walk the same way.  TEST INFRASTRUCTURE
ONLY, plain numpy, no GPU.

The specs here aim at what keep_runs_kernel adds to scan_path: the rank of a run end, scanned over the 256 threads of a tile (16 codes
each) and carried over the tiles of 4096 codes.  classify_runs() says which of those branches a path reaches from the path alone
(tests/test_keep_oracle_cpu.py checks every spec against what it is listed for), with the kernels' constants restated in place_cases.

Also here: the small families the command-line tests run (tests/test_gpu_keep.py)."""
from __future__ import annotations

from typing import Dict

import numpy as np

import place_cases as PC

TILE, CHUNK, THREADS = PC.TILE, PC.CHUNK, PC.ROUND


def classify_runs(path) -> Dict[str, object]:
    """What the rank scan of keep_runs_kernel meets on this path."""
    path = np.asarray(path)
    ends = [e for _, e in PC.runs_of(path)]
    per_tile: Dict[int, int] = {}
    for e in ends:
        per_tile[e // TILE] = per_tile.get(e // TILE, 0) + 1
    return {
        "runs": len(ends),
        "letters": int(np.count_nonzero(path == 1)),
        "end_on_item_15": any(e % CHUNK == CHUNK - 1 for e in ends),            # the thread's last code: the code behind it is the next thread's
        "end_on_item_0": any(e % CHUNK == 0 and e > 0 for e in ends),           # ... and the run end that follows in the next thread's first code
        "more_ends_than_threads_in_a_tile": any(n > THREADS for n in per_tile.values()),
        "more_ends_than_a_tile_of_codes": len(ends) > TILE,                     # the rank carried over the tiles passes 4096
        "tiles_with_ends": len(per_tile),
        "end_on_tile_end": any(e % TILE == TILE - 1 and e + 1 < len(path) for e in ends),      # the code behind the tile decides
        "one_run_is_the_path": len(ends) == 1 and len(path) > 0 and bool((path == 1).all()),
    }


_S = PC.Spec

KEEP_SPECS = [
    # ---- group ranks16: run ends on the last code of a thread and on the first of another; a run that crosses into a thread's first code ----
    _S("ends_15_and_32", "ranks16", 64, {15: 1, 31: 1}, (), dict(runs=2, end_on_item_15=True, end_on_item_0=True)),
    _S("ends_16", "ranks16", 64, {15: 2}, (3,), dict(runs=1, end_on_item_15=False, end_on_item_0=True)),
    _S("ends_15_31_47", "ranks16", 64, {15: 1, 30: 1, 45: 1}, (), dict(runs=3, end_on_item_15=True, end_on_item_0=False)),
    _S("no_run", "ranks16", 64, {}, (0, 17, 63), dict(runs=0, letters=0)),
    # ---- more run ends than threads in one tile ----
    _S("runs257", "runs257", 600, {2 * k: 1 for k in range(257)}, (1, 599), dict(runs=257, letters=257, more_ends_than_threads_in_a_tile=True, tiles_with_ends=1)),
    _S("runs257_of_3", "runs257", 600, {2 * k + 1: 3 for k in range(257)}, (), dict(runs=257, letters=771, more_ends_than_threads_in_a_tile=True)),
    # ---- more run ends than one tile has codes: the carried rank passes 4096, in the fourth tile ----
    _S("runs4097", "runs4097", 8200, {2 * k: 1 for k in range(4097)}, (8199,), dict(runs=4097, more_ends_than_a_tile_of_codes=True, tiles_with_ends=4,
                                                                                    more_ends_than_threads_in_a_tile=True)),
    _S("run_ends_every_tile_end", "runs4097", 8200, {4095: 1, 8190: 1, 8200: 3}, (), dict(runs=3, end_on_tile_end=True, tiles_with_ends=3)),
    # ---- the path is one single run (L = 0: twl_place_create takes it): no code != 1 anywhere, last stays -1 over the tiles ----
    _S("one_run_37", "onerun", 0, {0: 37}, (), dict(runs=1, letters=37, one_run_is_the_path=True)),
    _S("one_run_5000", "onerun", 0, {0: 5000}, (), dict(runs=1, letters=5000, one_run_is_the_path=True, tiles_with_ends=1)),
]

GROUPS = ("ranks16", "runs257", "runs4097", "onerun")


def group(name):
    return [s for s in KEEP_SPECS if s.group == name]


def group_inputs(name, n_backbone=2, seed=0):
    """(backbone rows, sequences, paths) of one group of KEEP_SPECS; the backbone holds letters and '-' (no '.')."""
    specs = group(name)
    rng = np.random.default_rng(seed + 100 + len(name))
    L = specs[0].L
    backbone = [rng.choice(list(b"ACGTacgt-"), L).astype(np.uint8).tobytes() for _ in range(n_backbone)]
    paths = [s.path() for s in specs]
    seqs = [PC.make_seq(rng, p) for p in paths]
    return backbone, seqs, paths


# ---- families of the command-line tests ----

NUC = list(b"ACGT")
AA = list(b"ACDEFGHIKLMNPQRSTVWY")


def family(rng, letters, L, n_bb, n_new, *, gap_rate=0.04, gappy_cols=20, sub=0.05, ins=()):
    """A backbone of n_bb rows over one core (some columns almost all gaps, scattered gaps) and n_new new sequences: the core mutated, with the
    given (position, length) insertions of random letters, some of them in lower case (the case is kept).  Records (name, bytes)."""
    core = rng.choice(letters, L).astype(np.uint8)
    bb = []
    gcols = rng.choice(L, gappy_cols, replace=False) if gappy_cols else np.zeros(0, dtype=np.int64)
    for k in range(n_bb):
        r = core.copy()
        r[rng.random(L) < gap_rate] = ord("-")
        r[gcols] = ord("-")
        if k == 0:
            r[gcols] = core[gcols]
        bb.append((b"bb%d" % k, r.tobytes()))
    new = []
    for k in range(n_new):
        s = core.copy()
        m = rng.random(L) < sub
        s[m] = rng.choice(letters, int(m.sum()))
        s = bytearray(s.tobytes())
        for pos, ln in ins[k % len(ins)] if ins else ():
            piece = rng.choice(letters, ln).astype(np.uint8).tobytes()
            s[pos:pos] = piece.lower() if (pos + k) % 2 else piece
        new.append((b"new%d" % k, bytes(s)))
    return bb, new


def nucleotide_family():
    return family(np.random.default_rng(31), NUC, 900, 30, 12, ins=[[(0, 5)], [(300, 12), (600, 3)], [(900, 8)], []])


def protein_family():
    return family(np.random.default_rng(32), AA, 500, 20, 10, ins=[[(100, 6)], [], [(0, 2), (250, 9)]])


def chunk_family():
    return family(np.random.default_rng(36), NUC, 400, 12, 50, ins=[[(10, 3)], [(200, 7)], [], [(400, 2)]])


def filtered_family():
    """... with a low-quality sequence (not placed, not written) and an empty one (a row of '-')."""
    bb, new = family(np.random.default_rng(34), NUC, 600, 15, 6, ins=[[(200, 5)]])
    new.insert(2, (b"ambiguous", b"N" * 400 + new[0][1][:200]))
    new.insert(4, (b"empty", b""))
    return bb, new


def plain_family():
    """No insertion anywhere: every new sequence is the backbone's one core."""
    core = np.random.default_rng(35).choice(NUC, 800).astype(np.uint8).tobytes()
    return [(b"bb%d" % k, core) for k in range(10)], [(b"n%d" % k, core) for k in range(5)]
