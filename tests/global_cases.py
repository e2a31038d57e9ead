"""Directed cases for the global-memory DP kernel (twilight_amd/csrc/talco_global.hip.h), the last rung of the re-run ladder.

The kernel is one workgroup of T = 1024 threads per pair.  Its cell loop, its convergence scan and its row re-initialisation each stride
by T; it is persistent (a workgroup pulls pairs from a queue until the queue is empty, and keeps its scratch from pair to pair); and
its scratch is sized by the call (`rowcap = min(flen, seq_len) + 2`), released by run_device when a call left it above 256 MiB.  The
cases below stand on those switch points:

A  ROUND_CASES   the widest band is exactly Q rows, Q on either side of one, two and three thread rounds, with flen above, at and one
                 below Q.  With an X-drop that never prunes the band of tile 0 grows by a row per diagonal to the whole shorter side.
B  CONV_CASES    tiles that end by convergence while the band is still wider than one round (the scan fills s_conv in several passes
                 of a thread), and one pair that converges after the band has fallen back below a round.
C  queue_pool    24 live pairs and two with an empty side, replicated by the GPU test to more pairs than the device has CUs, so that
                 every workgroup takes a second pair; four parameter sets, two of them chosen so that failed pairs (errorType 2, 1)
                 and good ones share a workgroup's queue; a protein pool; and marker 64 on twice the level, the one call whose second
                 pairs run past their marker (see QUEUE_CALLS).
D  scratch_*     a level whose scratch is above the release threshold and one far below it.

Every figure next to a case is the CPU oracle's (oracle_lib.align_pair with the trace hook, which reports the band [L, U] of each
diagonal it computes: see dp_cases).  tests/test_global_edge_inputs_cpu.py recomputes them; tests/test_gpu_global_edges.py runs the cases."""
from __future__ import annotations

import os
import sys
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
from dp_cases import matrix_of, replicate  # noqa: E402,F401
from twilight_amd import synth  # noqa: E402

T = 1024                                 # threads of the kernel's one workgroup per pair: the stride of its three loops
RELEASE_BYTES = 256 << 20                # run_device hands the scratch back after a call that left it above this


# ---- the oracle, pair by pair ----
@dataclass
class TileTrace:
    """One tile in the oracle's trace: its widest diagonal, and the number and width of the last diagonal it computed."""
    max_width: int = 0
    last_k: int = -1
    last_width: int = 0


@dataclass
class PairOracle:
    path: np.ndarray
    err: int
    cells: int
    n_tiles: int                         # the oracle's own count (Stats.tiles)
    max_width: int                       # the oracle's own figure (Stats.max_width)
    tiles: List[TileTrace] = field(default_factory=list)


def oracle_pair(batch, i: int, trace: bool = True, **pk) -> PairOracle:
    """Pair `i` of `batch` through oracle_lib.align_pair, with the trace hook (`tiles`) unless told otherwise (a call of the interpreter per diagonal)."""
    R, Q, P = int(batch.len[i, 0]), int(batch.len[i, 1]), batch.P
    if R <= 0 or Q <= 0:      # (as twlo_align_batch has it: length 0, errorType 0, the caller fills the all-gap path)
        return PairOracle(path=np.zeros(0, dtype=np.int8), err=0, cells=0, n_tiles=0, max_width=0)
    tiles: Dict[int, TileTrace] = {}

    def hook(_user, tile, k, L, U, _score):
        t = tiles.setdefault(tile, TileTrace())
        t.max_width = max(t.max_width, U - L + 1)
        t.last_k, t.last_width = k, U - L + 1

    path, err, st = O.align_pair(O.make_params(matrix_of(P), **pk), batch.freq[i, 0, :R, :P], batch.freq[i, 1, :Q, :P], batch.gap_open[i, 0, :R],
                                 batch.gap_extend[i, 0, :R], batch.gap_open[i, 1, :Q], batch.gap_extend[i, 1, :Q], int(batch.num[i, 0]), int(batch.num[i, 1]),
                                 trace=hook if trace else None)
    return PairOracle(path=path, err=err, cells=int(st.cells), n_tiles=int(st.tiles), max_width=int(st.max_width), tiles=[tiles[t] for t in sorted(tiles)])


def oracle_pairs(batch, trace: bool = True, **pk) -> List[PairOracle]:
    with ThreadPoolExecutor(max_workers=8) as ex:      # (the oracle runs outside the interpreter lock)
        return list(ex.map(lambda i: oracle_pair(batch, i, trace, **pk), range(batch.n_pairs)))


def join(*batches):
    """Batches of one alphabet and one stride as a single level."""
    b0 = batches[0]
    assert all(b.P == b0.P and b.seq_len == b0.seq_len for b in batches)
    cat = lambda name: np.concatenate([getattr(b, name) for b in batches])      # noqa: E731
    return synth.LevelBatch(P=b0.P, seq_len=b0.seq_len, freq=cat("freq"), gap_open=cat("gap_open"), gap_extend=cat("gap_extend"), len=cat("len"), num=cat("num"))


# ---- A. band width on the edges of a thread round ----
XDROP_OPEN = 10 ** 7                     # never prunes: the band of tile 0 opens by a row per diagonal until it is the whole shorter side


@dataclass(frozen=True)
class RoundCase:
    P: int
    Q: int                               # the shorter side; the other is Q + 40
    tiles: int                           # tiles of the pair when flen >= Q
    cells: Tuple[int, int, int]          # the oracle's band cells at flen = Q + 7, Q, Q - 1

    @property
    def name(self) -> str:
        return f"{'nuc' if self.P == 6 else 'prot'}{self.Q}"

    def batch(self):
        b = synth.make_level_batch(1, self.Q + 120, P=self.P, members=((1, 4), (1, 4)), seed=7, sub=0.25, indel=0.01)
        assert int(b.len.min()) >= self.Q + 40
        b.len[0] = (self.Q + 40, self.Q)
        return b

    def flens(self) -> Tuple[int, int, int]:
        return (self.Q + 7, self.Q, self.Q - 1)

    def expected(self, flen: int) -> Tuple[int, int, int]:
        """(errorType, widest band, band cells) at `flen`."""
        return (0, self.Q, self.cells[self.flens().index(flen)]) if flen >= self.Q else (2, self.Q - 1, self.cells[2])

    def params(self, flen: int) -> dict:
        return dict(xdrop=XDROP_OPEN, flen=flen)


ROUND_CASES: List[RoundCase] = [
    RoundCase(6, 1023, 3, (1309150, 1309150, 522753)),
    RoundCase(6, 1024, 3, (1286102, 1286102, 523776)),
    RoundCase(6, 1025, 3, (1329011, 1329011, 524800)),
    RoundCase(6, 2047, 5, (6584863, 6584863, 2094081)),
    RoundCase(6, 2048, 5, (6895081, 6895081, 2096128)),
    RoundCase(6, 2049, 5, (6840652, 6840652, 2098176)),
    RoundCase(6, 3073, 7, (19830048, 19830048, 4720128)),
    RoundCase(22, 1025, 3, (1246192, 1246192, 524800)),
]
ROUND_BY_NAME = {c.name: c for c in ROUND_CASES}


# ---- B. convergence while the band is wider than one round ----
@dataclass(frozen=True)
class ConvCase:
    name: str
    sub: float
    xdrop: int
    flen: int
    tiles: int
    max_width: int
    last_widths: Tuple[int, ...]         # width of the last traced diagonal of every tile but the pair's last
    tile_widths: Tuple[int, ...]         # widest diagonal of the same tiles
    cells: int
    seq_len: int = 3100                  # one stride for both pairs, so that they can share a call

    def batch(self):
        return synth.make_level_batch(1, 3000, members=((1, 4), (1, 4)), seed=7, sub=self.sub, indel=0.01, pad_to=self.seq_len)

    def params(self) -> dict:
        return dict(xdrop=self.xdrop, flen=self.flen)


CONV_CASES: List[ConvCase] = [
    # tiles 0, 1 and 2 end by convergence 1854, 1680 and 1206 rows wide; tile 0 was 2462 rows wide on the way
    ConvCase("conv_wide", 0.25, 20000, 3000, 6, 2462, (1854, 1680, 1206, 887, 437), (2462, 2407, 1971, 1460, 952), 17880247),
    # every tile converges after its band has fallen back below one round: the surviving range starts well above L
    ConvCase("conv_narrow", 0.35, 20000, 3000, 6, 2844, (835, 737, 745, 637, 193), (2844, 2476, 1973, 1461, 953), 21411039),
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}


# ---- C. more pairs than workgroups ----
QUEUE_LIVE = 24


def queue_pool(P: int = 6):
    """24 distinct live pairs of mixed lengths, then two with an empty side (order_pairs puts those last and does not launch them)."""
    lo, hi = (30, 1250) if P == 6 else (30, 400)
    pool = synth.make_level_batch(QUEUE_LIVE, 1300 if P == 6 else 420, P=P, members=((1, 3), (1, 3)), seed=3, sub=0.2 if P == 6 else 0.15, indel=0.01)
    rng = np.random.default_rng(1)
    lens = rng.integers(lo, hi, size=(QUEUE_LIVE, 2))
    assert (lens <= pool.len).all()      # (every pair is a prefix of the pair the synth made, never its padding)
    pool.len[:] = lens
    pool = replicate(pool, list(range(QUEUE_LIVE)) + [0, 1])
    pool.len[QUEUE_LIVE] = (0, pool.len[QUEUE_LIVE, 1])
    pool.len[QUEUE_LIVE + 1] = (pool.len[QUEUE_LIVE + 1, 0], 0)
    return pool


def queue_level_size(call: "QueueCall", cus: int) -> int:
    return call.cus_times * cus + 40


def queue_level_index(n_level: int) -> np.ndarray:
    """Which pool pair each pair of a level of `n_level` pairs is: the pool over and over."""
    return np.arange(n_level) % (QUEUE_LIVE + 2)


@dataclass(frozen=True)
class QueueCall:
    name: str
    P: int
    params: Tuple[Tuple[str, int], ...]
    errs: Tuple[int, int, int]           # live pool pairs that end with errorType 0, 1, 2
    max_width: int
    cells: int                           # band cells of the pool
    cus_times: int = 1                   # the level is cus_times x CUs + 40 pairs

    def pk(self) -> dict:
        return dict(self.params)


QUEUE_CALLS: List[QueueCall] = [
    QueueCall("defaults", 6, (), (24, 0, 0), 671, 9087721),
    QueueCall("open", 6, (("xdrop", XDROP_OPEN), ("flen", 4096)), (24, 0, 0), 1033, 10276790),      # first pairs of two rounds
    QueueCall("flen200", 6, (("flen", 200),), (8, 0, 16), 200, 1026322),                              # (flen 96: 3 good pairs, 160: 4, 200: 8)
    QueueCall("xdrop800", 6, (("xdrop", 800),), (8, 16, 0), 154, 2003481),                            # (X-drop 40 and 80: no good pair, 300: 4, 800: 8)
    QueueCall("protein", 22, (), (24, 0, 0), 334, 1051488),
    # None of the calls above takes a second pair past its marker: behind the CUs' first pairs a level of CUs + 40 has the two shortest pool pairs left, 197 and 277
    # diagonals long.  Before the marker the pointer rows are not read, and a float row is never read outside the band the diagonal before wrote, so those calls
    # do not depend on the row re-initialisation at all.  Here every pair has 4 to 40 tiles, and the second and third pairs of a workgroup are twelve different
    # pool pairs of 197 to 1258 diagonals, each tile of which reads the pointer row one element behind the band the diagonal before stored.
    QueueCall("marker64", 6, (("marker", 64),), (24, 0, 0), 671, 51846704, cus_times=2),
]
QUEUE_BY_NAME = {c.name: c for c in QUEUE_CALLS}


# ---- D. scratch above and below the release threshold ----
def scratch_words(flen: int, seq_len: int, marker: int) -> int:
    """32-bit words of one workgroup's scratch, as launch_global sizes them: 14 rows and marker + 2 rows of pointer bytes, each of rowcap elements."""
    rowcap = min(max(flen, 1), max(seq_len, 1)) + 2
    return 14 * rowcap + ((marker + 2) * rowcap + 3) // 4


SCRATCH_LARGE_PAIRS = 72
SCRATCH_LARGE_SEQ_LEN = 4096


def scratch_large():
    """72 short pairs in a level whose stride is 4096 columns: the rows are sized by the stride, not by the pairs."""
    b = synth.make_level_batch(SCRATCH_LARGE_PAIRS, 320, members=((1, 3), (1, 3)), seed=17, pad_to=SCRATCH_LARGE_SEQ_LEN)
    rng = np.random.default_rng(2)
    lens = rng.integers(60, 301, size=(SCRATCH_LARGE_PAIRS, 2))
    assert (lens <= b.len).all()
    b.len[:] = lens
    return b


def scratch_small(members=(1, 1)):
    """The 8-pair batch of test_gpu_global.test_small_pairs_through_the_global_kernel (stride about 600)."""
    return synth.make_level_batch(8, 600, members=members, seed=11)


SCRATCH_CELLS: Dict[str, int] = {"large": 2447897, "small": 2605405}      # band cells of scratch_large() and scratch_small() with every parameter at its default
