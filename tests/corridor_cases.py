"""Directed inputs for the corridor of the precomputed protein scores (score_matrix_kernel, talco_kernel.hip.h; TWL_KNOB_PROT_CORRIDOR).

THE TILE RULE, restated from the kernel's text.  One workgroup of score_matrix_kernel owns the tile of query rows [I0, I0 + 64) and anti-diagonals [K0, K0 + 64)
of a pair of R x Q columns (I0, K0 multiples of 64; the matrix is stored [K][I] with a pitch of (Q + 63) & ~63 floats).  With

    ic   = ((K0 + 32) * Q) // (R + Q)            the query row of the straight line between the corners on the tile's middle anti-diagonal
    need = max(I0 - ic, ic - I0 - 63, 0)         how far the tile's nearest row lies from that row

the kernel leaves the tile unscored -- filled with a quiet NaN -- when `I0 > ic + corridor || I0 + 63 < ic - corridor` and corridor > 0, which is
`0 < corridor < need`.  Nothing here imports anything from the kernel.

THE SMALLEST SAFE CORRIDOR OF A PAIR, c*.  A lean DP kernel on precomputed scores reads, on every anti-diagonal k it computes, the score of every row of the band
[L, U] of that diagonal, and ends the pair with its re-run code when one of them is a NaN.  The oracle's trace hook (oracle/talco_oracle.c, tile_run) reports
(tile, k, L, U) once per diagonal it computes, L, U and k relative to the cell the tile started in: `reference_idx, query_idx` on entry of tile_run, which is
(0, 0) for tile 0 and what the exit hook of the tile before reported as the pair's position after its advance (tests/exit_cases.py) for every later tile.  So
the band cell (tile, k, i) is the matrix cell I = query_idx + i, K = reference_idx + query_idx + k, and

    c* = max need(tile of (I, K)) over every band cell of every traced diagonal.

A pair is handed back to the kernel that scores in line iff 0 < knob < c*.

POOLS.  dp_cases prot16_margin (bands of ~960 rows: the 16-wave routes only), the 600-column short_prot pool of div_cases.py, and `skew700`: 4 pairs of
~700 aa of which pair 1 has its query side cut to 0.6 of its length, so its path leaves the straight line by hundreds of rows.  The tile-parallel route needs
tiles to spread (marker 128), and a pair's tiles and bands depend on the marker: c* is recorded per (pool, marker).  The constants below are the oracle's;
tests/test_corridor_edge_inputs_cpu.py recomputes them, tests/test_gpu_corridor_edges.py runs the pools at knob c* and c* - 1.

MATRIX LEVELS.  Levels of 3-4 pairs of exact lengths for the cell-by-cell comparison of the matrix itself: see LEVELS."""
from __future__ import annotations

import os
import sys
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import div_cases as V  # noqa: E402
import dp_cases as D  # noqa: E402
import oracle_lib as O  # noqa: E402
from twilight_amd import synth  # noqa: E402

TILE = 64


# ---- the tile rule ----
def pitch_of(Q: int) -> int:
    return (Q + 63) & ~63


def tile_grid(R: int, Q: int) -> Tuple[np.ndarray, np.ndarray]:
    """(I0[nI], K0[nK]) of the tiles score_matrix_kernel launches for a pair: query rows 0 .. Q - 1, anti-diagonals 0 .. R + Q - 2."""
    return np.arange(0, Q, TILE, dtype=np.int64), np.arange(0, R + Q - 1, TILE, dtype=np.int64)


def line_row(R: int, Q: int, K0):
    """ic of the tile row K0."""
    return ((np.asarray(K0, dtype=np.int64) + 32) * Q) // (R + Q)


def need(R: int, Q: int, I0, K0):
    I0 = np.asarray(I0, dtype=np.int64)
    ic = line_row(R, Q, K0)
    return np.maximum(np.maximum(I0 - ic, ic - I0 - 63), 0)


def dropped(R: int, Q: int, I0, K0, corridor: int):
    """The tile is left unscored (NaN) at this knob value."""
    n = need(R, Q, I0, K0)
    return (corridor > 0) & (corridor < n)


def need_grid(R: int, Q: int) -> np.ndarray:
    """need of every tile of the pair, [nK][nI]."""
    I0, K0 = tile_grid(R, Q)
    return need(R, Q, I0[None, :], K0[:, None])


def nan_cells(R: int, Q: int, corridor: int) -> np.ndarray:
    """[R + Q][pitch] bool: the float belongs to a dropped tile (cells of the matrix and padding alike)."""
    I0, K0 = tile_grid(R, Q)
    drop = dropped(R, Q, I0[None, :], K0[:, None], corridor)      # [nK][nI]
    full = np.repeat(np.repeat(drop, TILE, axis=0), TILE, axis=1)
    assert full.shape[1] == pitch_of(Q) and full.shape[0] >= R + Q - 1
    out = np.zeros((R + Q, pitch_of(Q)), dtype=bool)      # (row R + Q - 1 holds no cell; no tile covers it when R + Q - 1 is a multiple of 64)
    rows = min(full.shape[0], R + Q)
    out[:rows] = full[:rows]
    return out


def cell_mask(R: int, Q: int) -> np.ndarray:
    """[R + Q][pitch] bool: the float is a cell of the matrix -- I < Q and 0 <= K - I < R."""
    K = np.arange(R + Q, dtype=np.int64)[:, None]
    I = np.arange(pitch_of(Q), dtype=np.int64)[None, :]
    return (I < Q) & (K - I >= 0) & (K - I < R)


# ---- c* from the oracle ----
def band_of_pair(batch, i: int, matrix: np.ndarray, **pk):
    """(errorType, [(tile, K, Ilo, Ihi)]): every traced diagonal of pair `i` as absolute anti-diagonal and absolute query rows."""
    R, Q, P = int(batch.len[i, 0]), int(batch.len[i, 1]), batch.P
    origin = [(0, 0)]          # (reference_idx, query_idx) tile t starts in
    rows: List[Tuple[int, int, int, int]] = []

    def trace(_user, tile, k, L, U, _score):
        r0, q0 = origin[tile]
        rows.append((tile, r0 + q0 + k, q0 + L, q0 + U))

    def exits(_user, tile, _last_k, _kind, _state, _cr, _cq, ridx, qidx):
        assert tile == len(origin) - 1
        origin.append((int(ridx), int(qidx)))

    _, err, _ = O.align_pair_exits(O.make_params(matrix, **pk), batch.freq[i, 0, :R, :P], batch.freq[i, 1, :Q, :P], batch.gap_open[i, 0, :R], batch.gap_extend[i, 0, :R],
                                   batch.gap_open[i, 1, :Q], batch.gap_extend[i, 1, :Q], int(batch.num[i, 0]), int(batch.num[i, 1]), trace=trace, exits=exits)
    return err, rows


def cstar_of_rows(R: int, Q: int, rows) -> int:
    """max need over the tiles that hold a band cell.  need is convex in I0 along a tile row, so the two end tiles of a diagonal's band decide."""
    if not rows:
        return 0
    a = np.asarray(rows, dtype=np.int64)
    K, lo, hi = a[:, 1], a[:, 2], a[:, 3]
    assert (lo <= hi).all() and (lo >= 0).all() and (hi < Q).all() and (K - hi >= 0).all() and (K - lo < R).all()      # band cells are cells of the matrix
    K0 = (K // TILE) * TILE
    return int(max(need(R, Q, (lo // TILE) * TILE, K0).max(), need(R, Q, (hi // TILE) * TILE, K0).max()))


def cstar_pair(batch, i: int, matrix: np.ndarray, **pk) -> int:
    err, rows = band_of_pair(batch, i, matrix, **pk)
    assert err == 0, (i, err)
    return cstar_of_rows(int(batch.len[i, 0]), int(batch.len[i, 1]), rows)


def cstars(batch, matrix: np.ndarray, **pk) -> Tuple[int, ...]:
    with ThreadPoolExecutor(max_workers=4) as ex:
        return tuple(ex.map(lambda i: cstar_pair(batch, i, matrix, **pk), range(batch.n_pairs)))


def handed_back(cs, knob: int) -> List[int]:
    """The pairs whose band reads a NaN at this knob value."""
    return [n for n, c in enumerate(cs) if 0 < knob < c]


# ---- pools ----
SKEW_XDROP = 2000


def _skew700():
    b = synth.make_level_batch(4, 700, P=22, members=((2, 6), (2, 6)), seed=311, sub=0.15, indel=0.01)
    q = int(int(b.len[1, 1]) * 0.6)      # pair 1: the query side cut to 0.6 of its length
    for a in (b.freq, b.gap_open, b.gap_extend):
        a[1, 1, q:] = 0
    b.len[1, 1] = q
    return b


@dataclass(frozen=True)
class CorridorPool:
    name: str
    marker: int
    routes: Tuple[str, ...]              # the routes of test_gpu_corridor_edges.EDGE_ROUTES the pool is sent down
    cstar: Tuple[int, ...]               # the oracle's c* per pair
    spans: Tuple[int, ...]               # ... and largest span in 64-row blocks per pair (dp_cases.PairTrace.span): below the narrowest window of `routes`

    def batch(self):
        base = self.name.split("@")[0]
        if base == "skew700":
            return _skew700()
        return (V.SHORT_POOLS[base] if base in V.SHORT_POOLS else D.BY_NAME[base]).batch()

    def params(self) -> dict:
        base = self.name.split("@")[0]
        pk = dict(xdrop=SKEW_XDROP, flen=4096) if base == "skew700" else (V.SHORT_POOLS[base] if base in V.SHORT_POOLS else D.BY_NAME[base]).params()
        pk["marker"] = self.marker
        return pk

    def longest_q(self, batch=None) -> int:
        b = self.batch() if batch is None else batch
        return int(b.len[:, 1].max())

    def knob_values(self) -> List[int]:
        """c* and c* - 1 of every distinct c*."""
        return sorted({v for c in set(self.cstar) for v in (c, c - 1)})


LEAN16, ALL3 = ("prot_plain16", "prot_spec16"), ("prot_plain16", "prot_spec16", "prot_spec_shared")
POOLS: List[CorridorPool] = [
    CorridorPool("prot16_margin", 1024, LEAN16, cstar=(494, 466, 496), spans=(15, 15, 15)),
    CorridorPool("short_prot", 1024, ALL3, cstar=(47, 52, 50, 52, 51, 49, 49, 49), spans=(2,) * 8),
    CorridorPool("short_prot@128", 128, ("prot_tiles",), cstar=(47, 52, 50, 52, 51, 49, 49, 49), spans=(2,) * 8),
    CorridorPool("skew700", 1024, ALL3, cstar=(109, 166, 115, 113), spans=(3, 4, 4, 4)),
    CorridorPool("skew700@128", 128, ("prot_tiles",), cstar=(109, 166, 115, 113), spans=(4, 4, 4, 4)),
]
POOL_BY_NAME: Dict[str, CorridorPool] = {p.name: p for p in POOLS}


def check_pool(pool: CorridorPool, cs, spans, narrowest: int) -> None:
    """The pool is what it claims to be: raises AssertionError otherwise."""
    tag = f"{pool.name}: c* {tuple(cs)} spans {tuple(spans)}"
    assert tuple(cs) == pool.cstar and tuple(spans) == pool.spans, tag
    assert max(cs) >= 2, tag
    assert len(set(cs)) >= 2, tag
    assert max(spans) < narrowest, tag


# ---- matrix levels: (R, Q) per pair, exact ----
# Every level mixes sizes, so the walk over blk_off crosses items of different tile counts (launch order: longest R + Q first), and holds at least one tile the
# rule drops and one it keeps at MATRIX_KNOB (tests/test_corridor_edge_inputs_cpu.py).  `leaf` names the pair of single sequences (denominator 1), if any.
MATRIX_KNOB = 64


@dataclass(frozen=True)
class MatrixLevel:
    name: str
    shapes: Tuple[Tuple[int, int], ...]
    leaf: int = -1
    gap_char: float = -5.0

    def batch(self, seed: int):
        n = len(self.shapes)
        length = int(max(max(s) for s in self.shapes) / 0.9) + 16
        b = synth.make_level_batch(n, length, P=22, members=((2, 6), (2, 6)), seed=seed, sub=0.15, indel=0.01)
        if self.leaf >= 0:
            lf = synth.make_level_batch(n, length, P=22, members=(1, 1), seed=seed + 1000, sub=0.15, indel=0.01, pad_to=b.seq_len + 64)
            for a, s in ((b.freq, lf.freq), (b.gap_open, lf.gap_open), (b.gap_extend, lf.gap_extend)):
                a[self.leaf] = s[self.leaf][:, : b.seq_len]
            b.len[self.leaf] = np.minimum(lf.len[self.leaf], b.seq_len)
            b.num[self.leaf] = (1, 1)
        for i, (R, Q) in enumerate(self.shapes):
            for side, L in ((0, R), (1, Q)):
                assert 1 <= L <= int(b.len[i, side]), (self.name, i, side, L, int(b.len[i, side]))
                for a in (b.freq, b.gap_open, b.gap_extend):
                    a[i, side, L:] = 0
                b.len[i, side] = L
        return b

    def params(self) -> dict:
        return dict(gap_char=self.gap_char, xdrop=5000, flen=4096)

    def edge_knobs(self) -> Tuple[int, int]:
        """(below, above): the smallest positive `I0 - ic` and the smallest positive `ic - I0 - 63` over the tiles of the level.  With the knob ON such a value the tile
        that has it is the last one kept on its side of the line -- `I0 > ic + corridor` and `I0 + 63 < ic - corridor` are strict -- and one row less drops it."""
        below, above = [], []
        for R, Q in self.shapes:
            I0, K0 = tile_grid(R, Q)
            ic = line_row(R, Q, K0)[:, None]
            below += (I0[None, :] - ic)[(I0[None, :] - ic) > 0].tolist()
            above += (ic - I0[None, :] - 63)[(ic - I0[None, :] - 63) > 0].tolist()
        return int(min(below)), int(min(above))

    def knobs(self) -> List[int]:
        """The knob values of the cell-by-cell test: MATRIX_KNOB, the whole matrix, and on and one below each of the two edge values."""
        b, a = self.edge_knobs()
        return [MATRIX_KNOB, 0] + sorted({v for v in (b, b - 1, a, a - 1) if v > 0} - {MATRIX_KNOB})


LEVELS: List[MatrixLevel] = [
    # Q one below, on and one above a multiple of 64 (pitch 256, 256, 320), beside a leaf pair
    MatrixLevel("q_mod64", ((300, 255), (310, 256), (290, 257), (270, 250)), leaf=3),
    # R + Q - 1 one below, on and one above a multiple of 64: the last tile row holds 63, 64 and 1 anti-diagonals
    MatrixLevel("k_mod64", ((312, 200), (313, 200), (314, 200))),
    # Q < 64 (one tile column, nothing to drop), R = 1, Q = 1, beside a pair with tiles to drop
    MatrixLevel("thin", ((400, 40), (1, 300), (300, 1), (350, 330))),
    # R ~ 3 Q and Q ~ 3 R: the line's slope is far from the tile's diagonal
    MatrixLevel("skew", ((600, 200), (200, 600), (330, 310)), leaf=2),
    # the gap-letter terms off
    MatrixLevel("gap_char_0", ((300, 255), (310, 256), (290, 257), (270, 250)), leaf=3, gap_char=0.0),
]
LEVEL_BY_NAME = {lv.name: lv for lv in LEVELS}
