"""Directed inputs for the fast division of the lean DP kernels (fast_div, talco_div.hip.h) at the corners of its guard.

The three guards, as the code states them:

* a profile entry is zero or 2^-20 <= |x| <= 2^30 (div_guard_bad, talco_div.hip.h);
* the denominator float(refNum) * float(qryNum) lies in [1, 2^40] (talco_lean_kernel, in front of the first tile);
* every score of the matrix and gap_char are zero or within [2^-10, 2^10] (fast_div_in_range, twl_policy.inc.hip).

Inside them the smallest non-zero product is 2^-20 * 2^-10 * 2^-20 = 2^-50 (ulp 2^-73), the largest 2^30 * 2^10 * 2^30 = 2^70, and a
numerator is a sum of at most 483 of them: |n| == 0 or 2^-73 <= |n| < 2^80.

SCORE CASES.  A case is one pair of Q x R columns whose column scores are a grid: cell (query row i, reference column j) is a function
of row i and column j alone, so a planned operand combination is a special row crossed with a special column; `planned` lists them
with the numerator each must have.  The rest of the grid is a seeded random fill.  For the dump of the DP kernel to hold EVERY cell the
band must be the whole matrix, and the X-drop is a 32-bit integer while these quotients reach 2^75: a cell of a huge POSITIVE score
raises the running maximum, and everything not descended from it is dropped.  A huge NEGATIVE score does no harm (the cell is reached
through a gap instead).  So the cases keep every large term negative, which the division cannot tell from positive (it is odd in n):

* reference columns carry their large entries on the letters BIG_R, query rows on BIG_Q, and every score M[BIG_R][BIG_Q] is <= 0
  (nucleotide: A, C against G, T -- transitions and transversions; protein: chosen from the matrix);
* the other letters are `small`: at most s_max = 2^-12 * d / (largest positive score), so that a positive term is at most 2^18 * d --
  or exactly zero where s_max falls below 2^-20 (a zero passes the guard);
* gap_char is negative, so the gap letter may be large on both sides;
* row 0 and column 0 are plain one-letter columns (the band starts there and cell (0, 0) has no gap to fall back on).

tests/test_div_edge_inputs_cpu.py asserts the outcome -- no score above 2^21, cell (0, 0) small, and by the oracle's trace a band that
is the whole matrix on every diagonal -- with xdrop = 2^29 and ordinary gap penalties.

GUARD CASES are built from the pools of dp_cases.py: see GuardCase below."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dp_cases as D  # noqa: E402
from twilight_amd import synth  # noqa: E402

F = np.float32
ENTRY_LO, ENTRY_HI = F(2.0 ** -20), F(2.0 ** 30)
SCORE_LO, SCORE_HI = F(2.0 ** -10), F(2.0 ** 10)
DENOM_HI = F(2.0 ** 40)
XDROP, FLEN = 1 << 29, 4096
Q_ROWS, R_COLS = 70, 53          # two 64-row blocks of query rows, not a multiple of anything


def up(x) -> np.float32:
    return np.nextafter(F(x), F(np.inf))


def down(x) -> np.float32:
    return np.nextafter(F(x), F(0))


# ---- the three guards, as the code states them ----
def entry_ok(x) -> bool:
    ax = abs(F(x))
    return bool(F(x) == 0 or (ax >= ENTRY_LO and ax <= ENTRY_HI))


def score_ok(x) -> bool:
    ax = abs(F(x))
    return bool(F(x) == 0 or (ax >= SCORE_LO and ax <= SCORE_HI))


def denom_of(nums) -> np.float32:
    return F(F(nums[0]) * F(nums[1]))


def denom_ok(nums) -> bool:
    d = denom_of(nums)
    return bool(d >= F(1) and d <= DENOM_HI)


# ---- the oracle's numerator (oracle/talco_oracle.c, twlo_column_score) in numpy float32, for a whole grid at once ----
def numerators(P: int, mat: np.ndarray, gc, ref: np.ndarray, qry: np.ndarray) -> np.ndarray:
    """[Q][R] numerators of the column score: every operation one float32 operation, in the oracle's order."""
    ref = np.asarray(ref, dtype=F)
    qry = np.asarray(qry, dtype=F)
    mat = np.asarray(mat, dtype=F)
    gc = F(gc)
    n = P - 1                                   # letters with a score; the gap letter is P - 1
    num = np.zeros((qry.shape[0], ref.shape[0]), dtype=F)
    qc = [qry[:, m][:, None] for m in range(P)]
    rc = [ref[:, l][None, :] for l in range(P)]
    with np.errstate(all="raise"):
        if P == 6:
            for l in range(5):
                s = F(0) + (qc[0] * mat[l, 0]) * rc[l]
                for m in range(1, 5):
                    s = s + (F(0) + (qc[m] * mat[l, m]) * rc[l])
                num = num + s
        else:
            for l in range(21):
                v = []
                for t in range(8):
                    s = F(0) + (qc[t] * mat[l, t]) * rc[l]
                    v.append(s + (qc[8 + t] * mat[l, 8 + t]) * rc[l])
                for m in range(16, 21):
                    num = num + (rc[l] * qc[m]) * mat[l, m]
                s = v[0]
                for t in range(1, 8):
                    s = s + v[t]
                num = num + s
        for l in range(n):
            num = num + (rc[l] * qc[n]) * gc
        for m in range(n):
            num = num + (rc[n] * qc[m]) * gc
    assert num.dtype == F
    return num


# ---- denominators: (refNum, qryNum) ----
DENOMS: Dict[str, Tuple[int, int]] = {
    "d1": (1, 1),
    "d3": (3, 1), "d7": (1, 7), "d11": (11, 1), "d21": (3, 7),      # quotients that are not representable
    "d2p40": (1 << 20, 1 << 20),                                      # 2^40 exactly
    "d2p40_rounded": ((1 << 20) + 1, (1 << 20) - 1),                  # 2^40 - 1 as integers, 2^40 as float32 * float32: accepted
    "d2p40_below": (4095 << 8, 4097 << 8),                            # (2^24 - 1) * 2^16: the largest float32 below 2^40
    # spread log-uniformly over [1, 2^40]: 2^13.1, 2^19.2, 2^26.9, 2^33.9
    "r_13": (53, 167), "r_19": (1811, 331), "r_27": (30211, 4099), "r_34": (700001, 23003),
}


@dataclass
class ScoreCase:
    name: str
    mode: str                  # "nuc2" | "nuc2_leaf" | "nuc5" | "nuc1" | "nuc0" | "prot3"
    variant: str
    P: int
    matrix: np.ndarray
    gap_char: np.float32
    nums: Tuple[int, int]
    ref: np.ndarray            # [R][P]
    qry: np.ndarray            # [Q][P]
    planned: List[Tuple[int, int, str, Optional[np.float32]]] = field(default_factory=list)      # (row, column, corner, numerator or None)
    onehot_query: bool = False

    @property
    def denom(self) -> np.float32:
        return denom_of(self.nums)

    def params(self) -> dict:
        return dict(gap_char=float(self.gap_char), xdrop=XDROP, flen=FLEN)

    def batch(self):
        R, Q, P = self.ref.shape[0], self.qry.shape[0], self.P
        sl = max(R, Q)
        freq = np.zeros((1, 2, sl, P), dtype=F)
        freq[0, 0, :R] = self.ref
        freq[0, 1, :Q] = self.qry
        gop = np.zeros((1, 2, sl), dtype=F)
        gex = np.zeros((1, 2, sl), dtype=F)
        gop[0, 0, :R] = -50; gop[0, 1, :Q] = -50
        gex[0, 0, :R] = -5; gex[0, 1, :Q] = -5
        return synth.LevelBatch(P=P, seq_len=sl, freq=freq, gap_open=gop, gap_extend=gex, len=np.array([[R, Q]], dtype=np.int32),
                                num=np.array([self.nums], dtype=np.int32))

    def numer(self) -> np.ndarray:
        return numerators(self.P, self.matrix, self.gap_char, self.ref, self.qry)

    def corners(self) -> set:
        return {c for _i, _j, c, _n in self.planned}


# ---- matrices.  Every variant keeps M[BIG_R][BIG_Q] <= 0 ----
def _letters(P: int, mat: np.ndarray):
    """(a, a2, g, g2, BIG_R, BIG_Q): the letters the special columns / rows use and the sets that may carry large entries."""
    if P == 6:
        return 0, 1, 2, 3, (0, 1), (2, 3)
    # protein: from the matrix.  BIG_Q: the letters that score below zero against isoleucine-like letter 0 of the hydrophobic block ...
    seed = int(np.argmin(mat[:20, :20].sum(axis=1)))          # the letter with the lowest row sum (deterministic)
    big_q = tuple(m for m in range(20) if mat[seed, m] < 0)
    big_r = tuple(l for l in range(20) if l not in big_q and all(mat[l, m] <= 0 for m in big_q))
    assert len(big_r) >= 2 and len(big_q) >= 2, (big_r, big_q)
    return big_r[0], big_r[1], big_q[0], big_q[1], big_r, big_q


def _mode2(match, transversion, transition) -> np.ndarray:
    return synth.nucleotide_matrix(match=match, mismatch=transversion, transition=transition)


def _int_matrix(seed: int, n_zero_row: bool) -> np.ndarray:
    """The matrices of test_scores_inside_the_dp_kernel_match_oracle (integers in [-9, 18]), with the scores between BIG_R and BIG_Q below zero."""
    rng = np.random.default_rng(seed)
    mat = rng.integers(-9, 19, size=(5, 5)).astype(F)
    for l in (0, 1):
        for m in (2, 3):
            mat[l, m] = -abs(mat[l, m]) - 1
    if n_zero_row:
        mat[4, :] = 0
        mat[:, 4] = 0
    return mat


def _variants(mode: str):
    """(variant, matrix, gap_char, the corners its special cells reach) of a mode."""
    lo, hi = SCORE_LO, SCORE_HI
    if mode in ("nuc2", "nuc2_leaf", "nuc5"):
        return [("default", _mode2(18.0, -8.0, -4.0), F(-5)),
                # match 2^-10, transition -2^-10 (they cancel), transversion -2^10; gap_char on the lower limit
                ("limits_cancel", _mode2(lo, -hi, -lo), -lo),
                # the default matrix's shape (match > 0 > transition > transversion) on the limits: match 2^10, transition -2^-10, transversion -2^10
                ("limits_scaled", _mode2(hi, -hi, -lo), -hi),
                ("all_max", _mode2(-hi, -hi, -hi), -hi)]
    if mode == "nuc1":
        base = _int_matrix(5, True)
        lim = base.copy()
        lim[0, 2], lim[2, 2], lim[0, 3], lim[1, 2], lim[3, 3] = -lo, lo, -hi, -hi, hi
        mx = np.full((5, 5), -hi, dtype=F)
        mx[4, :] = 0; mx[:, 4] = 0
        mx[3, 3] = -F(512)                        # (sixteen equal scores would be mode 2: T against T is not on the limit, and the all_max column has no T)
        return [("default", base, F(-5)), ("limits_cancel", lim, -lo), ("all_max", mx, -hi)]
    if mode == "nuc0":
        wild = _mode2(18.0, -8.0, -4.0)
        wild[4, :] = 18.0; wild[:, 4] = 18.0
        base = _int_matrix(6, False)
        lim = base.copy()
        lim[0, 2], lim[2, 2], lim[0, 3], lim[1, 2], lim[3, 3], lim[4, 4], lim[4, 2] = -lo, lo, -hi, -hi, hi, hi, -lo
        return [("wildcard", wild, F(-5)), ("default", base, F(-5)), ("limits_cancel", lim, -lo), ("all_max", np.full((5, 5), -hi, dtype=F), -hi)]
    if mode == "prot3":
        base = synth.protein_matrix().copy()
        a, a2, g, g2, _br, _bq = _letters(22, base)
        lim = base.copy()
        lim[a, g], lim[g, g], lim[a, g2], lim[a2, g], lim[g2, g2] = -lo, lo, -hi, -hi, hi
        return [("default", base, F(-5)), ("limits_cancel", lim, -lo), ("all_max", np.full((21, 21), -hi, dtype=F), -hi)]
    raise ValueError(mode)


MODES = ("nuc2", "nuc2_leaf", "nuc5", "nuc1", "nuc0", "prot3")
# rows and columns of the special cells (row 0 and column 0 are the plain start)
ROW = {"lo": 5, "hi": 23, "lo2": 41, "max": 66, "last": Q_ROWS - 1}
COL = {"lo": 3, "hi": 19, "cancel": 30, "cancel_up": 37, "zero": 44, "max": 50, "last": R_COLS - 1}


def _log_uniform(rng, lo, hi, size):
    return np.exp2(rng.uniform(np.log2(float(lo)), np.log2(float(hi)), size=size)).astype(F)


def _onehot(P, letter, value):
    v = np.zeros(P, dtype=F)
    v[letter] = value
    return v


def build_score_case(mode: str, variant: str, mat: np.ndarray, gc, dname: str) -> ScoreCase:
    P = 22 if mode == "prot3" else 6
    nums = DENOMS[dname]
    d = float(denom_of(nums))
    onehot = mode == "nuc5"
    a, a2, g, g2, big_r, big_q = _letters(P, synth.protein_matrix() if P == 22 else mat)
    assert all(mat[l, m] <= 0 for l in big_r for m in big_q) and gc < 0
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"{mode}/{variant}/{dname}".encode()))
    maxpos = float(max(mat.max(), 0.0))
    s_max = float(ENTRY_HI) if maxpos == 0 else min(float(ENTRY_HI), 2.0 ** -12 * d / maxpos)
    n = P - 1

    def fill(count, big, is_query):
        """Random rows / columns: log-uniform over the whole range on the big letters and the gap letter, `small` (or zero) elsewhere; one entry in four is zero."""
        out = np.zeros((count, P), dtype=F)
        for t in range(count):
            if is_query and onehot:                  # one letter of A, C, G, T per query row, no gap letter
                m = int(rng.integers(0, 4))
                top = float(ENTRY_HI) if m in big else s_max
                if top < 2 * float(ENTRY_LO):
                    m, top = big[int(rng.integers(0, len(big)))], float(ENTRY_HI)
                out[t, m] = _log_uniform(rng, ENTRY_LO, top, 1)[0]
                continue
            for letter in range(P):
                if rng.random() < 0.25:
                    continue
                top = float(ENTRY_HI) if (letter in big or letter == n) else s_max
                if top < 2 * float(ENTRY_LO):
                    continue
                out[t, letter] = _log_uniform(rng, ENTRY_LO, top, 1)[0]
            if not out[t].any():
                out[t, big[0]] = F(1)
        return out

    ref = fill(R_COLS, big_r, False)
    qry = fill(Q_ROWS, big_q, True)
    ref[0] = _onehot(P, a, 1.0)
    qry[0] = _onehot(P, g, 1.0)
    # the special columns and rows
    ref[COL["lo"]] = _onehot(P, a, ENTRY_LO)
    ref[COL["hi"]] = _onehot(P, a, ENTRY_HI)
    ref[COL["cancel"]] = _onehot(P, a, ENTRY_LO) + _onehot(P, g, up(ENTRY_LO))
    ref[COL["cancel_up"]] = _onehot(P, a, 2 * ENTRY_LO) + _onehot(P, g, up(2 * ENTRY_LO))
    ref[COL["zero"]] = _onehot(P, a, ENTRY_LO) + _onehot(P, g, ENTRY_LO)
    qry[ROW["lo"]] = _onehot(P, g, ENTRY_LO)
    qry[ROW["hi"]] = _onehot(P, g, ENTRY_HI)
    qry[ROW["lo2"]] = _onehot(P, g, 2 * ENTRY_LO)
    mag, lo = F(mat[a, g]), ENTRY_LO
    planned: List[Tuple[int, int, str, Optional[np.float32]]] = []
    for rn, rv in (("lo", ENTRY_LO), ("hi", ENTRY_HI)):
        for cn, cv in (("lo", ENTRY_LO), ("hi", ENTRY_HI)):
            planned.append((ROW[rn], COL[cn], f"entry_{rn}_x_{cn}", F(F(rv * mag) * cv)))
    if variant == "limits_cancel":
        assert mat[a, g] == -SCORE_LO and mat[g, g] == SCORE_LO
        planned.append((ROW["lo"], COL["cancel"], "min_numerator", F(2.0 ** -73)))
        planned.append((ROW["lo"], COL["cancel_up"], "min_numerator_up", F(2.0 ** -72)))
        planned.append((ROW["lo2"], COL["cancel"], "min_numerator_up", F(2.0 ** -72)))
        planned.append((ROW["lo"], COL["zero"], "zero", F(0)))
        planned.append((ROW["hi"], COL["zero"], "zero", F(0)))
        planned.append((ROW["lo"], COL["lo"], "score_lo", F(-(2.0 ** -50))))
    if variant in ("limits_cancel", "limits_scaled"):
        # a transversion / a score of -2^10 between the second big letters, entries on both limits
        ref[COL["max"]] = _onehot(P, a2 if P == 22 or mode in ("nuc1", "nuc0") else a, ENTRY_HI)
        l2 = a2 if P == 22 or mode in ("nuc1", "nuc0") else a
        m2 = g if l2 == a2 else g2
        assert mat[l2, m2] == -SCORE_HI, (mode, variant)
        qry[ROW["max"]] = _onehot(P, m2, ENTRY_HI)
        planned.append((ROW["max"], COL["max"], "score_hi", F(-(2.0 ** 70))))
        planned.append((ROW["max"], COL["max"], "gap_char_on_limit", None))
    if variant == "all_max":
        # every term at 2^30 * 2^10 * 2^30, all negative
        col = np.full(P, ENTRY_HI, dtype=F)
        row = np.full(P, ENTRY_HI, dtype=F)
        if mode == "nuc1":
            col[3] = 0                              # (no T: see _variants)
        if onehot:
            row = _onehot(P, g, ENTRY_HI)
        ref[COL["max"]] = col
        qry[ROW["max"]] = row
        ref[COL["last"]] = col
        qry[ROW["last"]] = row
        terms = sum(1 for l in range(n) for m in range(n) if col[l] != 0 and row[m] != 0 and mat[l, m] != 0)
        terms += sum(1 for l in range(n) if col[l] != 0 and row[n] != 0) + sum(1 for m in range(n) if col[n] != 0 and row[m] != 0)
        for rn, cn in (("max", "max"), ("last", "last")):
            planned.append((ROW[rn], COL[cn], "max_numerator", F(-float(terms) * 2.0 ** 70)))
        planned.append((ROW["max"], COL["max"], "gap_char_on_limit", None))
    dn = {"d1": "denom_1", "d2p40": "denom_2p40", "d2p40_rounded": "denom_2p40_rounded", "d2p40_below": "denom_2p40_below"}.get(dname, "denom_odd" if dname.startswith("d") else "denom_random")
    planned.append((ROW["lo"], COL["lo"], dn, None))
    return ScoreCase(name=f"{mode}-{variant}-{dname}", mode=mode, variant=variant, P=P, matrix=mat, gap_char=F(gc), nums=nums, ref=ref, qry=qry, planned=planned,
                     onehot_query=onehot)


def _score_cases() -> List[ScoreCase]:
    out = []
    for mode in MODES:
        for variant, mat, gc in _variants(mode):
            for dname in DENOMS:
                if mode == "nuc2_leaf" and dname != "d1":
                    continue      # a leaf pair is two single sequences: refNum * qryNum == 1, the kernel's branch without a division
                out.append(build_score_case(mode, variant, mat, gc, dname))
    return out


SCORE_CASES: List[ScoreCase] = _score_cases()
SCORE_BY_NAME = {c.name: c for c in SCORE_CASES}
# what every mode's cases must reach between them (tests/test_div_edge_inputs_cpu.py)
CORNERS = ("entry_lo_x_lo", "entry_lo_x_hi", "entry_hi_x_lo", "entry_hi_x_hi", "score_lo", "score_hi", "gap_char_on_limit", "max_numerator", "min_numerator",
           "min_numerator_up", "zero", "denom_1", "denom_odd", "denom_2p40", "denom_2p40_rounded", "denom_2p40_below", "denom_random")
LEAF_CORNERS = tuple(c for c in CORNERS if not c.startswith("denom_") or c == "denom_1")


# ================================================================ guard cases ================================================================
# A guard case is a pool of dp_cases.py (or one of the two short pools below) in which the pairs `carriers` carry ONE changed profile entry
# each -- or changed member counts -- and nothing else differs.  The changed entry replaces a ZERO of the profile by a value of about 1e-6:
# no score moves by more than that, so the spans of the pool are the committed ones and the pool is still a margin pool of its window
# (tests/test_div_edge_inputs_cpu.py recomputes them).  `value`:
#   "below_lo"  the float32 below 2^-20: outside the guard, the pair must be re-run on the IEEE-division kernel
#   "lo"        2^-20 exactly: the twin, which must NOT be re-run
#   "hi" / "above_hi"   2^30 and the float32 above it (short pools only).  An entry that large makes one column score ~2^33 and the
#               running maximum with it: every cell that does not descend from that cell is dropped, and from there the band opens by a
#               row per diagonal.  The entry sits 40 rows before the end of the query, so the band that regrows stays below 100 rows and the
#               spans of the pool stay what they were: 2 blocks, far below every window.
# `where` places the entry: the row / column is inside the band (the pair's optimal path runs through it with a match step).
SHORT_XDROP = 1000
SHORT_POOLS = {
    "short_nuc": D.DpCase(name="short_nuc", P=6, nv=8, kind="short", length=600, n=8, seed=211, xdrop=SHORT_XDROP, gen=(("members", ((2, 6), (2, 6))),),
                          spans=(2,) * 8, widths=(102, 98, 98, 105, 109, 95, 110, 108)),
    "short_prot": D.DpCase(name="short_prot", P=22, nv=8, kind="short", length=600, n=8, seed=212, xdrop=SHORT_XDROP, gen=(("members", ((2, 6), (2, 6))),),
                           spans=(2,) * 8, widths=(78, 81, 91, 86, 80, 79, 81, 79)),
}
VALUES = {"below_lo": down(ENTRY_LO), "lo": ENTRY_LO, "hi": ENTRY_HI, "above_hi": up(ENTRY_HI)}
# where -> (side 0 reference / 1 query, index (negative: from the end), letter: None = the first of the scored letters whose entry is zero, "gap" = P - 1)
WHERE = {
    "first_tile": (1, 10, None),                 # query row 10: every window holds it from the first diagonal of the first tile
    "ref_first_tile": (0, 200, None),
    "mid": (1, 700, None),
    "last_ref_col": (0, -1, None),
    "last_query_row": (1, -1, None),
    "gap_letter": (1, 333, "gap"),
    "near_end": (1, -40, None),
    # short_nuc pair 3 at marker 128: the path crosses anti-diagonals 381 .. 384 = [3 * (marker - 1), 3 * marker] in reference columns 196 and 197, and every tile after the
    # first begins where ref + qry has advanced by marker - 1 or marker: the fourth tile begins in this column or next to it, the third ends around it
    "tile_boundary": (0, 197, None),
}


def pool_of(name: str) -> D.DpCase:
    return SHORT_POOLS[name] if name in SHORT_POOLS else D.BY_NAME[name]


@dataclass(frozen=True)
class GuardCase:
    name: str
    pool: str
    carriers: Tuple[int, ...]
    where: str = "first_tile"
    value: Optional[str] = "below_lo"            # None: no entry changes (the denominator twins)
    marker: int = 1024
    nums: Tuple[Tuple[int, Tuple[int, int]], ...] = ()      # (pair, (refNum, qryNum)) overrides
    spans: Optional[Tuple[int, ...]] = None      # the oracle's spans of the changed pool when they are not the pool's committed ones
    rerun: Tuple[int, ...] = ()                  # the pairs the lean kernels must hand to the IEEE-division kernel

    @property
    def P(self) -> int:
        return pool_of(self.pool).P

    def params(self) -> dict:
        pk = pool_of(self.pool).params()
        if self.marker != 1024:
            pk["marker"] = self.marker
        return pk

    def expected_spans(self) -> Tuple[int, ...]:
        return self.spans if self.spans is not None else pool_of(self.pool).spans

    def changes(self, base) -> List[Tuple[int, int, int, int]]:
        """(pair, side, index, letter) of every changed entry."""
        if self.value is None:
            return []
        side, index, letter = WHERE[self.where]
        out = []
        for n in self.carriers:
            L = int(base.len[n, side])
            i = index if index >= 0 else L + index
            assert 0 <= i < L
            row = base.freq[n, side, i]
            t = base.P - 1 if letter == "gap" else next(t for t in range(4 if base.P == 6 else 20) if row[t] == 0)
            out.append((n, side, i, t))
        return out

    def batch(self, base=None):
        base = pool_of(self.pool).batch() if base is None else base
        f = base.freq.copy()
        num = base.num.copy()
        for n, side, i, t in self.changes(base):
            assert f[n, side, i, t] == 0
            f[n, side, i, t] = VALUES[self.value]
        for n, ab in self.nums:
            num[n] = ab
        return synth.LevelBatch(P=base.P, seq_len=base.seq_len, freq=f, gap_open=base.gap_open, gap_extend=base.gap_extend, len=base.len, num=num)


def path_diagonals(batch, n: int, side: int, index: int, matrix: np.ndarray, **pk) -> List[int]:
    """The anti-diagonals (ref + qry) of the MATCH steps with which the oracle's optimal path of pair `n` consumes row / column `index` of `side`."""
    import oracle_lib as O
    R, Q, P = int(batch.len[n, 0]), int(batch.len[n, 1]), batch.P
    aln, err, _ = O.align_pair(O.make_params(matrix, **pk), batch.freq[n, 0, :R, :P], batch.freq[n, 1, :Q, :P], batch.gap_open[n, 0, :R], batch.gap_extend[n, 0, :R],
                               batch.gap_open[n, 1, :Q], batch.gap_extend[n, 1, :Q], int(batch.num[n, 0]), int(batch.num[n, 1]))
    if err != 0:
        return []
    r = np.cumsum(aln != 1) - 1          # reference column a step consumes (codes: 0 both, 1 query only, 2 reference only)
    q = np.cumsum(aln != 2) - 1
    pos = r if side == 0 else q
    return [int(k) for k in (r + q)[(aln == 0) & (pos == index)]]


def on_path(batch, n: int, side: int, index: int, matrix: np.ndarray, **pk) -> bool:
    """The oracle's optimal path of pair `n` consumes row / column `index` of `side` with a MATCH step: that cell was computed inside the band (and is not
    part of the tail the reference appends behind the last tile without a DP), so the kernel that took the pair has loaded the row and the column."""
    return len(path_diagonals(batch, n, side, index, matrix, **pk)) > 0


def _twins(name, pool, carriers, where, values=("below_lo", "lo"), **kw):
    spans = kw.pop("spans", {})
    return [GuardCase(name=f"{name}-{v}", pool=pool, carriers=carriers, where=where, value=v, rerun=carriers if v in ("below_lo", "above_hi") else (),
                      spans=spans.get(v) if isinstance(spans, dict) else spans, **kw) for v in values]


BIG = 1 << 20
NEXT_ABOVE = (3 << 8, 2796203 << 9)      # 3 * 2796203 = 2^23 + 1: the product is 2^40 + 2^17, one ulp above 2^40
GUARD_CASES: List[GuardCase] = [
    # ---- one entry just outside / on the lower limit, margin pools of every first-launch window ----
    *_twins("nuc8_first_tile", "nuc8_margin", (1,), "first_tile"),
    *_twins("nuc12_last_ref_col", "nuc12_margin", (0, 2), "last_ref_col"),
    *_twins("nuc16_first_tile", "nuc16_margin", (1,), "first_tile"),
    *_twins("nuc16_ref_first_tile", "nuc16_margin", (0,), "ref_first_tile"),
    *_twins("nuc16_last_ref_col", "nuc16_margin", (0, 2), "last_ref_col"),
    *_twins("nuc16_last_query_row", "nuc16_margin", (2,), "last_query_row"),
    *_twins("nuc16_gap_letter", "nuc16_margin", (0, 1), "gap_letter"),
    # marker 128: some twenty tiles per pair, the entry in a tile far behind the first (a tile runs on until its band has converged: the spans stay the committed ones)
    *_twins("nuc16_tile_behind", "nuc16_margin", (1,), "mid", marker=128),
    *_twins("prot8_gap_letter", "prot8_margin", (1,), "gap_letter"),
    *_twins("prot8_first_tile", "prot8_margin", (0, 2), "first_tile"),
    *_twins("prot16_last_query_row", "prot16_margin", (0, 2), "last_query_row"),
    *_twins("prot16_last_ref_col", "prot16_margin", (1,), "last_ref_col"),
    # ---- short pools: the tile-parallel and the precomputed-score routes, the upper limit, the denominators ----
    *_twins("short_nuc_first_tile", "short_nuc", (2, 5), "first_tile"),
    *_twins("short_nuc_tile_behind", "short_nuc", (3,), "gap_letter", marker=128),
    *_twins("short_nuc_tile_boundary", "short_nuc", (3,), "tile_boundary", marker=128),
    *_twins("short_prot_first_tile", "short_prot", (2, 5), "first_tile"),
    *_twins("short_prot_tile_behind", "short_prot", (3,), "gap_letter", marker=128),
    *_twins("short_nuc_hi", "short_nuc", (2, 5), "near_end", values=("above_hi", "hi")),
    *_twins("short_prot_hi", "short_prot", (2, 5), "near_end", values=("above_hi", "hi")),
    # denominators: 2^20 * 2^20 = 2^40 is accepted; (2^20 + 1) * 2^20 = 2^40 + 2^20 (exact in float32, eight ulps above 2^40) and NEXT_ABOVE, whose product
    # (2^23 + 1) * 2^17 is the very next float32 above 2^40, take the guard (scores of 1e-11: the gap penalties alone
    # shape the band, the spans are these cases' own)
    GuardCase(name="short_nuc_denom-2p40", pool="short_nuc", carriers=(1, 6), value=None, nums=((1, (BIG, BIG)), (6, (BIG, BIG))), spans=(2, 4, 2, 2, 2, 2, 4, 2)),
    GuardCase(name="short_nuc_denom-above_2p40", pool="short_nuc", carriers=(1, 6), value=None, nums=((1, (BIG + 1, BIG)), (6, NEXT_ABOVE)), spans=(2, 4, 2, 2, 2, 2, 4, 2), rerun=(1, 6)),
    GuardCase(name="short_prot_denom-2p40", pool="short_prot", carriers=(1, 6), value=None, nums=((1, (BIG, BIG)), (6, (BIG, BIG))), spans=(2, 4, 2, 2, 2, 2, 4, 2)),
    GuardCase(name="short_prot_denom-above_2p40", pool="short_prot", carriers=(1, 6), value=None, nums=((1, (BIG + 1, BIG)), (6, NEXT_ABOVE)), spans=(2, 4, 2, 2, 2, 2, 4, 2), rerun=(1, 6)),
    # refNum * qryNum == 1: the division by 1 is exact and the kernel does not take the vote -- an entry outside the range must NOT cause a re-run
    GuardCase(name="short_nuc_denom_one-below_lo", pool="short_nuc", carriers=(0,), where="first_tile", value="below_lo", nums=((0, (1, 1)),), spans=(1, 2, 2, 2, 2, 2, 2, 2), rerun=()),
    # ---- guard plus window: one changed entry in a pair of a just-over pool (the entry in query row 10: every kernel loads it in the pair's first tile) ----
    *_twins("nuc32_over_p0", "nuc32_over", (0,), "first_tile"),
    *_twins("nuc32_over_p1", "nuc32_over", (1,), "first_tile", values=("below_lo",)),
    *_twins("nuc72_margin_p1", "nuc72_margin", (1,), "first_tile", values=("below_lo",)),
    *_twins("prot16_over_p1", "prot16_over", (1,), "first_tile"),
    *_twins("prot16_over_p0", "prot16_over", (0,), "first_tile", values=("below_lo",)),
    *_twins("nuc16_margin_p1", "nuc16_margin", (1,), "first_tile", values=("below_lo",)),
]
GUARD_BY_NAME = {c.name: c for c in GUARD_CASES}

# The largest span of every TILE of the pools the guard-plus-window walk runs on (the oracle's trace; dp_cases commits the largest of a pair only).  The first tile
# holds the widest band of each of these pairs, and a tile that outgrows its window ends with the window's code BEFORE the vote on the guard is taken
# (talco_lean_kernel: `if (tile_err != 0) { err = tile_err; break; }` stands in front of it): a lean kernel reports the guard only from a window the first tile fits.
TILE_SPANS = {
    "nuc16_margin": ((15, 15, 7, 0), (14, 14, 7), (15, 15, 8)),
    "nuc32_over": ((31, 30, 24, 16, 8, 0), (32, 31, 23, 15, 7)),
    "nuc72_margin": ((70, 69, 65, 57, 49, 41, 33, 24, 16, 8, 0), (71, 71, 64, 56, 48, 40, 32, 24, 16, 8, 0)),
    "prot16_over": ((16, 15, 7), (15, 15, 7), (15, 14, 6)),
}
