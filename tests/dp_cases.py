"""Directed cases for the DP kernels: pairs whose band sits in the last two 64-row blocks of a kernel's row window, or just leaves it.

The window rule.  A register kernel of NV blocks (talco_lean_kernel: NV = waves x blocks per wave; talco_kernel likewise) holds the
rows [64 * (L >> 6), 64 * ((L >> 6) + NV)) of a diagonal whose band is [L, U].  In front of EVERY diagonal k it computes -- the test sits
at the top of the step in talco_kernel.hip.h and behind `++k`, guarded by `k < kEnd`, in talco_nuc.hip.h -- it tests, in this order:
band empty (errorType 1), `U - L + 1 > fLen` (errorType 2), `(U >> 6) - (L >> 6) >= NV` (the internal re-run code).  The band a tile
leaves behind its last diagonal (the tile ended by convergence, or the pair ended) is never tested.  So the limit is a span in blocks
from the band's first row, not a width: 449 rows always fit 8 blocks, 450 to 512 rows fit when L sits low enough in its block.

The oracle's trace hook (oracle/talco_oracle.c, tile_run) is called once per diagonal the oracle computes, behind the cell loop and in
front of the band update, with `Lk, Uk = L[k % 3], U[k % 3]`: the band OF DIAGONAL k, the one the two stop tests at the top of the loop
have just passed -- not the band of k + 1 that the update below the hook writes.  The diagonal on which the oracle stops with errorType
1 or 2 is not traced (the kernels test those two first as well), and neither is the band behind a tile's last diagonal.  So the pairs
that outgrow a window of NV blocks are exactly those with a trace record of span >= NV: `PairTrace.outgrows`.

Between `fcap = 64 * (NV - 2)` rows of width and the overflow talco_lean_kernel takes its wide-band branch (advance the blocks that
fell below the band before the activity test, reload their query rows, force a traceback flush).  A band of span NV - 2 or NV - 1 is
at least 64 * (NV - 3) + 1 ... wide and crosses fcap on the way; the MARGIN cases keep every pair there without leaving the window, the
JUST-OVER cases push at least one pair to span NV exactly (none beyond NV + 1) and leave the others in the margin.

Every X-drop below was searched on the CPU (bisection over X-drop: the span grows with it) and is a constant here; next to it are the
spans and widths the oracle gave.  tests/test_dp_edge_inputs_cpu.py recomputes them, tests/test_gpu_dp_edges.py runs the cases."""
from __future__ import annotations

import os
import sys
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
from twilight_amd import synth  # noqa: E402

# NV of every register window the dispatch has (twl_policy.inc.hip, rung_name; rows = 64 * NV)
NUC_WINDOWS = (8, 12, 16, 32, 48, 72)
PROT_WINDOWS = (8, 16)


def matrix_of(P: int) -> np.ndarray:
    return synth.nucleotide_matrix() if P == 6 else synth.protein_matrix()


def replicate(pool, idx):
    """The pairs `idx` of `pool` as a level of their own (a level of more pairs than CUs is the pool many times over)."""
    idx = np.asarray(idx)
    return synth.LevelBatch(P=pool.P, seq_len=pool.seq_len, freq=pool.freq[idx], gap_open=pool.gap_open[idx], gap_extend=pool.gap_extend[idx],
                            len=pool.len[idx], num=pool.num[idx])


@dataclass
class PairTrace:
    """What the oracle's trace says of one pair: per tile the largest block span and the largest width, and the pair's errorType."""
    err: int
    tile_span: List[int] = field(default_factory=list)
    tile_width: List[int] = field(default_factory=list)

    @property
    def span(self) -> int:
        return max(self.tile_span, default=0)

    @property
    def width(self) -> int:
        return max(self.tile_width, default=0)

    def outgrows(self, nv: int) -> bool:
        """A kernel with a window of `nv` blocks hands the pair back (see the module text: every traced diagonal is tested)."""
        return self.span >= nv


def trace_pair(batch, i: int, matrix: np.ndarray, **pk) -> PairTrace:
    """Pair `i` of `batch` through oracle_lib.align_pair with the trace hook."""
    R, Q = int(batch.len[i, 0]), int(batch.len[i, 1])
    P = batch.P
    spans: Dict[int, int] = {}
    widths: Dict[int, int] = {}

    def hook(_user, tile, _k, L, U, _score):
        s = (U >> 6) - (L >> 6)
        if s > spans.get(tile, -1):
            spans[tile] = s
        if U - L + 1 > widths.get(tile, -1):
            widths[tile] = U - L + 1

    _, err, _ = O.align_pair(O.make_params(matrix, **pk), batch.freq[i, 0, :R, :P], batch.freq[i, 1, :Q, :P], batch.gap_open[i, 0, :R],
                             batch.gap_extend[i, 0, :R], batch.gap_open[i, 1, :Q], batch.gap_extend[i, 1, :Q], int(batch.num[i, 0]), int(batch.num[i, 1]),
                             trace=hook)
    tiles = sorted(spans)
    return PairTrace(err=err, tile_span=[spans[t] for t in tiles], tile_width=[widths[t] for t in tiles])


@dataclass(frozen=True)
class DpCase:
    name: str
    P: int                               # 6 nucleotide, 22 protein
    nv: int                              # the window the case is about, in 64-row blocks (0: an fLen case, no window)
    kind: str                            # "margin" | "over" | "flen_ok" | "flen_stop"
    length: int                          # synth.make_level_batch(n, length, ...)
    n: int
    seed: int
    xdrop: int
    flen: int = 4096
    gen: Tuple[Tuple[str, object], ...] = (("members", ((1, 6), (1, 6))),)      # further arguments of make_level_batch
    pairs: Optional[Tuple[int, ...]] = None       # the pairs of that batch the pool keeps (None: all n)
    spans: Tuple[int, ...] = ()          # the oracle's largest span per pair ...
    widths: Tuple[int, ...] = ()         # ... and largest width
    errs: Optional[Tuple[int, ...]] = None        # errorType per pair (None: all 0)

    def batch(self):
        b = synth.make_level_batch(self.n, self.length, P=self.P, seed=self.seed, **dict(self.gen))
        return b if self.pairs is None else replicate(b, np.asarray(self.pairs))

    def params(self) -> dict:
        return dict(xdrop=self.xdrop, flen=self.flen)

    def traces(self, batch=None) -> List[PairTrace]:
        b = self.batch() if batch is None else batch
        with ThreadPoolExecutor(max_workers=4) as ex:      # (the oracle runs outside the interpreter lock; the hook is a few thousand calls per pair)
            return list(ex.map(lambda i: trace_pair(b, i, matrix_of(self.P), **self.params()), range(b.n_pairs)))

    def expected_errs(self) -> Tuple[int, ...]:
        return self.errs if self.errs is not None else (0,) * len(self.spans)


def outgrown(traces: List[PairTrace], nv: int) -> int:
    """How many pairs of the pool a window of `nv` blocks hands back."""
    return sum(1 for t in traces if t.outgrows(nv))


def check_case(case: DpCase, traces: List[PairTrace], batch) -> None:
    """The case is what it claims to be: raises AssertionError otherwise."""
    tag = f"{case.name}: spans {[t.span for t in traces]} widths {[t.width for t in traces]} errs {[t.err for t in traces]}"
    assert 2 <= len(traces) <= 6, tag
    assert tuple(t.err for t in traces) == case.expected_errs(), tag
    assert tuple(t.span for t in traces) == case.spans and tuple(t.width for t in traces) == case.widths, tag
    nv = case.nv
    if case.kind in ("margin", "over"):
        # fLen is min(flen, refLen, qLen) of a tile: it must not be what caps the band
        assert int(batch.len.min()) > 64 * nv and case.flen > 64 * (nv + 2), tag
    if case.kind == "margin":
        assert all(nv - 2 <= t.span <= nv - 1 for t in traces), tag
        # span NV - 1 means U - L >= 64 * (NV - 2) + 1 > fcap: at least one pair takes the wide-band branch
        assert any(t.span == nv - 1 and t.width > 64 * (nv - 2) for t in traces), tag
    elif case.kind == "over":
        over = [t for t in traces if t.span >= nv]
        assert any(t.span == nv for t in traces) and all(t.span <= nv + 1 for t in traces), tag
        assert all(nv - 2 <= t.span for t in traces) and len(over) >= 1, tag
    elif case.kind == "flen_ok":
        assert max(t.width for t in traces) == case.flen, tag
    elif case.kind == "flen_stop":
        assert case.errs is not None and 2 in case.errs, tag
    else:
        raise ValueError(case.kind)


# ---- the cases.  X-drop by bisection on the oracle; spans / widths are the oracle's, per pair of the pool ----
def _c(name, P, nv, kind, length, n, seed, xdrop, spans, widths, **kw):
    return DpCase(name=name, P=P, nv=nv, kind=kind, length=length, n=n, seed=seed, xdrop=xdrop, spans=spans, widths=widths, **kw)


CASES: List[DpCase] = [
    # nucleotide, 512 rows: 4 waves x 2 blocks
    _c("nuc8_margin", 6, 8, "margin", 1500, 3, 106, 4725, (7, 7, 7), (443, 420, 455)),
    _c("nuc8_over", 6, 8, "over", 1500, 3, 106, 4726, (7, 7, 8), (443, 420, 455)),
    # 768 rows: 4 waves x 3 blocks
    _c("nuc12_margin", 6, 12, "margin", 1500, 3, 106, 7520, (11, 10, 11), (690, 643, 707)),
    _c("nuc12_over", 6, 12, "over", 1500, 3, 106, 7521, (11, 10, 12), (690, 643, 707)),
    # 1024 rows: 8 waves x 2 blocks, 16 waves x 1 block
    _c("nuc16_margin", 6, 16, "margin", 1500, 3, 106, 10505, (15, 14, 15), (946, 890, 965)),
    _c("nuc16_over", 6, 16, "over", 1500, 3, 106, 10506, (15, 14, 16), (946, 890, 966)),
    # 2048 rows: 8 waves x 4 blocks (pair 1 of the batch is two blocks narrower than the others: left out)
    _c("nuc32_margin", 6, 32, "margin", 2500, 3, 106, 22403, (31, 31), (1949, 1991), pairs=(0, 2)),
    _c("nuc32_over", 6, 32, "over", 2500, 3, 106, 22404, (31, 32), (1949, 1991), pairs=(0, 2)),
    # 3072 rows: 16 waves x 3 blocks, tile-parallel
    _c("nuc48_margin", 6, 48, "margin", 3500, 2, 107, 33754, (47, 47), (2961, 3011)),
    _c("nuc48_over", 6, 48, "over", 3500, 2, 107, 33755, (47, 48), (2961, 3011)),
    # 4608 rows: 8 waves x 9 blocks (bands wider than the default fLen of 4096)
    _c("nuc72_margin", 6, 72, "margin", 5100, 2, 106, 50101, (70, 71), (4424, 4546), flen=8192),
    _c("nuc72_over", 6, 72, "over", 5100, 2, 106, 50102, (70, 72), (4424, 4546), flen=8192),
    # protein, 512 rows: 8 waves x 1 block (lean and round-1 kernels)
    _c("prot8_margin", 22, 8, "margin", 1500, 3, 106, 6078, (7, 7, 7), (443, 449, 455)),
    _c("prot8_over", 22, 8, "over", 1500, 3, 106, 6079, (7, 7, 8), (443, 449, 455)),
    # protein, 1024 rows: 16 waves x 1 block
    _c("prot16_margin", 22, 16, "margin", 1500, 3, 106, 13456, (15, 15, 15), (962, 958, 964)),
    _c("prot16_over", 22, 16, "over", 1500, 3, 106, 13457, (16, 15, 15), (962, 958, 964)),
]

# fLen: flen equal to the widest band of the pool passes, one less stops the widest pair with errorType 2 (`U - L + 1 > fLen`).
# Nucleotide: W = 455 lies inside the margin of the 512-row window (fcap = 384 < W, so the stop is found in the wide-band branch);
# protein: W = 308 lies below fcap (fcap = min(fLen, 384) = fLen: the one unsigned compare of the step is the fLen test itself).
FLEN_PAIRS: List[Tuple[DpCase, DpCase]] = [
    (_c("nuc_flen455", 6, 0, "flen_ok", 1500, 3, 106, 4725, (7, 7, 7), (443, 420, 455), flen=455),
     _c("nuc_flen454", 6, 0, "flen_stop", 1500, 3, 106, 4725, (7, 7, 7), (443, 420, 454), flen=454, errs=(0, 0, 2))),
    (_c("prot_flen308", 22, 0, "flen_ok", 1500, 3, 106, 4000, (5, 5, 5), (296, 307, 308), flen=308),
     _c("prot_flen307", 22, 0, "flen_stop", 1500, 3, 106, 4000, (5, 5, 5), (296, 307, 307), flen=307, errs=(0, 0, 2))),
]
CASES += [c for pair in FLEN_PAIRS for c in pair]
BY_NAME = {c.name: c for c in CASES}
