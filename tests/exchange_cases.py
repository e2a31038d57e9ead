"""The exchange of a level's final paths between ranks (include/twl_level.h, twl_level_paths_to_block / twl_level_paths_from_block):
a restatement of the block layout of twilight_amd/csrc/host/exchange_plan.hpp, and the levels and ownerships of
tests/test_gpu_level_exchange.py with the class each pair exists for.

The layout here is held to the C++ function by tests/test_exchange_plan_cpu.py (a dump of tests/exchange_plan_kats.cpp on the same cases),
the classes of the levels to the level oracle by tests/test_exchange_inputs_cpu.py."""
from __future__ import annotations

import os
import struct
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import level_cases as LC  # noqa: E402
import level_oracle as LO  # noqa: E402

F = np.float32

MAGIC = 0x54574C44 << 32          # "TWLD"
HEAD = 32
SENTINEL = 0xEE                   # no path code (0, 1, 2)


def pad8(x: int) -> int:
    return (x + 7) & ~7


@dataclass
class Plan:
    mine: List[List[int]]
    hdr: List[int]
    hdr_max: int
    block_max: int


def plan(owner: Sequence[int], takes_part: Sequence[int], bound: Sequence[int], world: int, descending: Sequence[int] = ()) -> Plan:
    """planExchange; ranks listed in `descending` pack their pairs in descending pair order (the caller of the C ABI is free to: the layout
    is a function of the order of mine[r], every rank uses the same one)."""
    mine = [[i for i in range(len(owner)) if takes_part[i] and owner[i] == r] for r in range(world)]
    for r in descending:
        mine[r].reverse()
    hdr = [HEAD + 8 * len(m) for m in mine]
    caps = [hdr[r] + sum(pad8(int(bound[i])) for i in mine[r]) for r in range(world)]
    return Plan(mine, hdr, max(hdr), (max(caps) + 255) & ~255)


def row_offsets(pl: Plan, r: int, lens: Sequence[int]) -> Tuple[List[int], int]:
    """exchangeRowOffsets: lens[t] of the t-th pair of mine[r]; (offsets in r's block, end of the last path's padded room)."""
    at, off = pl.hdr[r], []
    for n in lens:
        off.append(at)
        at += pad8(max(0, int(n)))
    return off, at


def header_bytes(pl: Plan, r: int, words: Tuple[int, int, float, int], lens: Sequence[int], errs: Sequence[int]) -> bytes:
    """exchangeHeader: words = (band cells, relaunched, kernel ms, level number)."""
    h = struct.pack("<QQdQ", words[0], words[1], words[2], MAGIC | words[3])
    for n, e in zip(lens, errs):
        h += struct.pack("<ii", int(n), int(e))
    assert len(h) == pl.hdr[r]
    return h


def block_bytes(pl: Plan, r: int, words, lens: Sequence[int], errs: Sequence[int], paths: Sequence[Optional[np.ndarray]], fill: int = SENTINEL) -> bytes:
    """Rank r's whole block of block_max bytes over a buffer filled with `fill`: header, then every path at its offset; the pad bytes and
    everything behind the last path keep `fill`."""
    blk = bytearray([fill]) * pl.block_max
    h = header_bytes(pl, r, words, lens, errs)
    blk[: len(h)] = h
    off, end = row_offsets(pl, r, lens)
    assert end <= pl.block_max
    for t, n in enumerate(lens):
        if n > 0:
            p = np.asarray(paths[t], dtype=np.int8)
            assert len(p) == n
            blk[off[t]: off[t] + n] = p.tobytes()
    return bytes(blk)


# ---- fixed layout cases: tests/exchange_plan_kats.cpp holds its known answers on the first five, the dump is compared on all of them ----

def layout_cases() -> List[dict]:
    out = [
        dict(name="rank_owns_nothing", world=3, owner=[0, 2, 0, 2], takes=[1, 1, 1, 1], bound=[10, 20, 30, 40], lens=[10, 0, 7, 40], errs=[0, 3, 0, 0]),
        dict(name="one_rank_owns_all", world=2, owner=[1, 1, 1], takes=[1, 1, 1], bound=[8, 9, 7], lens=[8, 9, 1], errs=[0, 0, 0]),
        dict(name="pairs_take_no_part", world=2, owner=[0, 1, 0, 1, 0], takes=[1, 0, 0, 1, 1], bound=[5, 1000, 1000, 6, 7], lens=[5, 0, 0, 6, 0], errs=[0, 0, 0, 0, 0]),
        dict(name="pad8_lengths", world=1, owner=[0] * 5, takes=[1] * 5, bound=[0, 1, 7, 8, 9], lens=[0, 1, 7, 8, 9], errs=[0, 0, 0, 0, 0]),
        dict(name="block_rounding", world=2, owner=[0, 1, 1], takes=[1, 1, 1], bound=[216, 104, 105], lens=[216, 100, 105], errs=[0, 0, 0]),
        dict(name="empty_level", world=2, owner=[], takes=[], bound=[], lens=[], errs=[]),
    ]
    return out


def filler_path(pair: int, n: int) -> np.ndarray:
    """The path bytes both dumps put into a layout case's blocks."""
    return ((pair * 131 + np.arange(n)) % 3).astype(np.int8)


def dump_case(c: dict, words=(1234567890123, 42, 3.25, 7)) -> List[str]:
    """What `exchange_plan_kats --dump` prints for the case, from the restatement."""
    pl = plan(c["owner"], c["takes"], c["bound"], c["world"])
    lines = [f"case {c['name']} hdrMax {pl.hdr_max} blockMax {pl.block_max}"]
    for r in range(c["world"]):
        lens = [c["lens"][i] for i in pl.mine[r]]
        errs = [c["errs"][i] for i in pl.mine[r]]
        off, end = row_offsets(pl, r, lens)
        lines.append(f"rank {r} hdr {pl.hdr[r]} mine {' '.join(map(str, pl.mine[r]))} | off {' '.join(map(str, off))} | end {end}")
        lines.append("block " + block_bytes(pl, r, words, lens, errs, [filler_path(i, c["lens"][i]) for i in pl.mine[r]]).hex())
    return lines


def case_stdin(cases: List[dict]) -> str:
    """The cases in the plain text `exchange_plan_kats --dump` reads: name world n, then owner / takes / bound / lens / errs."""
    out = []
    for c in cases:
        out.append(f"{c['name']} {c['world']} {len(c['owner'])}")
        for k in ("owner", "takes", "bound", "lens", "errs"):
            out.append(" ".join(str(int(x)) for x in c[k]))
    return "\n".join(out) + "\n"


# ---- the levels of tests/test_gpu_level_exchange.py ----

LENGTHS = (1, 7, 8, 9, 255, 256, 257, 513)      # around pad8 and the 256-thread stride of the two copy kernels


@dataclass
class XPair:
    name: str
    case: LC.PairCase
    where: int                       # 1: no column removed, the DP path is final; 2: restored (or handed back and written by the owner); 0: takes no part
    final_len: Optional[int] = None  # exact length of the final path, where the pair exists for it
    hand_back: bool = False


@dataclass
class Ownership:
    name: str
    world: int
    owner: List[int]
    descending: Tuple[int, ...] = ()


@dataclass
class XLevel:
    seq_type: str
    pairs: List[XPair]
    thr: float = 0.95
    ownerships: List[Ownership] = field(default_factory=list)

    @property
    def cases(self):
        return [p.case for p in self.pairs]

    @property
    def takes_part(self):
        return [int(p.where != 0) for p in self.pairs]


def main_level(seq_type: str = "n", small: bool = False) -> XLevel:
    """About 24 pairs (small: 8) of at most 600 columns.  Kinds come in twos (1, 1, 2, 2, ...), so a round-robin deal over 2 ranks gives
    each rank interleaved rows of both kinds and a deal over 8 ranks gives each rank one kind only."""
    E = LC.make_edge_case
    seed = [700]

    def ident(**kw):
        seed[0] += 1
        return E(seq_type, seed[0], identical=True, **kw)

    def members(**kw):
        seed[0] += 1
        return E(seq_type, seed[0], **kw)

    plain = [XPair(f"plain{n}", ident(length=n), 1, n) for n in LENGTHS]
    restored = [
        XPair("lead_ref_7", ident(length=5, lead=(2, 0)), 2, 7),
        XPair("trail_qry_8", ident(length=6, trail=(0, 2)), 2, 8),
        XPair("run_ref_9", ident(length=6, runs=([(3, 3)], [])), 2, 9),
        XPair("run_ref_255", ident(length=250, runs=([(100, 5)], [])), 2, 255),
        XPair("lead_qry_256", ident(length=250, lead=(0, 6)), 2, 256),
        XPair("runs_257", ident(length=250, runs=([(50, 3)], [(120, 4)])), 2, 257),
        XPair("trail_ref_513", ident(length=500, trail=(13, 0)), 2, 513),
        XPair("longest_600", ident(length=520, runs=([(200, 80)], [])), 2, 600),        # the level's longest final path: exactly out_stride
    ]
    extra1 = [XPair("plain_members", members(members=(3, 2), length=(140, 150)), 1), XPair("plain_members_b", members(members=(2, 2), length=(61, 59)), 1)]
    extra2 = [XPair("hb_1x128", ident(length=80, trail=(1, 128)), 2, None, True),
              XPair("two_sided_3x3", ident(length=64, runs=([(33, 3)], [(33, 3)])), 2),
              XPair("members_4x2", members(members=(4, 2), length=(120, 130), trail=(0, 6), runs=([(50, 3)], [(60, 2)])), 2),
              XPair("two_sided_31x31", ident(length=90, lead=(31, 31)), 2)]
    no_part = XPair("no_part", ident(length=30, runs=([(10, 2)], [])), 0)
    if small:
        k1 = [plain[1], plain[4], plain[6], extra1[1]]
        k2 = [restored[1], extra2[0], restored[3], restored[5]]
        pairs = [k1[0], k1[1], k2[0], k2[1], no_part, k1[2], k1[3], k2[2], k2[3]]
    else:
        k1, k2 = plain + extra1, restored + extra2
        pairs = []
        for a in range(0, 10, 2):
            pairs += k1[a: a + 2] + k2[a: a + 2]
        pairs += [k2[10], k2[11]]
        pairs.insert(9, no_part)         # (an odd position: the deal of the pairs behind it shifts)
    lv = XLevel(seq_type, pairs)
    n = len(pairs)
    part = [i for i in range(n) if pairs[i].where]
    rr = lambda w: [part.index(i) % w if i in part else 0 for i in range(n)]      # (the pair that takes no part is dealt to rank 0: nobody packs it)
    lv.ownerships = [Ownership("w2_round_robin", 2, rr(2))]
    if not small:
        lv.ownerships += [
            Ownership("w3_rank1_owns_nothing_descending", 3, [2 * x for x in rr(2)], descending=(2,)),
            Ownership("w8_round_robin", 8, rr(8)),
            Ownership("w2_rank1_owns_all", 2, [1] * n),
        ]
    return lv


def second_level_pairs(lv: XLevel) -> List[Tuple[int, int]]:
    """Level 2 of the two-level run: (reference node, query node) as pair indices of level 1; every node is at most 257 columns long, so the
    level's out_stride and blocks are smaller than level 1's."""
    idx = {p.name: i for i, p in enumerate(lv.pairs)}
    names = [("plain7", "plain9"), ("lead_ref_7", "trail_qry_8"), ("plain255", "lead_qry_256"), ("run_ref_9", "plain8"), ("plain256", "run_ref_255"), ("runs_257", "plain257")]
    return [(idx[a], idx[b]) for a, b in names]


def kinds_per_rank(lv: XLevel, own: Ownership) -> Dict[int, List[int]]:
    """where (1 / 2) of the rows each rank packs, in block order."""
    pl = plan(own.owner, lv.takes_part, [0] * len(lv.pairs), own.world, own.descending)
    return {r: [lv.pairs[i].where for i in pl.mine[r]] for r in range(own.world)}


def node_side(pair: XPair, exp: dict) -> LC.SideCase:
    """The node a committed pair leaves behind, as a side of the next level: its rows after the write-back, the members' weights, and the
    merged profile the commit cached under the reference side's id."""
    c = pair.case
    gws = [c.sides[sd].group_weight for sd in range(2)]
    caches = [LO.cache_from_profile(LC.side_profile(c, sd), gws[sd], len(c.sides[sd].rows)) for sd in range(2)]
    merged = LO.update_frequency(caches[0], caches[1], exp["path_full"], gws[0], gws[1])
    return LC.SideCase(rows=list(exp["rows_after"]), seq_weights=np.concatenate([c.sides[0].seq_weights, c.sides[1].seq_weights]),
                       group_weight=float(F(F(gws[0]) + F(gws[1]))), cache=merged)


def second_level(lv: XLevel, exps: Sequence[dict]) -> List[LC.PairCase]:
    """The pair cases of level 2 from level 1's expected results (exps[i] of pair i)."""
    return [LC.PairCase(seq_type=lv.seq_type, thr=lv.thr, sides=[node_side(lv.pairs[a], exps[a]), node_side(lv.pairs[b], exps[b])], seed=900 + k)
            for k, (a, b) in enumerate(second_level_pairs(lv))]


def second_level_owner(lv: XLevel, own1: Ownership) -> List[int]:
    """Level 2's deal: every pair goes to the rank behind the one that aligned its reference node on level 1."""
    return [(own1.owner[a] + 1) % own1.world for a, _ in second_level_pairs(lv)]


# ---- a DP output row filled to one code below its pitch ----
# A DP path holds at least one match (its walk starts on one), so R + Q - 1 codes is the longest there is; it takes a pair without a second
# match worth taking: a reference of A, a query of C, and gaps (-1) cheaper than mismatches (-8).  With R = Q = seq_len the row of 2 * seq_len
# codes is full but for its last one.
GAP_ONLY = dict(gap_open=-1.0, gap_extend=-1.0)
GAP_ONLY_SIDE = 300


def gap_only_level() -> XLevel:
    def one(letter):
        return LC.SideCase(rows=[letter * GAP_ONLY_SIDE], seq_weights=np.array([1.0], dtype=F), group_weight=1.0)

    no_match = LC.PairCase(seq_type="n", thr=0.95, sides=[one(b"A"), one(b"C")], seed=990)
    pairs = [XPair("plain9_b", LC.make_edge_case("n", 991, identical=True, length=9), 1, 9),
             XPair("no_match_599", no_match, 1, 2 * GAP_ONLY_SIDE - 1),
             XPair("plain256_b", LC.make_edge_case("n", 992, identical=True, length=256), 1, 256)]
    return XLevel("n", pairs, ownerships=[Ownership("w2_middle_pair_alone", 2, [0, 1, 0])])
