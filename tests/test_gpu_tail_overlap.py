"""The tile-parallel remainder of a throughput level beside its bulk launch (first_throughput, TWL_KNOB_TAIL_OVERLAP) (-m gpu).

A nucleotide level of more than one round of persistent workgroups runs its full rounds on the throughput kernel and, when the last round would be
filled badly, the remainder through scouts / tiles / stitch (plan_nucleotide).  With the knob at 1 the remainder is launched on a stream of its own,
with its own traceback scratch and work counters, while the bulk kernel is still running; with 0 behind it on the call's stream.  Every case below
runs both ways through twl_align_batch_device, and every pair's path, length, error code and band cells are held to the CPU oracle -- never to the
other run; the two runs' pair counters (relaunched, tiles predicted / in line) must be equal.

Shapes: pairs of ~520-640 columns per side at marker 128 (TWL_KNOB_MT_MIN_MARKER 128; R + Q >= 8 * marker holds for every pair, which the
remainder rule asks), a few hundred thousand band cells each; a level is a pool of at most 16 distinct pairs replicated by index, the oracle aligns
the pool only.  Pair counts come from the device's CU count: a round is 5 * CUs pairs on the 512-row geometry (TWL_KNOB_THR_SMALL 2) and 4 * CUs on
the 768-row one (1).

The traceback scratch of every DP launch is filled with 0xFF bytes first (TWL_KNOB_POISON_TB 1): a remainder that shared the bulk's scratch would
overwrite the words of the running bulk."""
import numpy as np
import pytest

import dp_cases as DC
import oracle_lib as O
from twilight_amd import api, synth

pytestmark = pytest.mark.gpu

M = synth.nucleotide_matrix()
MARKER = 128


@pytest.fixture()
def knobs(gpu):
    gpu.set_knob(api.KNOB_POISON_TB, 1)
    gpu.set_knob(api.KNOB_MT_MIN_MARKER, MARKER)
    gpu.set_knob(api.KNOB_MT_WIDE, 1)
    yield gpu
    gpu.set_knob(api.KNOB_TAIL_OVERLAP, 1)
    gpu.set_knob(api.KNOB_MT_MIN_MARKER, 512)
    gpu.set_knob(api.KNOB_MT_MAX_PAIRS, 1024)
    gpu.set_knob(api.KNOB_MT_TAIL_PCT, 70)
    gpu.set_knob(api.KNOB_MT_PERTURB, 0)
    gpu.set_knob(api.KNOB_MT_ROUNDS, 2)
    gpu.set_knob(api.KNOB_ASSUME_ONEHOT_QUERY, 0)
    gpu.set_knob(api.KNOB_THR_SMALL, 0)


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def per_round(small):
    return (5 if small == 2 else 4) * cus()


_REF = {}


def reference(name, make_pool, **pk):
    """The pool of a case and what the oracle says of each of its pairs, computed once: (pool, paths, lengths, error codes, band cells per pair)."""
    if name not in _REF:
        pool = make_pool()
        assert pool.n_pairs <= 64
        oa, on, oerr, _ = O.align_batch(O.make_params(M, **pk), pool, threads=8)
        cells = np.array([O.align_batch(O.make_params(M, **pk), DC.replicate(pool, [i]))[3].cells for i in range(pool.n_pairs)], dtype=np.uint64)
        _REF[name] = (pool, oa, on, oerr, cells)
    return _REF[name]


def profile_pool():
    return synth.make_level_batch(16, 585, members=((1, 6), (1, 6)), seed=2201, length_jitter=0.07)


def leaf_pool():
    return synth.make_level_batch(16, 585, members=(1, 1), seed=2202, length_jitter=0.07)


class Level:
    """A level on the device: the pool's pairs `idx`, uploaded once and run as often as a case asks."""

    def __init__(self, pool, idx):
        import torch
        self.idx = np.asarray(idx)
        b = DC.replicate(pool, self.idx)
        self.n, self.sl = b.n_pairs, b.seq_len
        dev = torch.device("cuda:0")
        self.t = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k))).to(dev) for k in ("freq", "gap_open", "gap_extend", "len", "num")}
        self.aln = torch.zeros((self.n, 2 * self.sl), dtype=torch.int8, device=dev)
        self.alen = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.err = torch.zeros(self.n, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()

    def run(self, twl, p):
        import torch
        self.aln.fill_(7); self.alen.fill_(-5); self.err.fill_(7)      # (nothing of an earlier run may pass for this one's)
        torch.cuda.synchronize()
        t = self.t
        twl.align_batch_device(p, self.n, self.sl, t["freq"].data_ptr(), t["gap_open"].data_ptr(), t["gap_extend"].data_ptr(), t["len"].data_ptr(),
                               t["num"].data_ptr(), self.aln.data_ptr(), self.alen.data_ptr(), self.err.data_ptr())
        torch.cuda.synchronize()
        return self.aln.cpu().numpy(), self.alen.cpu().numpy(), self.err.cpu().numpy(), twl.get_stats(0), twl.get_pair_cells(self.n)


def hold_to_oracle(tag, level, ref, out):
    _pool, oa, on, oerr, ocells = ref
    aln, ln, err, st, cells = out
    idx = level.idx
    assert np.array_equal(err, oerr[idx]), f"{tag}: error codes differ at pairs {np.flatnonzero(err != oerr[idx])[:8].tolist()}"
    assert np.array_equal(ln, on[idx]), f"{tag}: path lengths differ at pairs {np.flatnonzero(ln != on[idx])[:8].tolist()}"
    assert np.array_equal(cells, ocells[idx]), f"{tag}: band cells differ at pairs {np.flatnonzero(cells != ocells[idx])[:8].tolist()}"
    for i in range(level.n):
        assert np.array_equal(aln[i, : ln[i]], oa[idx[i], : on[idx[i]]]), f"{tag}: pair {i} (pool pair {idx[i]}): path differs"
    assert st.band_cells == int(ocells[idx].sum()), tag


_COUNTERS = {}      # case -> [(relaunched, tiles predicted, tiles in line) with the remainder beside the bulk, ... behind it]


def both_ways(twl, tag, level, ref, p, small, expect_tail=True):
    """The level with the remainder beside the bulk and behind it, each held to the oracle.  Returns the stats of the two runs and remembers their pair counters."""
    seen = []
    for overlap in (1, 0):
        twl.set_knob(api.KNOB_TAIL_OVERLAP, overlap)
        twl.set_knob(api.KNOB_THR_SMALL, small)      # (also forgets what the level before found of the 512-row window)
        out = level.run(twl, p)
        st = out[3]
        print(f"{tag} overlap {overlap}: {level.n} pairs, kernel {bytes(st.kernel).split(bytes(1))[0].decode()}, {st.kernel_ms:.3f} ms, relaunched {st.n_relaunched}, "
              f"tiles predicted {st.mt_tiles_predicted} in line {st.mt_tiles_inline}, launches {st.n_launches}")
        hold_to_oracle(f"{tag} overlap {overlap}", level, ref, out)
        assert (b"<6, 4, 2" if small == 2 else b"<6, 4, 3") in bytes(st.kernel), (tag, st.kernel)
        if expect_tail:
            assert st.mt_tiles_predicted + st.mt_tiles_inline > 0, f"{tag}: the remainder did not take the tile-parallel path"
        seen.append(st)
    _COUNTERS[tag] = [(st.n_relaunched, st.mt_tiles_predicted, st.mt_tiles_inline) for st in seen]
    return seen


def largest_tail(small):
    return min(70 * per_round(small) // 100, 1024)


# (name, TWL_KNOB_THR_SMALL, full rounds, pairs of the remainder, one-letter sides, TWL_KNOB_MT_PERTURB, TWL_KNOB_MT_ROUNDS)
CASES = [
    ("one_pair_512", 2, 1, lambda: 1, 0, 0, 2),
    ("one_pair_768", 1, 1, lambda: 1, 0, 0, 2),
    ("twenty_512", 2, 1, lambda: 21, 0, 0, 2),
    ("twenty_768", 1, 1, lambda: 21, 0, 0, 2),
    ("largest_512", 2, 1, lambda: largest_tail(2), 0, 0, 2),
    ("largest_768", 1, 1, lambda: largest_tail(1), 0, 0, 2),
    ("two_rounds_768", 1, 2, lambda: 37, 0, 0, 2),
    ("leaf_512", 2, 1, lambda: 23, 1, 0, 2),
    ("leaf_768", 1, 1, lambda: 23, 1, 0, 2),
    ("spoiled_two_rounds", 1, 1, lambda: 29, 0, 3, 2),
    ("spoiled_one_round", 1, 1, lambda: 29, 0, 3, 1),
]


@pytest.mark.parametrize("small", [2, 1])
def test_two_calls_in_a_row_the_second_with_a_larger_remainder(knobs, small):
    """Every buffer of the remainder's side grows in the second call (tables, jobs, traceback scratch -- the first test of this file, so that the remainder's own
    scratch has not been grown by a larger level yet): nothing of the first call may still be using them, which is what the join in front of the first call's
    collect guarantees."""
    two_calls(knobs, small)


def two_calls(knobs, small):
    pk = dict(marker=MARKER)
    ref = reference("profile", profile_pool, **pk)
    p = knobs.make_params(M, **pk)
    levels = [Level(ref[0], np.arange(per_round(small) + t) % ref[0].n_pairs) for t in (3, largest_tail(small) // 2)]
    seen = {0: [], 1: []}
    for overlap in (1, 0):
        knobs.set_knob(api.KNOB_TAIL_OVERLAP, overlap)
        for which, level in enumerate(levels):
            knobs.set_knob(api.KNOB_THR_SMALL, small)
            out = level.run(knobs, p)
            st = out[3]
            print(f"two calls ({'512' if small == 2 else '768'} rows) overlap {overlap} call {which}: {level.n} pairs, {st.kernel_ms:.3f} ms, relaunched {st.n_relaunched}, "
                  f"tiles predicted {st.mt_tiles_predicted} in line {st.mt_tiles_inline}")
            hold_to_oracle(f"two calls, overlap {overlap}, call {which}", level, ref, out)
            assert st.mt_tiles_predicted + st.mt_tiles_inline > 0
            seen[which].append((st.n_relaunched, st.mt_tiles_predicted, st.mt_tiles_inline))
    for which in (0, 1):
        _COUNTERS[f"two_calls_{small}_call{which}"] = seen[which]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_remainder_beside_the_bulk_and_behind_it(knobs, name):
    run_case(knobs, name)


def run_case(knobs, name):
    _, small, rounds, tail, onehot, perturb, mt_rounds = next(c for c in CASES if c[0] == name)
    pk = dict(marker=MARKER)
    ref = reference("leaf" if onehot else "profile", leaf_pool if onehot else profile_pool, **pk)
    n = rounds * per_round(small) + tail()
    level = Level(ref[0], np.arange(n) % ref[0].n_pairs)
    knobs.set_knob(api.KNOB_ASSUME_ONEHOT_QUERY, onehot)
    knobs.set_knob(api.KNOB_MT_PERTURB, perturb)
    knobs.set_knob(api.KNOB_MT_ROUNDS, mt_rounds)
    on, off = both_ways(knobs, name, level, ref, knobs.make_params(M, **pk), small)
    assert on.matrix_mode == off.matrix_mode == (5 if onehot else 2), (on.matrix_mode, off.matrix_mode)
    if perturb:      # every third predicted start spoiled: the stitch launches have tiles to compute in line (one round) or a second round to run
        assert on.mt_tiles_inline > 0 or mt_rounds > 1, (on.mt_tiles_predicted, on.mt_tiles_inline)


def test_a_bulk_pair_and_a_remainder_pair_outgrow_the_window(knobs):
    """The pool of tests/dp_cases.py's nuc8_over (three pairs of ~1500 columns; with X-drop 4726 one of them reaches a band of 8 blocks and leaves the 512-row
    window, whatever the marker: the band is not reset between tiles) as a level on the 512-row geometry in which that pair stands on both sides of the
    split: once at the end of the bulk, once at the head of the remainder.  The bulk's copy comes back with the re-run code and climbs the ladder (768 rows),
    which reads the error codes behind the join; the remainder's copy has the tile that outgrows the window computed in line by its stitch launch."""
    outgrown_case(knobs)


def outgrown_case(knobs):
    case = DC.BY_NAME["nuc8_over"]
    pk = dict(case.params(), marker=MARKER)
    ref = reference("nuc8_over", case.batch, **pk)
    pool = ref[0]
    traces = case.traces(pool)
    out8 = [i for i, t in enumerate(traces) if t.outgrows(8)]
    assert len(out8) == 1 and all(t.err == 0 for t in traces), [t.span for t in traces]
    by_cost = np.argsort(-pool.len.sum(axis=1), kind="stable").tolist()       # the launch order: longest first
    at = by_cost.index(out8[0])
    assert len(set(pool.len.sum(axis=1).tolist())) == pool.n_pairs and 0 < at < pool.n_pairs - 1, pool.len.tolist()
    bulk, tail = per_round(2), 40
    longer, shorter = by_cost[:at], by_cost[at + 1:]
    idx = [longer[t % len(longer)] for t in range(bulk - 1)] + [out8[0]] * 2 + [shorter[t % len(shorter)] for t in range(tail - 1)]
    # (the same stable sort puts the first copy of the pair at position bulk - 1 and the second at position bulk)
    order = np.argsort(-pool.len.sum(axis=1)[idx], kind="stable")
    assert idx[order[bulk - 1]] == idx[order[bulk]] == out8[0] and len(idx) == bulk + tail
    level = Level(pool, idx)
    on, off = both_ways(knobs, "outgrown", level, ref, knobs.make_params(M, **pk), 2)
    assert on.n_relaunched >= 1, on.n_relaunched


COUNTER_CASES = [c[0] for c in CASES] + ["outgrown"] + [f"two_calls_{small}_call{which}" for small in (2, 1) for which in (0, 1)]


@pytest.mark.parametrize("name", COUNTER_CASES)
def test_pair_counters_are_equal_both_ways(knobs, name):
    """relaunched, tiles predicted and tiles in line of the run with the remainder beside the bulk and of the run with it behind (the runs of the tests above,
    made here when a test is run alone).

    Both are functions of the level alone.  (They were not while a scout's share of the traceback scratch was sized by the level's marker: at marker 128 a
    scout, which keeps words up to its own longer marker, wrote into the next workgroup's share, and the split between predicted and in line differed from run to
    run -- 6557 / 60, 6572 / 45, 6554 / 63, 6563 / 54 for largest_768 behind the bulk, 6352 / 265 beside it; launch_mt_kernel.  With the share sized for the scout
    every start of largest_768 is predicted: 6617 / 0 both ways.)"""
    if name not in _COUNTERS:
        if name.startswith("two_calls"):
            two_calls(knobs, int(name.split("_")[2]))
        elif name == "outgrown":
            outgrown_case(knobs)
        else:
            run_case(knobs, name)
    beside, behind = _COUNTERS[name]
    print(f"{name}: (relaunched, predicted, in line) beside {beside} behind {behind}")
    assert beside[0] == behind[0] and beside[1] + beside[2] == behind[1] + behind[2], (name, beside, behind)
    assert beside == behind, (name, beside, behind)
