"""The tile-parallel kernels (talco_mt.hip.h: mt_anchor_kernel, mt_chain_kernel; talco_nuc.hip.h: the MT 2 scouts, the MT 1 tile jobs, the MT 3 stitch; launch_mt /
plan_tile_level on the host) where anchors, chain and records switch (-m gpu).

tests/test_gpu_mt.py holds whole levels to the oracle.  Here every case of tests/mt_cases.py (tests/test_mt_edge_inputs_cpu.py proves, without a GPU, that each
reaches the branch it is listed for) runs on both geometries of the scout and tile launches, and the tables the level left behind are read back
(twl_mt_tables) and held to the restatements of tests/mt_oracle.py and to single tiles of the oracle -- integers and bytes, no tolerance anywhere:

  a  results      errorType, path length, path bytes, band cells: the oracle's
  b  plan         dims and the pair of every table row
  c  anchors      every entry of every row, the -1 entries included
  d  chain        after one round, with every 0th / 1st / 2nd / 3rd prediction spoiled: the restated chain of the scout samples READ BACK from the device,
                  whatever the scouts found
  e  records      every record is the tile function of the start it names (next start, last flag, band cells, forward segment and tail; the errorType of a
                  failed one) -- records of starts off the path included
  f  adoption     the predicted / in-line counters are what the records at the true starts say; every round adds at least one such record
  g  front        every row done, its 64-bit cell count the pair's

Out of scope here: wide re-runs (the MT 4 pair scout and the 3072-row geometry: their mt_spath has another source) and the 512-row tile geometry.  Both depend on
what a pass remembers and have behavioural tests in tests/test_gpu_mt.py; the fixture below keeps a level off them."""
import numpy as np
import pytest

import mt_cases as MC
import mt_oracle as MO
import oracle_lib as O
from twilight_amd import api

pytestmark = pytest.mark.gpu

# (rounds, perturb): one round with every kind of spoiling for the chain, three rounds plain and with every second prediction spoiled
SETTINGS = [(1, 0), (1, 1), (1, 2), (1, 3), (3, 0), (3, 2)]


@pytest.fixture()
def knobs(gpu):
    gpu.set_knob(api.KNOB_THR_SMALL, 0)          # (also forgets what the levels of earlier tests found of the 512-row window)
    gpu.set_knob(api.KNOB_MT_WIDE, 0)            # (no wide-first start after a streak an earlier test left behind)
    yield gpu
    gpu.set_knob(api.KNOB_MT_PERTURB, 0)
    gpu.set_knob(api.KNOB_MT_MAX_PAIRS, 1024)
    gpu.set_knob(api.KNOB_MT_MIN_MARKER, 512)
    gpu.set_knob(api.KNOB_MT_LEAD, 320)
    gpu.set_knob(api.KNOB_MT_MARGIN, -1)
    gpu.set_knob(api.KNOB_MT_ROUNDS, 2)
    gpu.set_knob(api.KNOB_MT_THR_JOBS, 256)
    gpu.set_knob(api.KNOB_MT_WIDE, 1)
    gpu.set_knob(api.KNOB_THR_SMALL, 0)
    gpu.set_knob(api.KNOB_MT_ANCHOR, 1)
    gpu.set_knob(api.KNOB_MT_LEAD2, -1)


_REF = {}


def reference(name):
    """The oracle's side of a case, computed once: per pair its true starts, tiles, errorType, band cells and path; the tile function, remembered."""
    if name not in _REF:
        c = MC.case(name)
        op = O.make_params(c.matrix, **c.pk)
        tiles = MO.Tiles(op, c.batch)
        order = MO.launch_order(c.batch.len)
        pairs = {p: MO.true_starts(op, tiles.view(p)) for p in order}
        _REF[name] = dict(case=c, params=op, tiles=tiles, order=order, pairs=pairs)
    return _REF[name]


def run_level(twl, c, thr_jobs, rounds, perturb):
    for k, v in ((api.KNOB_MT_LEAD, 320), (api.KNOB_MT_LEAD2, -1), (api.KNOB_MT_MARGIN, -1), (api.KNOB_MT_ANCHOR, 1)):
        twl.set_knob(k, c.knob(k, v))
    twl.set_knob(api.KNOB_MT_MIN_MARKER, c.knob(api.KNOB_MT_MIN_MARKER))
    twl.set_knob(api.KNOB_MT_THR_JOBS, thr_jobs)
    twl.set_knob(api.KNOB_MT_ROUNDS, rounds)
    twl.set_knob(api.KNOB_MT_PERTURB, perturb)
    aln, n, err = twl.align_batch(twl.make_params(c.matrix, **c.pk), c.batch)
    st = twl.get_stats(0)
    cells = twl.get_pair_cells(c.batch.n_pairs)
    assert st.speculative == 3 and st.n_relaunched == 0, (st.speculative, st.n_relaunched, st.kernel)      # the tables are this level's
    return aln, n, err, st, cells, twl.mt_tables(0)


def check_level(ref, thr_jobs, rounds, perturb, aln, n, err, st, cells, tb):
    c, order, pairs, b = ref["case"], ref["order"], ref["pairs"], ref["case"].batch
    tag = f"{c.name} thr_jobs {thr_jobs} rounds {rounds} perturb {perturb}"
    # a. results
    for p in range(b.n_pairs):
        if p not in pairs:
            assert n[p] == 0 and err[p] == 0, f"{tag}: pair {p} does not run"
            continue
        _starts, _tiles, oerr, ocells, oaln = pairs[p]
        assert err[p] == oerr, f"{tag}: pair {p} errorType gpu {err[p]} oracle {oerr}"
        assert n[p] == oaln.shape[0] and np.array_equal(aln[p, : n[p]], oaln), f"{tag}: pair {p} path differs (gpu {n[p]} bytes, oracle {oaln.shape[0]})"
        assert int(cells[p]) == ocells, f"{tag}: pair {p} band cells gpu {cells[p]} oracle {ocells}"
    assert st.band_cells == sum(v[3] for v in pairs.values()), tag
    # b. plan
    pl = MO.plan(b.len, order, b.seq_len, c.marker, rounds=rounds, thr_jobs=thr_jobs, anchor=c.knob(api.KNOB_MT_ANCHOR, 1), lead2=c.knob(api.KNOB_MT_LEAD2),
                 marg=c.knob(api.KNOB_MT_MARGIN))
    assert tb["dims"] == pl["dims"], f"{tag}: dims device {tb['dims']} plan {pl['dims']}"
    assert tb["order"].tolist() == pl["order"], tag
    d = tb["dims"]
    # c. anchors
    if d["anchors"]:
        want = MO.anchor_table(b, pl, c.marker, d["lead2"])
        bad = np.argwhere(want != tb["anchor"])
        assert bad.shape[0] == 0, f"{tag}: anchors differ at (row, slot) {bad[:8].tolist()}: device {[int(tb['anchor'][r, s]) for r, s in bad[:8]]} restated {[int(want[r, s]) for r, s in bad[:8]]}"
    else:
        assert tb["anchor"] is None
    # d. chain
    if rounds == 1:
        MO.check_chain(tb, b.len, c.marker, perturb)
    # e. records
    ok, failed, internal = MO.check_records(tb, ref["tiles"])
    assert internal == 0, f"{tag}: {internal} records with an internal re-run code (the bands of these cases fit every window)"
    assert ok > 0, tag
    # f. adoption and counters
    hits_all = inline_lo = inline_hi = 0
    for row, p in enumerate(order):
        starts, tiles, oerr, _cells, _aln = pairs[p]
        rec = tb["rec"][row]
        hits = sum(1 for t in range(len(starts)) if rec[t, 0] == 1 and (int(rec[t, 1]), int(rec[t, 2])) == starts[t])
        hits_all += hits
        if oerr == 0:
            assert hits >= min(tiles, rounds), f"{tag}: pair {p}: {hits} records at true starts after {rounds} round(s), {tiles} tiles"
            inline_lo += tiles - hits
            inline_hi += tiles - hits
        else:      # the failing tile's record: state 2 at the true start, its code the pair's errorType
            t = tiles - 1
            at_true = (int(rec[t, 1]), int(rec[t, 2])) == starts[t] and rec[t, 0] != 0
            # (a spoiled prediction may leave the failing tile to the stitch launch, which then fails it in line: with perturb the record is only held to
            # its code where it names the true start; tile 0 always does)
            if perturb == 0 or t == 0:
                assert at_true, f"{tag}: pair {p} tile {t}: record {rec[t].tolist()}, true start {starts[t]}"
            if at_true:
                assert rec[t, 0] == 2 and rec[t, 10] == oerr == err[p], f"{tag}: pair {p} tile {t}: record {rec[t].tolist()}, errorType {oerr}"
            inline_hi += tiles - hits          # (tiles without a record at their true start, the failing one included when the stitch launch had to compute it)
    assert st.mt_tiles_predicted == hits_all, f"{tag}: predicted {st.mt_tiles_predicted}, records at true starts {hits_all}"
    assert inline_lo <= st.mt_tiles_inline <= inline_hi, f"{tag}: in line {st.mt_tiles_inline}, expected {inline_lo}..{inline_hi}"
    # g. front
    for row, p in enumerate(order):
        fr = tb["front"][row]
        assert fr[0] == 2, f"{tag}: row {row} front {fr.tolist()}"
        assert (int(np.uint32(fr[6])) | (int(np.uint32(fr[7])) << 32)) == pairs[p][3] == int(cells[p]), f"{tag}: row {row} front {fr.tolist()} cells {pairs[p][3]}"
    return ok, failed


@pytest.mark.parametrize("geometry", ["latency", "throughput"])
@pytest.mark.parametrize("name", MC.NAMES)
def test_tables_of_a_tile_parallel_level(knobs, name, geometry):
    ref = reference(name)
    c = ref["case"]
    thr_jobs = 0 if geometry == "throughput" else 1 << 20
    for rounds, perturb in SETTINGS:
        out = run_level(knobs, c, thr_jobs, rounds, perturb)
        ok, failed = check_level(ref, thr_jobs, rounds, perturb, *out)
        print(f"{name} {geometry} rounds {rounds} perturb {perturb}: {ok} records held to the oracle's tiles, {failed} failed ones; predicted {out[3].mt_tiles_predicted} in line {out[3].mt_tiles_inline} scouts failed {out[3].mt_scouts_failed}")
        if geometry == "throughput":
            assert out[5]["dims"]["thr"] == 1
        if c.batch.P == 22:
            assert out[3].matrix_mode == 4      # the records of the protein case come from tile jobs on the precomputed scores


def test_anchor_table_of_a_level_without_anchors_is_refused(knobs):
    """twl_mt_tables asked for the anchors of a level that ran without them, or for a device that was not selected: an error code, nothing copied."""
    import ctypes as C

    c = MC.case("long")                      # (runs with TWL_KNOB_MT_ANCHOR 0)
    run_level(knobs, c, 1 << 20, 1, 0)
    lib = api.load_library()
    dm = api.TwlMtDims()
    one = np.zeros(1, dtype=np.int32)
    rc = lib.twl_mt_tables(C.c_int(0), C.byref(dm), None, one.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None, None)
    assert rc == -2 and b"anchor" in lib.twl_last_error()
    assert lib.twl_mt_tables(C.c_int(7), C.byref(dm), None, None, None, None, None, None, None) == -2      # a device twl_init did not select
