"""Randomized campaign on the tile-parallel path (long pairs, random markers, spoiled predictions, rounds, leads, both geometries) against
the oracle:  python tools/fuzz_mt.py START COUNT      (GPU box)
After every case that took the path without a re-run the level's tables are read back (twl_mt_tables) and held to tests/mt_oracle.py: the chain to the
restated chain of the scout samples (cases of one round), every record to the oracle's tile from the start it names."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import twilight_amd as twl
import mt_oracle as MO
import oracle_lib as O
from test_gpu_mt import check_mt_case, random_mt_case

start, count = int(sys.argv[1]), int(sys.argv[2])
twl.init([0])
twl.set_knob(twl.knobs.KNOB_POISON_TB, 1)      # a traceback word whose store was wrongly skipped must read as garbage, not as zeros
bad = took = errs = tabled = records = internal = 0
for seed in range(start, start + count):
    try:
        mt, e = check_mt_case(twl, seed)
        took += mt; errs += 1 if e else 0
        st = twl.get_stats(0)
        if mt and st.n_relaunched == 0:          # the tables are this level's (a re-run overwrites them)
            batch, matrix, pk, knobs = random_mt_case(seed)
            tb = twl.mt_tables(0)
            if tb["dims"]["rounds"] == 1:
                MO.check_chain(tb, batch.len, pk["marker"], knobs[twl.knobs.KNOB_MT_PERTURB])
            ok, failed, inner = MO.check_records(tb, MO.Tiles(O.make_params(matrix, **pk), batch))
            tabled += 1; records += ok + failed; internal += inner
    except AssertionError as ex:
        bad += 1
        print("FAIL", f"seed {seed}:", ex, flush=True)
print(f"seeds {start}..{start+count-1}: {bad} failures; {took} cases through the tile-parallel path, {errs} cases with algorithmic errorTypes; "
      f"tables of {tabled} levels read back, {records} records held to the oracle's tiles, {internal} with an internal re-run code not compared", flush=True)
sys.exit(1 if bad else 0)
