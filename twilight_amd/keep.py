"""ctypes binding of the placement finish that keeps the backbone's length (C ABI: include/twl_keep.h).  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import api
from .place import Placement

_SYMBOLS = ["twl_place_finish_keep", "twl_place_dropped_counts", "twl_place_dropped_runs", "twl_place_keep_timing"]


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    return lib


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def finish_keep(pl: Placement) -> Tuple[int, int]:
    """twl_place_finish_keep: every collected sequence becomes a row of the backbone's L columns; (dropped runs, dropped letters) over all."""
    runs, letters = C.c_int64(-1), C.c_int64(-1)
    api._check(_lib().twl_place_finish_keep(pl._h, C.byref(runs), C.byref(letters)))
    return int(runs.value), int(letters.value)


def dropped_counts(pl: Placement, seq_ids: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """twl_place_dropped_counts: (runs int32 [n], letters int32 [n]).  Both arrays are followed by a guard element the call must leave alone."""
    ids = _i32(list(seq_ids))
    n = len(ids)
    runs = np.full(n + 1, -7, dtype=np.int32)
    letters = np.full(n + 1, -7, dtype=np.int32)
    api._check(_lib().twl_place_dropped_counts(pl._h, C.c_int32(n), _p32(ids) if n else None, _p32(runs), _p32(letters)))
    assert runs[n] == -7 and letters[n] == -7, "the call wrote behind its output"
    return runs[:n], letters[:n]


def dropped_runs(pl: Placement, seq_ids: Sequence[int], run_off=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """twl_place_dropped_runs: (run_off int64 [n + 1], col, qpos, len int32 [total]).  run_off defaults to the exclusive scan of the counts; the
    record arrays are followed by a guard element the call must leave alone."""
    ids = _i32(list(seq_ids))
    n = len(ids)
    if run_off is None:
        cnt = dropped_counts(pl, ids)[0] if n else np.zeros(0, np.int32)
        run_off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    off = np.ascontiguousarray(run_off, dtype=np.int64)
    total = int(off[-1]) if len(off) else 0
    out = [np.full(max(total, 0) + 1, -7, dtype=np.int32) for _ in range(3)]
    api._check(_lib().twl_place_dropped_runs(pl._h, C.c_int32(n), _p32(ids) if n else None, off.ctypes.data_as(C.POINTER(C.c_int64)), *[_p32(a) for a in out]))
    assert all(a[max(total, 0)] == -7 for a in out), "the call wrote behind its output"
    return off, out[0][:total], out[1][:total], out[2][:total]


def timing(pl: Placement) -> Tuple[float, float]:
    """twl_place_keep_timing: milliseconds of the rows kernel and of the runs kernels."""
    a, b = C.c_double(0), C.c_double(0)
    api._check(_lib().twl_place_keep_timing(pl._h, C.byref(a), C.byref(b)))
    return a.value, b.value
