"""ctypes binding of the column trim of a store's finished rows (C ABI: include/twl_trim.h).  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import api
from .level import Store

_SYMBOLS = ["twl_store_trim_columns", "twl_store_trim_read", "twl_store_trim_timing", "twl_trim_describe"]

MAX_GAPS = 0      # TWL_TRIM_MAX_GAPS
TO_ROW = 1        # TWL_TRIM_TO_ROW


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    return lib


def describe() -> Tuple[int, int, int, int]:
    """twl_trim_describe: (columns of a column tile, rows of a counts row slice, columns the scan walks per round, rows per flush of the
    packed byte counters)."""
    out = (C.c_int32 * 4)()
    api._check(_lib().twl_trim_describe(out))
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


def trim_columns_raw(store, n_ids: int, ids, rule: int, arg: int, want_out: bool = True) -> int:
    """twl_store_trim_columns with the arguments as given (None: a null store or table); raises api.TwlError on a refusal."""
    idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    kept = C.c_int32(-1)
    api._check(_lib().twl_store_trim_columns(None if store is None else store._h, C.c_int32(n_ids), None if idv is None else idv.ctypes.data_as(C.POINTER(C.c_int32)),
                                             C.c_int32(rule), C.c_int32(arg), C.byref(kept) if want_out else None))
    return int(kept.value)


def trim_columns(store: Store, ids: Sequence[int], rule: int, arg: int) -> int:
    """Every listed row (all of one current length) becomes its kept columns; returns the kept count.  rule MAX_GAPS: a column is kept iff at
    most `arg` listed rows hold '-' there; rule TO_ROW: iff the row of sequence `arg` holds anything but '-' there."""
    return trim_columns_raw(store, len(ids), list(ids) or None, rule, arg)


def trim_read(store: Store, width: int, kept: int) -> Tuple[np.ndarray, np.ndarray]:
    """twl_store_trim_read: (the kept columns' original indices, the gap count of every original column) of the last trim, whose width and
    kept count the caller names."""
    cols = np.full(max(1, kept), -1, dtype=np.int32)
    gaps = np.full(max(1, width), 0xFFFFFFFF, dtype=np.uint32)
    api._check(_lib().twl_store_trim_read(store._h, cols.ctypes.data_as(C.POINTER(C.c_int32)), gaps.ctypes.data_as(C.POINTER(C.c_uint32))))
    return cols[:kept], gaps[:width]


def trim_read_raw(store, cols: bool = False, gaps: bool = False) -> None:
    """twl_store_trim_read with null tables unless asked otherwise (the refusals)."""
    c = np.zeros(1, dtype=np.int32) if cols else None
    g = np.zeros(1, dtype=np.uint32) if gaps else None
    api._check(_lib().twl_store_trim_read(None if store is None else store._h, None if c is None else c.ctypes.data_as(C.POINTER(C.c_int32)),
                                          None if g is None else g.ctypes.data_as(C.POINTER(C.c_uint32))))


def trim_ms(store: Store) -> float:
    """twl_store_trim_timing: HIP-event time of the last call's kernels."""
    ms = C.c_double(0)
    api._check(_lib().twl_store_trim_timing(store._h, C.byref(ms)))
    return float(ms.value)
