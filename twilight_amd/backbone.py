"""ctypes binding of the backbone squeeze of placement along a tree (C ABI: include/twl_backbone.h).  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import api
from .level import Store

_SYMBOLS = ["twl_store_squeeze_groups", "twl_store_squeeze_timing", "twl_squeeze_describe"]


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    return lib


def describe() -> Tuple[int, int, int]:
    """twl_squeeze_describe: (columns of a column tile, rows of a row slice, columns the scan walks per round)."""
    t, r, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    api._check(_lib().twl_squeeze_describe(C.byref(t), C.byref(r), C.byref(c)))
    return int(t.value), int(r.value), int(c.value)


def squeeze_groups_raw(store: Store, n_groups: int, group_off, ids, want_out: bool = True) -> np.ndarray:
    """twl_store_squeeze_groups with the tables as given (None: a null table); raises api.TwlError on a refusal."""
    off = None if group_off is None else np.ascontiguousarray(group_off, dtype=np.int32)
    idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    out = np.zeros(max(1, n_groups), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    api._check(_lib().twl_store_squeeze_groups(store._h, C.c_int32(n_groups), ptr(off), ptr(idv), ptr(out) if want_out else None))
    return out[:n_groups]


def squeeze_groups(store: Store, groups: Sequence[Sequence[int]]) -> List[int]:
    """Every group (a list of sequence ids of one current length) loses the columns in which all of its rows hold '-'; returns the kept length of each."""
    off = [0]
    ids: List[int] = []
    for g in groups:
        ids.extend(int(i) for i in g)
        off.append(len(ids))
    return [int(x) for x in squeeze_groups_raw(store, len(groups), off, ids or [0])]


def squeeze_ms(store: Store) -> float:
    """twl_store_squeeze_timing: HIP-event time of the last call's kernels."""
    ms = C.c_double(0)
    api._check(_lib().twl_store_squeeze_timing(store._h, C.byref(ms)))
    return float(ms.value)
