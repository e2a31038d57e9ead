"""ctypes binding of the subtree profile (C ABI: include/twl_subtree.h).  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import api
from .level import Store

_SYMBOLS = ["twl_store_weighted_columns"]


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    return lib


def weighted_columns(store: Store, ids: Sequence[int], weights: Sequence[float], cache_id: int) -> None:
    """twl_store_weighted_columns: the rows `ids` (one length L > 0), row t weighted by weights[t] and added in the order of `ids` in fp32,
    as the cached profile `cache_id`."""
    idv = np.ascontiguousarray(list(ids), dtype=np.int32)
    wv = np.ascontiguousarray(weights, dtype=np.float32)
    if wv.shape != idv.shape:
        raise ValueError("one weight per id")
    api._check(_lib().twl_store_weighted_columns(store._h, C.c_int32(len(idv)), idv.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 wv.ctypes.data_as(C.POINTER(C.c_float)), C.c_int32(cache_id)))
