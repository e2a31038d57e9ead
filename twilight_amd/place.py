"""ctypes binding of placement without a tree (C ABI: include/twl_place.h).  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import api
from .level import Store

_SYMBOLS = ["twl_store_count_columns", "twl_place_create", "twl_place_destroy", "twl_place_collect", "twl_place_finish", "twl_place_read_insertions"]


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        if name != "twl_place_destroy":
            getattr(lib, name).restype = C.c_int
    lib.twl_place_destroy.restype = None
    return lib


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def count_columns(store: Store, ids: Sequence[int], cache_id: int) -> None:
    """twl_store_count_columns: column counts of the rows `ids` (one length L) as the cached profile `cache_id`."""
    idv = _i32(list(ids))
    api._check(_lib().twl_store_count_columns(store._h, C.c_int32(len(idv)), idv.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(cache_id)))


class Placement:
    """A placement against a backbone of L columns on `store` (which must outlive it)."""

    def __init__(self, store: Store, L: int):
        self.store, self.L = store, int(L)
        self._h = C.c_void_p()
        api._check(_lib().twl_place_create(store._h, C.c_int32(self.L), C.byref(self._h)))
        store._dependants.append(self)      # whichever of the two is closed or collected first, the placement ends before its store

    def close(self):
        if self._h:
            _lib().twl_place_destroy(self._h)
            self._h = C.c_void_p()
            if self in self.store._dependants:
                self.store._dependants.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def collect_host(self, seq_ids: Sequence[int], paths: Sequence[np.ndarray]) -> None:
        """twl_place_collect with every path from the host (from_dp = NULL)."""
        n = len(seq_ids)
        stride = max([1] + [len(p) for p in paths])
        flat = np.zeros((max(n, 1), stride), dtype=np.int8)
        plen = np.zeros(max(n, 1), dtype=np.int32)
        for i, p in enumerate(paths):
            flat[i, : len(p)] = p
            plen[i] = len(p)
        ids = _i32(list(seq_ids) or [0])
        api._check(_lib().twl_place_collect(self._h, self.store._h, C.c_int32(n), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                            flat.ctypes.data_as(C.POINTER(C.c_int8)), plen.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(stride), None))

    def collect_level(self, seq_ids: Sequence[int], path_len: Sequence[int], stride: int, from_dp: Sequence[int],
                      paths: Optional[Sequence[Optional[np.ndarray]]] = None) -> None:
        """twl_place_collect on the store's prepared and aligned level: from_dp[i] 1 = DP output, 2 = path buffer, 0 = paths[i] (host)."""
        n = len(seq_ids)
        flat = np.zeros((max(n, 1), stride), dtype=np.int8)
        if paths is not None:
            for i, p in enumerate(paths):
                if p is not None:
                    flat[i, : len(p)] = p
        ids, plen = _i32(seq_ids), _i32(path_len)
        fd = np.ascontiguousarray(from_dp, dtype=np.uint8)
        api._check(_lib().twl_place_collect(self._h, self.store._h, C.c_int32(n), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                            flat.ctypes.data_as(C.POINTER(C.c_int8)), plen.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(stride),
                                            fd.ctypes.data_as(C.POINTER(C.c_uint8))))

    def insertions(self) -> np.ndarray:
        """twl_place_read_insertions: longest[0..L]."""
        out = np.zeros(self.L + 1, dtype=np.int32)
        api._check(_lib().twl_place_read_insertions(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def finish(self, backbone_ids: Sequence[int]) -> int:
        """twl_place_finish: every collected row and the backbone rows become rows of the final width W (returned)."""
        ids = _i32(list(backbone_ids) or [0])
        w = C.c_int32(0)
        api._check(_lib().twl_place_finish(self._h, C.c_int32(len(backbone_ids)), ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(w)))
        return int(w.value)
