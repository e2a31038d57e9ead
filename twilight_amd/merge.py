"""ctypes binding of the merge of existing alignments (C ABI: include/twl_merge.h).  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import api
from .level import Store

_SYMBOLS = ["twl_merge_create", "twl_merge_destroy", "twl_merge_apply", "twl_merge_finish", "twl_merge_read_map", "twl_merge_timing"]


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        if name != "twl_merge_destroy":
            getattr(lib, name).restype = C.c_int
    lib.twl_merge_destroy.restype = None
    return lib


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    for i, l in enumerate(lists):
        off[i + 1] = off[i] + len(l)
    flat = _i32([x for l in lists for x in l] or [0])
    return off, flat


class Merge:
    """The column maps of the groups `groups` (lists of store ids, the rows of one input alignment each) on `store`, which must outlive it."""

    def __init__(self, store: Store, groups: Sequence[Sequence[int]]):
        self.store = store
        self.lengths = None
        self._h = C.c_void_p()
        off, ids = _csr(groups)
        self.n_groups = len(groups)
        api._check(_lib().twl_merge_create(store._h, C.c_int32(self.n_groups), _p32(off), _p32(ids), C.byref(self._h)))
        store._dependants.append(self)      # whichever of the two is closed or collected first, the merge ends before its store
        rows = store.rows_of([g[0] for g in groups]) if groups else []
        self.lengths = [len(r) for r in rows]

    def close(self):
        if self._h:
            _lib().twl_merge_destroy(self._h)
            self._h = C.c_void_p()
            if self in self.store._dependants:
                self.store._dependants.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply_host(self, ref_groups: Sequence[Sequence[int]], qry_groups: Sequence[Sequence[int]], paths: Sequence[np.ndarray]) -> None:
        """twl_merge_apply with every path from the host (from_dp = NULL): pair i has the groups ref_groups[i] / qry_groups[i] under its sides."""
        n = len(paths)
        stride = max([1] + [len(p) for p in paths])
        flat = np.zeros((max(n, 1), stride), dtype=np.int8)
        plen = np.zeros(max(n, 1), dtype=np.int32)
        for i, p in enumerate(paths):
            flat[i, : len(p)] = p
            plen[i] = len(p)
        roff, rg = _csr(ref_groups)
        qoff, qg = _csr(qry_groups)
        api._check(_lib().twl_merge_apply(self._h, self.store._h, C.c_int32(n), _p32(roff), _p32(rg), _p32(qoff), _p32(qg),
                                          flat.ctypes.data_as(C.POINTER(C.c_int8)), _p32(plen), C.c_int32(stride), None))

    def apply_level(self, ref_groups, qry_groups, path_len: Sequence[int], stride: int, from_dp: Sequence[int],
                    paths: Optional[Sequence[Optional[np.ndarray]]] = None) -> None:
        """twl_merge_apply on the store's prepared and aligned level: from_dp[i] 1 = DP output, 2 = path buffer, 0 = paths[i] (host)."""
        n = len(path_len)
        roff, rg = _csr(ref_groups)
        qoff, qg = _csr(qry_groups)
        plen = _i32(path_len)
        fd = np.ascontiguousarray(from_dp, dtype=np.uint8)
        flat = None
        if paths is not None:
            flat = np.zeros((max(n, 1), stride), dtype=np.int8)
            for i, p in enumerate(paths):
                if p is not None:
                    flat[i, : len(p)] = p
        api._check(_lib().twl_merge_apply(self._h, self.store._h, C.c_int32(n), _p32(roff), _p32(rg), _p32(qoff), _p32(qg),
                                          flat.ctypes.data_as(C.POINTER(C.c_int8)) if flat is not None else None, _p32(plen), C.c_int32(stride),
                                          fd.ctypes.data_as(C.POINTER(C.c_uint8))))

    def map(self, g: int) -> np.ndarray:
        """twl_merge_read_map: pos_g[0, L_g)."""
        out = np.zeros(max(self.lengths[g], 1), dtype=np.int32)
        api._check(_lib().twl_merge_read_map(self._h, C.c_int32(g), _p32(out)))
        return out[: self.lengths[g]]

    def timing(self):
        """twl_merge_timing: HIP-event ms of (every apply so far, the finish, the finish's row rewrite alone)."""
        a, f, r = C.c_double(0), C.c_double(0), C.c_double(0)
        api._check(_lib().twl_merge_timing(self._h, C.byref(a), C.byref(f), C.byref(r)))
        return a.value, f.value, r.value

    def finish(self) -> int:
        """twl_merge_finish: every row of every group becomes a row of the final width W (returned)."""
        w = C.c_int32(0)
        api._check(_lib().twl_merge_finish(self._h, C.byref(w)))
        return int(w.value)
