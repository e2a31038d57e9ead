"""ctypes binding of the two-stage rebuilt guide tree's device side (C ABI: include/twl_retree_set.h): the rows of a finished alignment kept on
the device as bit-planes, every row assigned to its closest seed row, and the pair counts of groups of rows.  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import api

_SYMBOLS = ["twl_retree_set_describe", "twl_retree_set_create", "twl_retree_set_destroy", "twl_retree_set_letters", "twl_retree_set_assign",
            "twl_retree_set_pair_groups", "twl_retree_set_timing"]
SET_MAX_SEQS = 1048576


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    return lib


def describe() -> dict:
    """twl_retree_set_describe: the geometry of the kernels.  Needs no device."""
    out = (C.c_int32 * 4)()
    n = _lib().twl_retree_set_describe(out)
    api._check(min(n, 0))
    return {"assign_rows": out[0], "assign_seeds": out[1], "group_tile": out[2], "pack_rows": out[3]}


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class RetreeSet:
    """twl_retree_set_*: the bit-planes of the rows of an alignment kept on the device.  `rows` is a sequence of bytes of one width, or a
    C-contiguous uint8 array [n][width].  Use as a context manager, or call close()."""

    def __init__(self, rows, type_: str, max_gaps: int, device: int = 0):
        if isinstance(rows, np.ndarray):
            keep = np.ascontiguousarray(rows, dtype=np.uint8)
            self.n, width = keep.shape
            ptrs = (C.c_void_p * max(self.n, 1))(*(keep.ctypes.data + i * width for i in range(self.n)))
        else:
            keep = [bytes(r) for r in rows]
            self.n, width = len(keep), (len(keep[0]) if keep else 0)
            assert all(len(r) == width for r in keep), "the rows of an alignment have one width"
            ptrs = (C.c_char_p * max(self.n, 1))(*keep)
        self._lib = _lib()
        self._h = C.c_void_p()
        kept = C.c_int32(-1)
        api._check(self._lib.twl_retree_set_create(C.c_int(device), C.c_char(type_.encode()[:1] or b"\0"), C.c_int32(self.n), C.c_int32(width), ptrs, C.c_int32(max_gaps),
                                                   C.byref(self._h), C.byref(kept)))
        self.kept = kept.value

    def close(self):
        if self._h:
            api._check(self._lib.twl_retree_set_destroy(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def letters(self) -> np.ndarray:
        """twl_retree_set_letters: uint32 [n]."""
        out = np.full(self.n + 1, 0xFFFFFFFF, dtype=np.uint32)
        api._check(self._lib.twl_retree_set_letters(self._h, _u32(out)))
        assert out[self.n] == 0xFFFFFFFF, "the call wrote behind its output"
        return out[: self.n]

    def assign(self, seeds, want_counts: bool = True):
        """twl_retree_set_assign: (seed_out int32 [n], match_out, both_out uint32 [n] or None).  Every array is followed by a guard word the call
        must leave alone; it is checked here."""
        ids = np.ascontiguousarray(seeds, dtype=np.int32)
        seed = np.full(self.n + 1, -7, dtype=np.int32)
        match = np.full(self.n + 1, 0xFFFFFFFF, dtype=np.uint32) if want_counts else None
        both = np.full(self.n + 1, 0xFFFFFFFF, dtype=np.uint32) if want_counts else None
        api._check(self._lib.twl_retree_set_assign(self._h, C.c_int32(len(ids)), _i32(ids), _i32(seed), _u32(match) if want_counts else None, _u32(both) if want_counts else None))
        assert seed[self.n] == -7 and (not want_counts or (match[self.n] == 0xFFFFFFFF and both[self.n] == 0xFFFFFFFF)), "the call wrote behind its output"
        return seed[: self.n], (match[: self.n] if want_counts else None), (both[: self.n] if want_counts else None)

    def pair_groups(self, groups, guard_words: int = 0):
        """twl_retree_set_pair_groups: `groups` is a list of lists of row ids; returns the flat uint32 outputs (match, both), block after block,
        each followed by guard_words words of 0xFFFFFFFF that the call must leave alone."""
        off = np.zeros(len(groups) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(g) for g in groups])
        ids = np.ascontiguousarray([i for g in groups for i in g], dtype=np.int32)
        if len(ids) == 0:
            ids = np.zeros(1, dtype=np.int32)
        words = int(sum(len(g) ** 2 for g in groups))
        match = np.full(words + guard_words, 0xFFFFFFFF, dtype=np.uint32)
        both = np.full(words + guard_words, 0xFFFFFFFF, dtype=np.uint32)
        api._check(self._lib.twl_retree_set_pair_groups(self._h, C.c_int32(len(groups)), _i32(off), _i32(ids), _u32(match), _u32(both)))
        return match, both

    def timing(self) -> Tuple[float, float, float, float, float, float]:
        """twl_retree_set_timing: milliseconds of upload, gaps, pack, assign, groups and downloads since the set was made."""
        v = [C.c_double(0) for _ in range(6)]
        api._check(self._lib.twl_retree_set_timing(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)
