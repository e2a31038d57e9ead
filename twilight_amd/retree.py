"""ctypes binding of the rebuilt guide tree's device side (C ABI: include/twl_retree.h): gap counts of the columns and pair counts of the rows
of a finished alignment.  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import api

_SYMBOLS = ["twl_retree_describe", "twl_retree_column_gaps", "twl_retree_pair_counts", "twl_retree_timing"]
MAX_SEQS = 16384


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    return lib


def describe() -> dict:
    """twl_retree_describe: the geometry of the kernels.  Needs no device."""
    out = (C.c_int32 * 4)()
    n = _lib().twl_retree_describe(out)
    api._check(min(n, 0))
    return {"word_columns": out[0], "pair_tile": out[1], "slice_words": out[2], "gap_rows": out[3]}


def _pack(rows: Sequence[bytes]):
    keep = [bytes(r) for r in rows]
    width = len(keep[0]) if keep else 0
    assert all(len(r) == width for r in keep), "the rows of an alignment have one width"
    ptrs = (C.c_char_p * max(len(keep), 1))(*keep)
    return keep, ptrs, width


def column_gaps(rows: Sequence[bytes], device: int = 0, guard_words: int = 0) -> np.ndarray:
    """twl_retree_column_gaps: uint32 [width], followed by guard_words words of 0xFFFFFFFF that the call must leave alone."""
    keep, ptrs, width = _pack(rows)
    out = np.full(width + guard_words, 0xFFFFFFFF, dtype=np.uint32)
    api._check(_lib().twl_retree_column_gaps(C.c_int(device), C.c_int32(len(keep)), C.c_int32(width), ptrs, out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def pair_counts(rows: Sequence[bytes], type_: str, max_gaps: int, device: int = 0, guard_words: int = 0):
    """twl_retree_pair_counts: (match, both, kept): uint32 [n][n] each and the number of kept columns.  With guard_words > 0 the two flat buffers
    are returned instead, n * n values each followed by that many words of 0xFFFFFFFF that the call must leave alone."""
    keep, ptrs, width = _pack(rows)
    n = len(keep)
    match = np.full(n * n + guard_words, 0xFFFFFFFF, dtype=np.uint32)
    both = np.full(n * n + guard_words, 0xFFFFFFFF, dtype=np.uint32)
    kept = C.c_int32(-1)
    api._check(_lib().twl_retree_pair_counts(C.c_int(device), C.c_char(type_.encode()[:1] or b"\0"), C.c_int32(n), C.c_int32(width), ptrs, C.c_int32(max_gaps),
                                             match.ctypes.data_as(C.POINTER(C.c_uint32)), both.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(kept)))
    if guard_words:
        return match, both, kept.value
    return match.reshape(n, n), both.reshape(n, n), kept.value


def timing(device: int = 0) -> Tuple[float, float, float, float, float]:
    """twl_retree_timing: milliseconds of upload, gaps, pack, pairs, download of the device's last pair_counts()."""
    v = [C.c_double(0) for _ in range(5)]
    api._check(_lib().twl_retree_timing(C.c_int(device), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)
