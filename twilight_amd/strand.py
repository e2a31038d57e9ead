"""ctypes binding of the strand calls (C ABI: include/twl_strand.h): opposite-strand k-mer counts and the direction of every sequence of a
guide.GuideSet.  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from . import api, guide

_SYMBOLS = ["twl_strand_rc_bin", "twl_guide_set_opposite", "twl_guide_set_strand_assign", "twl_guide_set_strand_timing"]


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib.twl_strand_rc_bin.restype = C.c_int32
    lib.twl_strand_rc_bin.argtypes = [C.c_int32]
    return lib


def rc_bin(b: int) -> int:
    """twl_strand_rc_bin: the code of the reverse complement of the 6-mer with code b, -1 outside 0 .. 4095.  Needs no device."""
    return int(_lib().twl_strand_rc_bin(int(b)))


def opposite(gset: guide.GuideSet, ids, guard_words: int = 0) -> np.ndarray:
    """twl_guide_set_opposite: uint32 [n_ids][n_ids].  With guard_words > 0 the flat buffer is returned instead, followed by that many words of
    0xFFFFFFFF that the call must leave alone."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    m = len(ids)
    flat = np.full(m * m + guard_words, 0xFFFFFFFF, dtype=np.uint32)
    api._check(_lib().twl_guide_set_opposite(gset._h, C.c_int32(m), ids.ctypes.data_as(C.POINTER(C.c_int32)), flat.ctypes.data_as(C.POINTER(C.c_uint32))))
    return flat if guard_words else flat.reshape(m, m)


def assign(gset: guide.GuideSet, seed_ids, seed_flip, want_shared: bool = True):
    """twl_guide_set_strand_assign: (seed_out int32 [n], dir_out uint8 [n], shared_out uint32 [n] or None).  Every array is followed by a guard
    element the call must leave alone; it is checked here."""
    ids = np.ascontiguousarray(seed_ids, dtype=np.int32)
    flip = np.ascontiguousarray(seed_flip, dtype=np.uint8)
    assert len(flip) == len(ids)
    n = gset.n
    seed = np.full(n + 1, -7, dtype=np.int32)
    dirs = np.full(n + 1, 0xEE, dtype=np.uint8)
    shared = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32) if want_shared else None
    api._check(_lib().twl_guide_set_strand_assign(gset._h, C.c_int32(len(ids)), ids.ctypes.data_as(C.POINTER(C.c_int32)), flip.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  seed.ctypes.data_as(C.POINTER(C.c_int32)), dirs.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  shared.ctypes.data_as(C.POINTER(C.c_uint32)) if want_shared else None))
    assert seed[n] == -7 and dirs[n] == 0xEE and (shared is None or shared[n] == 0xFFFFFFFF), "the call wrote behind its output"
    return seed[:n], dirs[:n], (shared[:n] if want_shared else None)


def timing(gset: guide.GuideSet) -> Tuple[float, float, float, float]:
    """twl_guide_set_strand_timing: milliseconds of the permute, assign and opposite kernels and of their downloads since the set was made."""
    v = [C.c_double(0) for _ in range(4)]
    api._check(_lib().twl_guide_set_strand_timing(gset._h, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)
