"""ctypes binding of the guide tree's device side (C ABI: include/twl_guide.h): k-mer counts and shared k-mer counts.  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import api

_SYMBOLS = ["twl_guide_bins", "twl_guide_describe", "twl_guide_kmer_counts", "twl_guide_shared", "twl_guide_timing"]
MAX_SEQS = 16384


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib.twl_guide_bins.argtypes = [C.c_char]
    return lib


def bins(type_: str) -> int:
    """twl_guide_bins: 4096 for 'n', 7776 for 'p'.  Needs no device."""
    b = _lib().twl_guide_bins(type_.encode()[:1])
    api._check(min(b, 0))
    return b


def describe() -> dict:
    """twl_guide_describe: the geometry of the two kernels.  Needs no device."""
    out = (C.c_int32 * 4)()
    n = _lib().twl_guide_describe(out)
    api._check(min(n, 0))
    return {"count_chunk": out[0], "count_round": out[1], "pair_tile": out[2], "bin_slice": out[3]}


def _pack(seqs: Sequence[bytes]):
    keep = [bytes(s) for s in seqs]
    ptrs = (C.c_char_p * max(len(keep), 1))(*keep)
    lens = np.ascontiguousarray([len(s) for s in keep], dtype=np.int32)
    return keep, ptrs, lens


def kmer_counts(seqs: Sequence[bytes], type_: str, device: int = 0) -> np.ndarray:
    """twl_guide_kmer_counts: uint16 [n][bins]."""
    keep, ptrs, lens = _pack(seqs)
    out = np.zeros((len(keep), bins(type_)), dtype=np.uint16)
    api._check(_lib().twl_guide_kmer_counts(C.c_int(device), C.c_char(type_.encode()[:1]), C.c_int32(len(keep)), ptrs, lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                            out.ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


def shared(seqs: Sequence[bytes], type_: str, device: int = 0, guard_words: int = 0) -> np.ndarray:
    """twl_guide_shared: uint32 [n][n].  With guard_words > 0 the flat buffer is returned instead, n * n values followed by that many words
    of 0xFFFFFFFF that the call must leave alone."""
    keep, ptrs, lens = _pack(seqs)
    n = len(keep)
    flat = np.full(n * n + guard_words, 0xFFFFFFFF, dtype=np.uint32)
    api._check(_lib().twl_guide_shared(C.c_int(device), C.c_char(type_.encode()[:1]), C.c_int32(n), ptrs, lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                       flat.ctypes.data_as(C.POINTER(C.c_uint32))))
    return flat if guard_words else flat.reshape(n, n)


def timing(device: int = 0) -> Tuple[float, float, float]:
    """twl_guide_timing: milliseconds of upload + count, all pairs, download of the device's last shared()."""
    a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
    api._check(_lib().twl_guide_timing(C.c_int(device), C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value
