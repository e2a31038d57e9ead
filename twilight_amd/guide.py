"""ctypes binding of the guide tree's device side (C ABI: include/twl_guide.h): k-mer counts and shared k-mer counts.  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import api

_SYMBOLS = ["twl_guide_bins", "twl_guide_describe", "twl_guide_kmer_counts", "twl_guide_shared", "twl_guide_timing",
            "twl_guide_set_create", "twl_guide_set_destroy", "twl_guide_set_weights", "twl_guide_set_assign", "twl_guide_set_shared_groups", "twl_guide_set_timing"]
MAX_SEQS = 16384
SET_MAX_SEQS = 1048576


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


class GuideSet:
    """twl_guide_set_*: the k-mer counts of a set of sequences kept on the device (the two-stage guide tree).  Use as a context manager, or
    call close()."""

    def __init__(self, seqs: Sequence[bytes], type_: str, device: int = 0):
        keep, ptrs, lens = _pack(seqs)
        self.n = len(keep)
        self._lib = _lib()
        self._h = C.c_void_p()
        api._check(self._lib.twl_guide_set_create(C.c_int(device), C.c_char(type_.encode()[:1]), C.c_int32(self.n), ptrs, lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  C.byref(self._h)))

    def close(self):
        if self._h:
            api._check(self._lib.twl_guide_set_destroy(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def weights(self) -> np.ndarray:
        """twl_guide_set_weights: uint32 [n]."""
        out = np.zeros(self.n, dtype=np.uint32)
        api._check(self._lib.twl_guide_set_weights(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def assign(self, seed_ids, want_shared: bool = True):
        """twl_guide_set_assign: (seed_out int32 [n], shared_out uint32 [n] or None).  Both arrays are followed by a guard word the call must
        leave alone; it is checked here."""
        ids = np.ascontiguousarray(seed_ids, dtype=np.int32)
        seed = np.full(self.n + 1, -7, dtype=np.int32)
        shared = np.full(self.n + 1, 0xFFFFFFFF, dtype=np.uint32) if want_shared else None
        api._check(self._lib.twl_guide_set_assign(self._h, C.c_int32(len(ids)), ids.ctypes.data_as(C.POINTER(C.c_int32)), seed.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  shared.ctypes.data_as(C.POINTER(C.c_uint32)) if want_shared else None))
        assert seed[self.n] == -7 and (shared is None or shared[self.n] == 0xFFFFFFFF), "the call wrote behind its output"
        return seed[: self.n], (shared[: self.n] if want_shared else None)

    def shared_groups(self, groups, guard_words: int = 0) -> np.ndarray:
        """twl_guide_set_shared_groups: `groups` is a list of lists of sequence ids; returns the flat uint32 output, block after block, followed
        by guard_words words of 0xFFFFFFFF that the call must leave alone."""
        off = np.zeros(len(groups) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(g) for g in groups])
        ids = np.ascontiguousarray([i for g in groups for i in g], dtype=np.int32)
        if len(ids) == 0:
            ids = np.zeros(1, dtype=np.int32)
        words = int(sum(len(g) ** 2 for g in groups))
        out = np.full(words + guard_words, 0xFFFFFFFF, dtype=np.uint32)
        api._check(self._lib.twl_guide_set_shared_groups(self._h, C.c_int32(len(groups)), off.ctypes.data_as(C.POINTER(C.c_int32)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def timing(self) -> Tuple[float, float, float, float]:
        """twl_guide_set_timing: milliseconds of upload + count, assign, groups and downloads since the set was made."""
        v = [C.c_double(0) for _ in range(4)]
        api._check(self._lib.twl_guide_set_timing(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)
