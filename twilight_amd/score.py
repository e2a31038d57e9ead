"""ctypes binding of the affine sum-of-pairs score of a store's finished rows (C ABI: include/twl_score.h).  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence, Tuple

import numpy as np

from . import api
from .level import Store

_SYMBOLS = ["twl_store_score_rows", "twl_store_score_timing", "twl_score_describe"]

MAX_ROWS = 1 << 20      # TWL_SCORE_MAX_ROWS
TOTALS = ("R", "G", "RT", "GT", "letters")


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    return lib


def classes(seq_type: str) -> int:
    """K: the letter classes without "other"."""
    return {"n": 4, "p": 20}[seq_type]


def sub_index(K: int, a: int, b: int) -> int:
    """Where sub[a][b], a <= b <= K, lies in the table the call fills."""
    return a * (K + 1) - a * (a - 1) // 2 + (b - a)


def describe() -> Tuple[int, int, int, int]:
    """twl_score_describe: (words of a plane staged per step, rows of a pair tile's edge, rows of a counts row slice, rows per flush of the
    packed byte counters)."""
    out = (C.c_int32 * 4)()
    api._check(_lib().twl_score_describe(out))
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


def score_rows_raw(store, n_ids: int, ids, seq_type: str, sub_entries: int = 231, want_sub: bool = True, want_runs: bool = True, want_totals: bool = True):
    """twl_store_score_rows with the arguments as given (None: a null store or table); raises api.TwlError on a refusal."""
    idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    sub = np.full(max(1, sub_entries), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    runs = np.full(max(1, n_ids), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    totals = np.full(5, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    p64 = C.POINTER(C.c_uint64)
    api._check(_lib().twl_store_score_rows(None if store is None else store._h, C.c_int32(n_ids), None if idv is None else idv.ctypes.data_as(C.POINTER(C.c_int32)),
                                           C.c_char(seq_type.encode()[:1] or b"\0"), sub.ctypes.data_as(p64) if want_sub else None,
                                           runs.ctypes.data_as(p64) if want_runs else None, totals.ctypes.data_as(p64) if want_totals else None))
    return sub, runs, totals


def score_rows(store: Store, ids: Sequence[int], seq_type: str) -> Tuple[np.ndarray, np.ndarray, Dict[str, int]]:
    """The integers of the score of the listed rows (all of one current length): sub as a (K + 1) x (K + 1) table filled where a <= b,
    runs_row, and the totals R, G, RT, GT, letters."""
    K = classes(seq_type)
    flat, runs, totals = score_rows_raw(store, len(ids), list(ids), seq_type, (K + 1) * (K + 2) // 2)
    sub = np.zeros((K + 1, K + 1), dtype=np.uint64)
    for a in range(K + 1):
        for b in range(a, K + 1):
            sub[a, b] = flat[sub_index(K, a, b)]
    return sub, runs[:len(ids)], {k: int(v) for k, v in zip(TOTALS, totals)}


def score_ms(store: Store) -> Tuple[float, float, float]:
    """twl_store_score_timing: HIP-event times of the last call's pack, column and pair kernels."""
    ms = [C.c_double(0) for _ in range(3)]
    api._check(_lib().twl_store_score_timing(store._h, *[C.byref(m) for m in ms]))
    return tuple(float(m.value) for m in ms)
