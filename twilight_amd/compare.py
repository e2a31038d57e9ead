"""ctypes binding of the comparison of an alignment with a reference alignment (C ABI: include/twl_compare.h).  No fallback path."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import api

_SYMBOLS = ["twl_compare_create", "twl_compare_columns", "twl_compare_timing", "twl_compare_describe", "twl_compare_destroy"]


def exported_symbols():
    return list(_SYMBOLS)


def _lib():
    lib = api.load_library()
    for name in _SYMBOLS:
        getattr(lib, name).restype = C.c_int
    return lib


def describe() -> Tuple[int, int, int, int]:
    """twl_compare_describe: (counters per key window T, columns of a column tile, rows a workgroup takes per step of the column kernel,
    columns the row scans walk per round).  No device needed."""
    out = (C.c_int32 * 4)()
    api._check(_lib().twl_compare_describe(out))
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


def _row_table(rows: Optional[Sequence[bytes]]):
    """(the pointer table, what keeps its rows alive): every row in a buffer of exactly its own length, so nothing behind it belongs to it."""
    if rows is None:
        return None, None
    keep = [C.create_string_buffer(bytes(r), max(1, len(r))) for r in rows]
    table = (C.c_void_p * max(1, len(keep)))(*[C.addressof(b) for b in keep])
    return table, keep


class BadRow(api.TwlError):
    """twl_compare_create refused a row: .row is the smallest row whose letter count or letters differ."""

    def __init__(self, message: str, row: int):
        super().__init__(message)
        self.row = row


def create_raw(n: int, w_est: int, est: Optional[Sequence[bytes]], w_ref: int, ref: Optional[Sequence[bytes]], device: int = 0, want_cmp: bool = True, want_bad: bool = True):
    """twl_compare_create with the arguments as given (None: a null table); returns (handle, bad_row); raises on a refusal."""
    te, ke = _row_table(est)
    tr, kr = _row_table(ref)
    h = C.c_void_p(None)
    bad = C.c_int32(-2)
    rc = _lib().twl_compare_create(C.c_int(device), C.c_int32(n), C.c_int32(w_est), te, C.c_int32(w_ref), tr, C.byref(h) if want_cmp else None, C.byref(bad) if want_bad else None)
    if rc != 0:
        assert not h.value, "a refused twl_compare_create left a handle"
        msg = f"libtwl_align error {rc}: {api.load_library().twl_last_error().decode()}"
        if bad.value >= 0:
            raise BadRow(msg, int(bad.value))
        raise api.TwlError(msg)
    return h, int(bad.value)


class Compare:
    """An estimate and a reference alignment of the same rows on the device (twl_compare_create): rows are bytes of one width per alignment."""

    def __init__(self, est: Sequence[bytes], ref: Sequence[bytes], device: int = 0):
        assert len(est) == len(ref)
        self.n = len(est)
        self.w_est = len(est[0]) if est else 0
        self.w_ref = len(ref[0]) if ref else 0
        assert all(len(r) == self.w_est for r in est) and all(len(r) == self.w_ref for r in ref)
        self._h, _ = create_raw(self.n, self.w_est, est, self.w_ref, ref, device)

    def columns(self, guard_words: int = 0) -> Dict[str, np.ndarray]:
        """twl_compare_columns: shared uint64 [w_est], letters, distinct uint32 [w_est], recovered uint8 [w_est], ref_letters uint32 [w_ref].
        With guard_words > 0 every array is followed by that many poisoned elements, which the call must leave alone (asserted here)."""
        g = guard_words
        out = {"shared": np.full(self.w_est + g, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), "letters": np.full(self.w_est + g, 0xA5A5A5A5, dtype=np.uint32),
               "distinct": np.full(self.w_est + g, 0xA5A5A5A5, dtype=np.uint32), "recovered": np.full(self.w_est + g, 0xA5, dtype=np.uint8),
               "ref_letters": np.full(self.w_ref + g, 0xA5A5A5A5, dtype=np.uint32)}
        api._check(_lib().twl_compare_columns(self._h, *[out[k].ctypes.data_as(C.c_void_p) for k in ("shared", "letters", "distinct", "recovered", "ref_letters")]))
        res = {}
        for k, a in out.items():
            w = self.w_ref if k == "ref_letters" else self.w_est
            assert np.all(a[w:] == a.dtype.type(0xA5A5A5A5A5A5A5A5 & ((1 << (8 * a.itemsize)) - 1))), f"{k}: guard words overwritten"
            res[k] = a[:w]
        return res

    def columns_raw(self, **want: bool) -> None:
        """twl_compare_columns with null pointers but for the arrays named true (every pointer may be NULL)."""
        bufs = {"shared": np.zeros(max(1, self.w_est), np.uint64), "letters": np.zeros(max(1, self.w_est), np.uint32), "distinct": np.zeros(max(1, self.w_est), np.uint32),
                "recovered": np.zeros(max(1, self.w_est), np.uint8), "ref_letters": np.zeros(max(1, self.w_ref), np.uint32)}
        api._check(_lib().twl_compare_columns(self._h, *[bufs[k].ctypes.data_as(C.c_void_p) if want.get(k) else None for k in ("shared", "letters", "distinct", "recovered", "ref_letters")]))

    def timing(self) -> Tuple[float, float, float, float]:
        """twl_compare_timing: (upload, keys, columns, download) in ms; the two kernel times are HIP-event times."""
        v = [C.c_double(0) for _ in range(4)]
        api._check(_lib().twl_compare_timing(self._h, *[C.byref(x) for x in v]))
        return tuple(float(x.value) for x in v)

    def close(self) -> None:
        if self._h is not None:
            _lib().twl_compare_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def totals(cols: Dict[str, np.ndarray]) -> Dict[str, int]:
    """The sums a report is made of, as exact Python integers: shared, pairs_out, pairs_ref, recovered, ref_columns (those with 2 letters or more)."""
    le = cols["letters"].astype(object)
    lr = cols["ref_letters"].astype(object)
    return {"shared": int(sum(cols["shared"].astype(object))), "pairs_out": int(sum(x * (x - 1) // 2 for x in le)), "pairs_ref": int(sum(x * (x - 1) // 2 for x in lr)),
            "recovered": int(cols["recovered"].sum()), "ref_columns": int((cols["ref_letters"] >= 2).sum())}
