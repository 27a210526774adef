"""ctypes view of include/pangenie_kmers.h: the device k-mer counter (HIP, gfx950).  No CPU fallback: every
call that computes goes through libpangenie_hmm.so and raises when it is missing or the device call fails."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, NamedTuple

import numpy as np

from . import _lib
from ._lib import u64p, f64p

KMERS_ABI_SYMBOLS = ["pg_kmer_counter_new", "pg_kmer_counter_destroy", "pg_kmer_counter_add_codes", "pg_kmer_counter_add_text",
                     "pg_kmer_counter_freeze", "pg_kmer_counter_count", "pg_kmer_counter_acquire", "pg_kmer_counter_submit",
                     "pg_kmer_counter_sync", "pg_kmer_counter_lookup", "pg_kmer_counter_stats", "pg_kmer_counter_histogram",
                     "pg_kmer_counter_reset_counts", "pg_kmer_counter_capacity", "pg_kmer_counter_table",
                     "pg_kmer_counter_count_resident", "pg_kmer_tile_bytes", "pg_kmer_last_error"]
NOT_REGISTERED = 0xFFFFFFFFFFFFFFFF

_bound = False


def _hip():
    global _bound
    lib = _lib.load_hip()
    if not _bound:
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        for name, args in (("pg_kmer_counter_new", [u32, C.c_int, C.POINTER(vp)]), ("pg_kmer_counter_destroy", [vp]),
                           ("pg_kmer_counter_add_codes", [vp, u64p, u64]), ("pg_kmer_counter_add_text", [vp, C.c_char_p, u64, u64p]),
                           ("pg_kmer_counter_freeze", [vp]), ("pg_kmer_counter_count", [vp, C.c_char_p, u64]),
                           ("pg_kmer_counter_acquire", [vp, C.POINTER(vp), u64p]), ("pg_kmer_counter_submit", [vp, u64]),
                           ("pg_kmer_counter_sync", [vp]), ("pg_kmer_counter_lookup", [vp, u64p, u64, u64p]),
                           ("pg_kmer_counter_stats", [vp, u64p, u64p]), ("pg_kmer_counter_histogram", [vp, u64, u64p]),
                           ("pg_kmer_counter_reset_counts", [vp]), ("pg_kmer_counter_capacity", [vp, u64p]),
                           ("pg_kmer_counter_table", [vp, u64p, u64]),
                           ("pg_kmer_counter_count_resident", [vp, C.c_char_p, u64, u32, f64p])):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = C.c_int
        lib.pg_kmer_tile_bytes.argtypes = []
        lib.pg_kmer_tile_bytes.restype = u32
        lib.pg_kmer_last_error.argtypes = []
        lib.pg_kmer_last_error.restype = C.c_char_p
        _bound = True
    return lib


class KmerCounterError(RuntimeError):
    def __init__(self, call: str, code: int, text: str):
        super().__init__(f"{call}: error {code}: {text}")
        self.code = code


def _check(rc: int, call: str) -> None:
    if rc != _lib.PG_OK:
        raise KmerCounterError(call, rc, (_hip().pg_kmer_last_error() or b"").decode(errors="replace"))


def tile_bytes() -> int:
    """text positions one workgroup of the counting kernel takes"""
    return int(_hip().pg_kmer_tile_bytes())


_LETTER = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _LETTER[ord(_c)] = _LETTER[ord(_c.lower())] = _i


def canonical_codes(kmers: Iterable[str | bytes], k: int) -> np.ndarray:
    """Canonical 2-bit codes (u64) of k-mers given as strings: A, C, G, T = 0..3, first letter in the highest bits, the
    smaller of the k-mer's code and its reverse complement's.  A k-mer with another letter gets NOT_REGISTERED."""
    if not 1 <= k <= 32:
        raise ValueError("k-mer size must be 1..32")
    kmers = [s.encode() if isinstance(s, str) else bytes(s) for s in kmers]
    if any(len(s) != k for s in kmers):
        raise ValueError(f"every k-mer must have {k} letters")
    if not kmers:
        return np.zeros(0, np.uint64)
    letters = _LETTER[np.frombuffer(b"".join(kmers), np.uint8).reshape(len(kmers), k)]
    bad = (letters > 3).any(axis=1)
    b = (letters & 3).astype(np.uint64)
    fwd = np.zeros(len(kmers), np.uint64)
    rev = np.zeros(len(kmers), np.uint64)
    for i in range(k):
        fwd = (fwd << np.uint64(2)) | b[:, i]
        rev = (rev << np.uint64(2)) | (np.uint64(3) - b[:, k - 1 - i])
    out = np.minimum(fwd, rev)
    out[bad] = np.uint64(NOT_REGISTERED)
    return out


class Stats(NamedTuple):
    targets: int
    windows: int


class KmerCounter:
    """Counts of a registered set of k-mers in texts, on the device (TargetedKmerCounter's semantics)."""

    def __init__(self, k: int, device: int = 0):
        self.k = int(k)
        self._h = C.c_void_p()
        if not 0 <= self.k < 2 ** 32:
            raise KmerCounterError("pg_kmer_counter_new", _lib.PG_ERR_INVALID, "k-mer size must be 1..32")
        _check(_hip().pg_kmer_counter_new(self.k, int(device), C.byref(self._h)), "pg_kmer_counter_new")

    def close(self) -> None:
        if self._h:
            _hip().pg_kmer_counter_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_codes(self, codes) -> None:
        a = np.ascontiguousarray(codes, dtype=np.uint64)
        _check(_hip().pg_kmer_counter_add_codes(self._h, a.ctypes.data_as(u64p), a.size), "pg_kmer_counter_add_codes")

    def add_text(self, text: bytes) -> int:
        """registers every window of the text; returns how many (repeats included)"""
        n = C.c_uint64(0)
        text = bytes(text)
        _check(_hip().pg_kmer_counter_add_text(self._h, text, len(text), C.byref(n)), "pg_kmer_counter_add_text")
        return int(n.value)

    def freeze(self) -> None:
        _check(_hip().pg_kmer_counter_freeze(self._h), "pg_kmer_counter_freeze")

    def count(self, text: bytes, sync: bool = True) -> None:
        text = bytes(text)
        _check(_hip().pg_kmer_counter_count(self._h, text, len(text)), "pg_kmer_counter_count")
        if sync:
            self.sync()

    def sync(self) -> None:
        _check(_hip().pg_kmer_counter_sync(self._h), "pg_kmer_counter_sync")

    def lookup_codes(self, codes) -> np.ndarray:
        a = np.ascontiguousarray(codes, dtype=np.uint64)
        out = np.zeros(a.size, np.uint64)
        _check(_hip().pg_kmer_counter_lookup(self._h, a.ctypes.data_as(u64p), a.size, out.ctypes.data_as(u64p)), "pg_kmer_counter_lookup")
        return out

    def lookup(self, kmers) -> np.ndarray:
        """counts of k-mers given as strings (u64; NOT_REGISTERED for a k-mer that was never registered)"""
        return self.lookup_codes(canonical_codes(kmers, self.k))

    def stats(self) -> Stats:
        t, w = C.c_uint64(0), C.c_uint64(0)
        _check(_hip().pg_kmer_counter_stats(self._h, C.byref(t), C.byref(w)), "pg_kmer_counter_stats")
        return Stats(int(t.value), int(w.value))

    def histogram(self, max_count: int) -> np.ndarray:
        out = np.zeros(int(max_count) + 1, np.uint64)
        _check(_hip().pg_kmer_counter_histogram(self._h, int(max_count), out.ctypes.data_as(u64p)), "pg_kmer_counter_histogram")
        return out

    def reset_counts(self) -> None:
        _check(_hip().pg_kmer_counter_reset_counts(self._h), "pg_kmer_counter_reset_counts")

    def table(self) -> np.ndarray:
        """the device table as it is: [capacity, 2] of (key, count), empty slots with key NOT_REGISTERED"""
        cap = C.c_uint64(0)
        _check(_hip().pg_kmer_counter_capacity(self._h, C.byref(cap)), "pg_kmer_counter_capacity")
        out = np.zeros((int(cap.value), 2), np.uint64)
        _check(_hip().pg_kmer_counter_table(self._h, out.ctypes.data_as(u64p), cap.value), "pg_kmer_counter_table")
        return out

    def count_resident(self, text: bytes, repeats: int = 1) -> np.ndarray:
        """measurement: the counting kernel alone on a text uploaded once; device ms per repeat"""
        ms = np.zeros(int(repeats), np.float64)
        text = bytes(text)
        _check(_hip().pg_kmer_counter_count_resident(self._h, text, len(text), int(repeats), ms.ctypes.data_as(f64p)), "pg_kmer_counter_count_resident")
        return ms
