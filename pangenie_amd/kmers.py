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


# ------------------------------------------------------------------------------------------------ include/pangenie_counts.h
COUNTS_ABI_SYMBOLS = ["pg_count_plan_new", "pg_count_plan_destroy", "pg_count_plan_fill_host", "pg_count_plan_fill_device",
                      "pg_count_plan_fill_job", "pg_count_plan_stats", "pg_count_plan_last_fill_ms"]


class PgCountContig(C.Structure):
    _fields_ = [("n_variants", C.c_uint32), ("kmer_off", _lib.u32p), ("kmer_code", u64p), ("flank_off", u64p), ("flank_code", u64p)]


_counts_bound = False


def _counts():
    global _counts_bound
    lib = _hip()
    if not _counts_bound:
        vp, u64 = C.c_void_p, C.c_uint64
        rows = C.POINTER(_lib.u16p)
        for name, args in (("pg_count_plan_new", [vp, C.c_uint32, C.POINTER(PgCountContig), C.c_int, C.POINTER(vp)]),
                           ("pg_count_plan_destroy", [vp]), ("pg_count_plan_fill_host", [vp, u64, rows, rows]),
                           ("pg_count_plan_fill_device", [vp, u64, C.POINTER(vp), C.POINTER(vp)]),
                           ("pg_count_plan_fill_job", [vp, u64, vp, C.c_uint32, C.c_char_p, C.c_size_t]),
                           ("pg_count_plan_stats", [vp, u64p, u64p, u64p, u64p])):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = C.c_int
        lib.pg_count_plan_last_fill_ms.argtypes = [vp]
        lib.pg_count_plan_last_fill_ms.restype = C.c_double
        _counts_bound = True
    return lib


class CountContig(NamedTuple):
    """What the index asks about on one contig: the unique k-mers of variant v are kmer_code[kmer_off[v]:kmer_off[v + 1]],
    its flanking k-mers flank_code[flank_off[v]:flank_off[v + 1]] (canonical codes; NOT_REGISTERED for a k-mer with a
    letter outside ACGT)."""
    kmer_off: np.ndarray     # u32 [V + 1]
    kmer_code: np.ndarray    # u64
    flank_off: np.ndarray    # u64 [V + 1]
    flank_code: np.ndarray   # u64
    chromosome: str = ""
    start: np.ndarray | None = None   # u64 [V] second column of the table

    @property
    def n_variants(self) -> int:
        return int(len(self.kmer_off)) - 1 if len(self.kmer_off) else 0


def parse_kmer_table(path, k: int) -> CountContig:
    """One `<prefix>_<chromosome>_kmers.tsv(.gz)` table as a CountContig: five tab-separated columns (chromosome, start, one
    this step does not use, unique k-mers, flanking k-mers; the lists comma-separated, `nan` when empty), rows whose first
    column starts with '#' are headers."""
    import gzip
    path = str(path)
    kmers, flanks, koff, foff, starts, chrom = [], [], [0], [0], [], ""
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        for line in f:
            line = line.rstrip("\n")
            if not line:
                continue
            cols = line.split("\t")
            if cols and cols[-1] == "" and len(cols) == 6:
                cols.pop()
            if len(cols) != 5:
                raise ValueError(f"{path}: expected 5 tab-separated fields")
            if cols[0].startswith("#"):
                continue
            if chrom and cols[0] != chrom:
                raise ValueError(f"{path}: line of chromosome {cols[0]} in the table of {chrom}")
            chrom = cols[0]
            digits = cols[1][:len(cols[1]) - len(cols[1].lstrip("0123456789"))]
            starts.append(int(digits) if digits else 0)
            for col, items, off in ((cols[3], kmers, koff), (cols[4], flanks, foff)):
                if col != "nan" and col != "":
                    items += col.split(",")
                off.append(len(items))
    V = len(starts)
    return CountContig(np.asarray(koff if V else [0], np.uint32), canonical_codes(kmers, k), np.asarray(foff if V else [0], np.uint64),
                       canonical_codes(flanks, k), chrom, np.asarray(starts, np.uint64))


class PlanStats(NamedTuple):
    n_kmers: int
    n_flanks: int
    unresolved: int
    device_bytes: int


class CountPlan:
    """The index-level half of fill_read_kmercounts resident on the device (include/pangenie_counts.h): the slot of every
    unique and flanking k-mer in `counter`'s table, resolved once; fill*() turn the counter's counts into one sample's
    kmer_count / coverage arrays with one kernel.  `counter` must outlive the plan."""

    def __init__(self, counter: KmerCounter, contigs, lenient: bool = False):
        self.counter = counter
        self.contigs = [CountContig(np.ascontiguousarray(c.kmer_off, np.uint32), np.ascontiguousarray(c.kmer_code, np.uint64),
                                    np.ascontiguousarray(c.flank_off, np.uint64), np.ascontiguousarray(c.flank_code, np.uint64),
                                    *tuple(c)[4:]) for c in contigs]
        arr = (PgCountContig * max(len(self.contigs), 1))()
        for a, c in zip(arr, self.contigs):
            a.n_variants = c.n_variants
            a.kmer_off = c.kmer_off.ctypes.data_as(_lib.u32p) if c.kmer_off.size else None
            a.kmer_code = c.kmer_code.ctypes.data_as(u64p) if c.kmer_code.size else None
            a.flank_off = c.flank_off.ctypes.data_as(u64p) if c.flank_off.size else None
            a.flank_code = c.flank_code.ctypes.data_as(u64p) if c.flank_code.size else None
        self._h = C.c_void_p()
        _check(_counts().pg_count_plan_new(counter._h, len(self.contigs), arr, 1 if lenient else 0, C.byref(self._h)), "pg_count_plan_new")

    @classmethod
    def from_tables(cls, counter: KmerCounter, paths, k: int | None = None, lenient: bool = False) -> "CountPlan":
        """a plan over `_kmers.tsv(.gz)` tables, one contig per table in the order given"""
        return cls(counter, [parse_kmer_table(p, counter.k if k is None else k) for p in paths], lenient)

    def close(self) -> None:
        if self._h:
            _counts().pg_count_plan_destroy(self._h)
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

    def _sizes(self):
        return [(int(c.kmer_off[-1]) if c.n_variants else 0, c.n_variants) for c in self.contigs]

    def fill(self, kmer_coverage: int):
        """(kmer_count, coverage): per contig a uint16 array of each, on the host"""
        kc = [np.zeros(nk, np.uint16) for nk, _ in self._sizes()]
        cv = [np.zeros(nv, np.uint16) for _, nv in self._sizes()]
        n = max(len(kc), 1)
        pk = (_lib.u16p * n)(*[a.ctypes.data_as(_lib.u16p) if a.size else None for a in kc])
        pc = (_lib.u16p * n)(*[a.ctypes.data_as(_lib.u16p) if a.size else None for a in cv])
        _check(_counts().pg_count_plan_fill_host(self._h, int(kmer_coverage), pk, pc), "pg_count_plan_fill_host")
        return kc, cv

    def fill_device(self, kmer_coverage: int, device: int = 0, out=None):
        """the same into torch tensors on the counter's device (dtype int16: the bits are the uint16 values).  `out`: two
        tables of device pointers, one entry per contig (pangenie_amd.sampler.SamplerCounts.rows(s)): the arrays they point
        at are filled instead, nothing is allocated, and `out` is returned."""
        if out is not None:
            pk, pc = out
            _check(_counts().pg_count_plan_fill_device(self._h, int(kmer_coverage), C.cast(pk, C.POINTER(C.c_void_p)),
                                                       C.cast(pc, C.POINTER(C.c_void_p))), "pg_count_plan_fill_device")
            return out
        import torch
        dev = torch.device("cuda", int(device))
        kc = [torch.zeros(nk, dtype=torch.int16, device=dev) for nk, _ in self._sizes()]
        cv = [torch.zeros(nv, dtype=torch.int16, device=dev) for _, nv in self._sizes()]
        torch.cuda.synchronize(dev)
        n = max(len(kc), 1)
        pk = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in kc])
        pc = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in cv])
        _check(_counts().pg_count_plan_fill_device(self._h, int(kmer_coverage), pk, pc), "pg_count_plan_fill_device")
        return kc, cv

    def fill_job(self, job, sample: int, kmer_coverage: int) -> None:
        """straight into the arrays of sample `sample` of a cohort job (pangenie_amd.hmm.Job.cohort)"""
        err = C.create_string_buffer(512)
        rc = _counts().pg_count_plan_fill_job(self._h, int(kmer_coverage), C.c_void_p(job.h), int(sample), err, 512)
        if rc != _lib.PG_OK:
            raise KmerCounterError("pg_count_plan_fill_job", rc, err.value.decode(errors="replace"))

    def stats(self) -> PlanStats:
        v = [C.c_uint64(0) for _ in range(4)]
        _check(_counts().pg_count_plan_stats(self._h, *[C.byref(x) for x in v]), "pg_count_plan_stats")
        return PlanStats(*[int(x.value) for x in v])

    def last_fill_ms(self) -> float:
        return float(_counts().pg_count_plan_last_fill_ms(self._h))
