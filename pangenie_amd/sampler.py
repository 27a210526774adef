"""Host-side mirror of the reference's HaplotypeSampler interface over the C ABI of
include/pangenie_sampler.h (HIP, gfx950).  No CPU fallback: every entry point that computes goes through
libpangenie_hmm.so and raises when it is missing.

reference: src/haplotypesampler.hpp:16-59 (SampledPaths), :62-96 (HaplotypeSampler),
           src/samplingemissions.hpp, src/samplingtransitions.hpp
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import PgContigBatch, PgSampleCounts, u8p, u16p, u32p, f64p, c_ld as _c_ld
from .panel import ContigBatch

_bound = False


def _hip():
    global _bound
    lib = _lib.load_hip()
    if not _bound:
        ld = C.c_longdouble
        lib.pg_sampler_emission_costs.argtypes = [C.POINTER(PgContigBatch), u16p]
        lib.pg_sampler_emission_costs.restype = C.c_int
        lib.pg_sampler_transition_cost.argtypes = [C.c_uint64, C.c_uint64, C.c_double, C.c_uint32, ld]
        lib.pg_sampler_transition_cost.restype = C.c_uint32
        lib.pg_sampler_column_minima.argtypes = [u32p, u8p, C.c_uint32, C.c_int, u32p, C.c_char_p, C.c_size_t]
        lib.pg_sampler_column_minima.restype = C.c_int
        lib.pg_sampler_run.argtypes = [C.POINTER(PgContigBatch), C.c_uint32, C.c_double, ld, C.c_uint16, C.c_int,
                                       u32p, u32p, C.c_char_p, C.c_size_t]
        lib.pg_sampler_run.restype = C.c_int
        lib.pg_sampler_run_batch.argtypes = [C.POINTER(PgContigBatch), C.c_uint32, C.c_uint32, C.c_double, ld, C.c_uint16, C.c_int,
                                             C.POINTER(u32p), C.POINTER(u32p), C.c_char_p, C.c_size_t]
        lib.pg_sampler_run_batch.restype = C.c_int
        lib.pg_sampler_then_job.argtypes = [C.POINTER(PgContigBatch), C.c_uint32, C.c_uint32, C.c_int, C.c_double, ld, C.c_uint16,
                                            C.c_void_p, C.c_void_p, C.c_int, C.POINTER(u32p), C.POINTER(u32p),
                                            C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        lib.pg_sampler_then_job.restype = C.c_int
        lib.pg_sampler_last_ms.argtypes = [f64p, C.POINTER(C.c_int)]
        lib.pg_sampler_last_ms.restype = C.c_int
        lib.pg_sampler_cohort_new.argtypes = [C.c_int, C.c_uint32, C.POINTER(PgContigBatch), C.c_uint32, C.POINTER(PgSampleCounts),
                                              C.c_uint32, C.c_int, C.c_double, ld, C.c_uint16, C.c_void_p, C.c_void_p,
                                              C.POINTER(u32p), C.POINTER(u32p), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        lib.pg_sampler_cohort_new.restype = C.c_int
        lib.pg_sampler_cohort_new_device.argtypes = lib.pg_sampler_cohort_new.argtypes
        lib.pg_sampler_cohort_new_device.restype = C.c_int
        lib.pg_sampler_counts_new.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_uint64), u32p, C.c_uint32, C.POINTER(C.c_void_p),
                                              C.c_char_p, C.c_size_t]
        lib.pg_sampler_counts_new.restype = C.c_int
        lib.pg_sampler_counts_destroy.argtypes = [C.c_void_p]
        lib.pg_sampler_counts_destroy.restype = C.c_int
        lib.pg_sampler_counts_rows.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(u16p)), C.POINTER(C.POINTER(u16p)),
                                               C.c_char_p, C.c_size_t]
        lib.pg_sampler_counts_rows.restype = C.c_int
        lib.pg_sampler_last_h2d_bytes.argtypes = [C.POINTER(C.c_uint64)]
        lib.pg_sampler_last_h2d_bytes.restype = C.c_int
        lib.pg_sampler_last_phase_ms.argtypes = [f64p]
        lib.pg_sampler_last_phase_ms.restype = C.c_int
        _bound = True
    return lib


SAMPLER_ABI_SYMBOLS = ["pg_sampler_emission_costs", "pg_sampler_transition_cost", "pg_sampler_column_minima",
                       "pg_sampler_run", "pg_sampler_run_batch", "pg_sampler_last_ms", "pg_sampler_then_job",
                       "pg_sampler_cohort_new", "pg_sampler_last_phase_ms", "pg_sampler_cohort_new_device",
                       "pg_sampler_counts_new", "pg_sampler_counts_destroy", "pg_sampler_counts_rows"]
# (pg_sampler_last_h2d_bytes is exported too; it stays off this list, which mirrors the header's letters-only names)
NO_ID = 0xFFFFFFFF


class SampledPaths:
    """reference src/haplotypesampler.hpp:16-59.  sampled_paths[j][v] = path id of sampled path j at variant v."""

    def __init__(self, sampled_paths: Sequence[Sequence[int]] = ()):
        self.sampled_paths = [list(map(int, p)) for p in sampled_paths]

    def mask_indexes(self, column_index: int, max_index: int) -> list[bool]:
        masked = [True] * (max_index + 1)
        for p in self.sampled_paths:
            if column_index >= len(p):
                raise RuntimeError("HaplotypeSampler::SampledPaths::mask_indexes: column_index exceeds number of columns.")
            if p[column_index] > max_index:
                raise RuntimeError("HaplotypeSampler::SampledPaths::mask_indexes: observed index exceeds max_index.")
            masked[p[column_index]] = False
        return masked

    def recombination(self, column_index: int, path_id: int) -> bool:
        if path_id >= len(self.sampled_paths):
            raise RuntimeError("HaplotypeSampler::SampledPaths::recombination: path_id does not exist.")
        if column_index >= len(self.sampled_paths[path_id]):
            raise RuntimeError("HaplotypeSampler::SampledPaths::recombination: column_id does not exist.")
        if column_index > 0:
            return self.sampled_paths[path_id][column_index - 1] != self.sampled_paths[path_id][column_index]
        return False


class SamplingTransitions:
    """reference src/samplingtransitions.cpp:5-23."""

    def __init__(self, from_variant: int, to_variant: int, recomb_rate: float, nr_paths: int, effective_N=25000.0):
        assert from_variant <= to_variant
        self.cost = int(_hip().pg_sampler_transition_cost(int(from_variant), int(to_variant), float(recomb_rate), int(nr_paths),
                                                          _c_ld(effective_N)))

    def compute_transition_cost(self, recombination: bool) -> int:
        return self.cost if recombination else 0


def emission_costs(batch: ContigBatch) -> np.ndarray:
    """SamplingEmissions ctor for every allele slot of the batch (u16 [sumA])."""
    out = np.zeros(max(1, int(batch.allele_off[-1])), np.uint16)
    rc = _hip().pg_sampler_emission_costs(C.byref(batch.as_c()), out.ctypes.data_as(u16p))
    if rc:
        raise RuntimeError(f"pg_sampler_emission_costs: error {rc}")
    return out[: int(batch.allele_off[-1])]


class SamplingEmissions:
    """reference src/samplingemissions.cpp:9-45 for ONE variant of a batch."""

    def __init__(self, batch: ContigBatch, variant: int = 0, _costs: np.ndarray | None = None):
        costs = emission_costs(batch) if _costs is None else _costs
        lo, hi = int(batch.allele_off[variant]), int(batch.allele_off[variant + 1])
        ids = batch.allele_id[lo:hi]
        self.allele_penalties = np.zeros(int(ids.max()) + 1, np.uint16)
        self.allele_penalties[ids] = costs[lo:hi]
        self.default_penalty = 25

    def get_emission_cost(self, allele_id: int) -> int:
        return int(self.allele_penalties[allele_id])

    def penalize(self, allele_id: int, penalty: int):
        v = (int(self.allele_penalties[allele_id]) + int(penalty)) & 0xFFFF
        self.allele_penalties[allele_id] = min(v, self.default_penalty)


def column_minima(column: Sequence[int], mask: Sequence[bool], device: int = 0):
    """HaplotypeSampler::get_column_minima on the device -> (first_id, second_id, first_val, second_val)."""
    col = np.ascontiguousarray(column, np.uint32)
    m = np.ascontiguousarray(mask, np.uint8)
    assert col.size > 1 and col.size == m.size
    out = np.zeros(4, np.uint32)
    err = C.create_string_buffer(256)
    rc = _hip().pg_sampler_column_minima(col.ctypes.data_as(u32p), m.ctypes.data_as(u8p), col.size, device,
                                         out.ctypes.data_as(u32p), err, 256)
    if rc:
        raise RuntimeError(err.value.decode())
    return tuple(int(x) for x in out)


def last_ms():
    """((expand, forward, backtrack) kernel ms of this thread's last run, waves per workgroup of the fast kernel or 0)"""
    ms = np.zeros(3)
    k = C.c_int(0)
    _hip().pg_sampler_last_ms(ms.ctypes.data_as(f64p), C.byref(k))
    return (float(ms[0]), float(ms[1]), float(ms[2])), int(k.value)


def sample_contigs(batches: Sequence[ContigBatch], size: int, recombrate: float = 1.26, effective_N=25000.0,
                   allele_penalty: int = 10, device: int = 0):
    """pg_sampler_run_batch: all contigs of a sample in one call (one workgroup per contig and pass).
    -> (list of sampled paths [size, V_g], list of best scores [size])"""
    n = len(batches)
    arr = (PgContigBatch * n)(*[b.as_c() for b in batches])
    sampled = [np.zeros((size, max(1, b.n_variants)), np.uint32) for b in batches]
    best = [np.zeros(max(1, size), np.uint32) for _ in batches]
    sp = (u32p * n)(*[a.ctypes.data_as(u32p) for a in sampled])
    bp = (u32p * n)(*[a.ctypes.data_as(u32p) for a in best])
    err = C.create_string_buffer(512)
    rc = _hip().pg_sampler_run_batch(arr, n, size, float(recombrate), _c_ld(effective_N), int(allele_penalty), device, sp, bp, err, 512)
    if rc:
        raise RuntimeError(f"pg_sampler_run_batch: {err.value.decode()} (error {rc})")
    return [s[:, : b.n_variants] for s, b in zip(sampled, batches)], [x[:size] for x in best]


def sample_then_job(batches: Sequence[ContigBatch], size: int, table, params=None, add_reference: bool = False,
                    recombrate: float = 1.26, effective_N=25000.0, allele_penalty: int = 10, device: int = 0, want_paths: bool = True):
    """pg_sampler_then_job: the sampler, UniqueKmers::update_paths and the genotyping job's upload without the panel
    leaving the device.  -> (hmm.Job over the reduced panels — job.batches are read back from the device —,
    sampled paths per contig [size, V] or None, best scores per contig [size] or None)."""
    from . import hmm
    n = len(batches)
    arr = (PgContigBatch * n)(*[b.as_c() for b in batches])
    sampled = [np.zeros((size, max(1, b.n_variants)), np.uint32) for b in batches] if want_paths else None
    best = [np.zeros(max(1, size), np.uint32) for _ in batches] if want_paths else None
    sp = (u32p * n)(*[a.ctypes.data_as(u32p) for a in sampled]) if want_paths else None
    bp = (u32p * n)(*[a.ctypes.data_as(u32p) for a in best]) if want_paths else None
    params = params or hmm.make_params()
    err = C.create_string_buffer(512)
    h = C.c_void_p()
    rc = _hip().pg_sampler_then_job(arr, n, size, int(bool(add_reference)), float(recombrate), _c_ld(effective_N), int(allele_penalty),
                                    table.h, C.byref(params), device, sp, bp, C.byref(h), err, 512)
    if rc:
        raise hmm.PanGenieError(rc, err.value.decode(errors="replace"))
    job = hmm.Job.from_handle(h.value, table, params)
    if want_paths:
        return job, [s[:, : b.n_variants] for s, b in zip(sampled, batches)], [x[:size] for x in best]
    return job, None, None


def marshal_samples(index: Sequence[ContigBatch], samples):
    """(pg_sample_counts[n], arrays to keep alive) from samples in the format of hmm.Job.cohort — one (kmer_counts,
    coverages) per sample, one uint16 array per index contig —, the lengths checked against the index on the host."""
    nc = len(index)
    arr = (PgSampleCounts * len(samples))()
    keep = []
    for s, (kcs, covs) in enumerate(samples):
        if len(kcs) != nc or len(covs) != nc:
            raise ValueError(f"sample {s}: {len(kcs)} count arrays and {len(covs)} coverage arrays for {nc} contigs")
        kc = [np.ascontiguousarray(a, np.uint16) for a in kcs]
        cv = [np.ascontiguousarray(a, np.uint16) for a in covs]
        for c, b in enumerate(index):
            if kc[c].size != int(b.kmer_off[-1]) or cv[c].size != b.n_variants:
                raise ValueError(f"sample {s}, contig {c}: {kc[c].size} counts / {cv[c].size} coverages, the index has "
                                 f"{int(b.kmer_off[-1])} k-mers / {b.n_variants} variants")
        kc = [a if a.size else np.zeros(1, np.uint16) for a in kc]
        cv = [a if a.size else np.zeros(1, np.uint16) for a in cv]
        pk = (u16p * nc)(*[a.ctypes.data_as(u16p) for a in kc])
        pc = (u16p * nc)(*[a.ctypes.data_as(u16p) for a in cv])
        arr[s].kmer_count = pk
        arr[s].coverage = pc
        keep += [kc, cv, pk, pc]
    return arr, keep


def sample_cohort(index: Sequence[ContigBatch], samples, size: int, table, params=None, add_reference: bool = False,
                  recombrate: float = 1.26, effective_N=25000.0, allele_penalty: int = 10, device: int = 0, want_paths: bool = True):
    """pg_sampler_cohort_new: sample_then_job for every sample over ONE index (uploaded once; per sample only the k-mer
    counts).  samples: as hmm.Job.cohort takes them.  -> (hmm.Job — chain s * n_contigs + c; job.batches are the reduced
    panels read back from the device —, sampled[s][c] [size, V_c] or None, best[s][c] [size] or None)."""
    from . import hmm
    index = list(index)
    samples = list(samples)
    nc, ns = len(index), len(samples)
    arr = (PgContigBatch * nc)(*[b.as_c() for b in index])
    cs, keep = marshal_samples(index, samples)
    sampled = best = sp = bp = None
    if want_paths:
        sampled = [[np.zeros((size, max(1, b.n_variants)), np.uint32) for b in index] for _ in range(ns)]
        best = [[np.zeros(max(1, size), np.uint32) for _ in index] for _ in range(ns)]
        sp = (u32p * (ns * nc))(*[a.ctypes.data_as(u32p) for row in sampled for a in row])
        bp = (u32p * (ns * nc))(*[a.ctypes.data_as(u32p) for row in best for a in row])
    params = params or hmm.make_params()
    err = C.create_string_buffer(1024)
    h = C.c_void_p()
    rc = _hip().pg_sampler_cohort_new(device, nc, arr, ns, cs, size, int(bool(add_reference)), float(recombrate), _c_ld(effective_N),
                                      int(allele_penalty), table.h, C.byref(params), sp, bp, C.byref(h), err, 1024)
    del keep
    if rc:
        raise hmm.PanGenieError(rc, err.value.decode(errors="replace"))
    job = hmm.Job.from_handle(h.value, table, params)
    if want_paths:
        return (job, [[s[:, : b.n_variants] for s, b in zip(row, index)] for row in sampled],
                [[x[:size] for x in row] for row in best])
    return job, None, None


def _memcpy(dst: int, src: int, nbytes: int, kind: int) -> None:
    """hipMemcpy of the HIP runtime the product library is linked against, found through the library's own handle (kind 2:
    device to host, 3: device to device)"""
    fn = _hip().hipMemcpy
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn.restype = C.c_int
    rc = fn(C.c_void_p(dst), C.c_void_p(src), nbytes, kind)
    if rc:
        raise RuntimeError(f"hipMemcpy: error {rc}")


class SamplerCounts:
    """pg_sampler_counts: for each of n_samples samples and every contig of `index` one uint16 array of the contig's k-mers
    and one of its variants, in one allocation on `device` — what CountPlan.fill_device(out=counts.rows(s)) fills and
    sample_cohort_device reads.  A context manager; the arrays are gone when it closes."""

    def __init__(self, index: Sequence[ContigBatch], n_samples: int, device: int = 0):
        from . import hmm
        self.sizes = [(int(b.kmer_off[-1]), int(b.n_variants)) for b in index]
        self.n_samples, self.device = int(n_samples), int(device)
        nc = len(self.sizes)
        nk = (C.c_uint64 * max(nc, 1))(*[k for k, _ in self.sizes])
        nv = (C.c_uint32 * max(nc, 1))(*[v for _, v in self.sizes])
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = _hip().pg_sampler_counts_new(self.device, nc, nk, nv, self.n_samples, C.byref(self._h), err, 512)
        if rc:
            raise hmm.PanGenieError(rc, err.value.decode(errors="replace"))

    def close(self) -> None:
        if self._h:
            _hip().pg_sampler_counts_destroy(self._h)
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

    def rows(self, sample: int):
        """(d_kmer_count, d_coverage): the handle's own pointer tables of one sample, [n_contigs] device pointers each"""
        from . import hmm
        pk, pc = C.POINTER(u16p)(), C.POINTER(u16p)()
        err = C.create_string_buffer(256)
        rc = _hip().pg_sampler_counts_rows(self._h, int(sample), C.byref(pk), C.byref(pc), err, 256)
        if rc:
            raise hmm.PanGenieError(rc, err.value.decode(errors="replace"))
        return pk, pc

    def pointers(self, sample: int):
        """the same as integers: ([address of kmer_count[c]], [address of coverage[c]])"""
        pk, pc = self.rows(sample)
        addr = lambda p: C.cast(p, C.c_void_p).value
        return [addr(pk[c]) for c in range(len(self.sizes))], [addr(pc[c]) for c in range(len(self.sizes))]

    def as_tensors(self, sample: int):
        """(kmer_count, coverage) of one sample as torch int16 tensors on the host (the bits are the uint16 values), read
        back from the device"""
        import torch
        ks, cs = self.pointers(sample)
        out = ([], [])
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            for c, (nk, nv) in enumerate(self.sizes):
                for which, (addr, n) in enumerate(((ks[c], nk), (cs[c], nv))):
                    t = torch.zeros(n, dtype=torch.int16)
                    if n:
                        _memcpy(t.data_ptr(), addr, 2 * n, 2)
                    out[which].append(t)
        return out

    def copy_from(self, sample: int, kmer_count, coverage) -> None:
        """fills one sample's arrays from torch int16 tensors on the device, one D2D copy per array"""
        import torch
        ks, cs = self.pointers(sample)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            for c, (nk, nv) in enumerate(self.sizes):
                for t, addr, n in ((kmer_count[c], ks[c], nk), (coverage[c], cs[c], nv)):
                    if t.numel() != n or t.dtype != torch.int16 or not t.is_cuda:
                        raise ValueError(f"sample {sample}, contig {c}: an int16 device tensor of {n} entries is expected")
                    if n:
                        _memcpy(addr, t.contiguous().data_ptr(), 2 * n, 3)


def marshal_device_samples(index: Sequence[ContigBatch], d_samples):
    """(pg_sample_counts[n], objects to keep alive) from a SamplerCounts, or from one (kmer_counts, coverages) per sample with
    one torch int16 device tensor per index contig (what CountPlan.fill_device returns).  Lengths are checked against the
    index here; where the memory lies is checked by the C ABI."""
    nc = len(index)
    if isinstance(d_samples, SamplerCounts):
        if d_samples.sizes != [(int(b.kmer_off[-1]), int(b.n_variants)) for b in index]:
            raise ValueError("the SamplerCounts was made over another index")
        arr = (PgSampleCounts * d_samples.n_samples)()
        for s in range(d_samples.n_samples):
            arr[s].kmer_count, arr[s].coverage = d_samples.rows(s)
        return arr, [d_samples]
    d_samples = list(d_samples)
    arr = (PgSampleCounts * len(d_samples))()
    keep = []
    for s, (kcs, covs) in enumerate(d_samples):
        if len(kcs) != nc or len(covs) != nc:
            raise ValueError(f"sample {s}: {len(kcs)} count arrays and {len(covs)} coverage arrays for {nc} contigs")
        rows = []
        for what, arrays, sizes in (("kmer_count", kcs, [int(b.kmer_off[-1]) for b in index]), ("coverage", covs, [b.n_variants for b in index])):
            ptrs = []
            for c, (a, n) in enumerate(zip(arrays, sizes)):
                if isinstance(a, np.ndarray):   # (not a device array: handed on as it is, for the C ABI to refuse)
                    a = np.ascontiguousarray(a, np.uint16)
                    size, addr = a.size, a.ctypes.data
                else:
                    a = a.contiguous()
                    size, addr = a.numel(), a.data_ptr()
                    if a.element_size() != 2:
                        raise ValueError(f"sample {s}, contig {c}: {what} must be 16-bit")
                if size != n:
                    raise ValueError(f"sample {s}, contig {c}: {size} entries of {what}, the index has {n}")
                keep.append(a)
                ptrs.append(C.cast(C.c_void_p(addr if n else None), u16p))
            rows.append((u16p * nc)(*ptrs))
        arr[s].kmer_count, arr[s].coverage = rows
        keep += rows
    return arr, keep


def sample_cohort_device(index: Sequence[ContigBatch], d_samples, size: int, table, params=None, add_reference: bool = False,
                         recombrate: float = 1.26, effective_N=25000.0, allele_penalty: int = 10, device: int = 0, want_paths: bool = True):
    """pg_sampler_cohort_new_device: sample_cohort with the samples' arrays already on the device — `d_samples` a
    SamplerCounts, or per sample a pair of lists of torch int16 device tensors.  The counts are read in place; only the
    coverage (2 bytes per variant) comes back.  Returns what sample_cohort returns."""
    from . import hmm
    index = list(index)
    nc = len(index)
    arr = (PgContigBatch * nc)(*[b.as_c() for b in index])
    cs, keep = marshal_device_samples(index, d_samples)
    ns = len(cs)
    sampled = best = sp = bp = None
    if want_paths:
        sampled = [[np.zeros((size, max(1, b.n_variants)), np.uint32) for b in index] for _ in range(ns)]
        best = [[np.zeros(max(1, size), np.uint32) for _ in index] for _ in range(ns)]
        sp = (u32p * (ns * nc))(*[a.ctypes.data_as(u32p) for row in sampled for a in row])
        bp = (u32p * (ns * nc))(*[a.ctypes.data_as(u32p) for row in best for a in row])
    params = params or hmm.make_params()
    err = C.create_string_buffer(1024)
    h = C.c_void_p()
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize(device)   # (tensors filled on torch's stream: the sampler's kernels sit on the null stream)
    except ImportError:
        pass
    rc = _hip().pg_sampler_cohort_new_device(device, nc, arr, ns, cs, size, int(bool(add_reference)), float(recombrate), _c_ld(effective_N),
                                             int(allele_penalty), table.h, C.byref(params), sp, bp, C.byref(h), err, 1024)
    del keep
    if rc:
        raise hmm.PanGenieError(rc, err.value.decode(errors="replace"))
    job = hmm.Job.from_handle(h.value, table, params)
    if want_paths:
        return (job, [[s[:, : b.n_variants] for s, b in zip(row, index)] for row in sampled],
                [[x[:size] for x in row] for row in best])
    return job, None, None


def last_h2d_bytes():
    """H2D bytes of this thread's last sample_cohort / sample_then_job: (index arrays, per-sample arrays)"""
    out = (C.c_uint64 * 2)()
    _hip().pg_sampler_last_h2d_bytes(out)
    return int(out[0]), int(out[1])


def last_phase_ms() -> dict:
    """Milliseconds of this thread's last sample_cohort, phase by phase (include/pangenie_sampler.h: pg_sampler_last_phase_ms)."""
    ms = np.zeros(8)
    _hip().pg_sampler_last_phase_ms(ms.ctypes.data_as(f64p))
    return dict(zip(("host_prep", "h2d", "cost_kernel", "slots", "passes", "reduction", "job_new", "total"), map(float, ms)))


class HaplotypeSampler:
    """reference src/haplotypesampler.cpp:20-77: `size` Viterbi passes over the panel, then (update_unique_kmers)
    the panel reduced to the sampled paths — here returned as `self.panel` (a new ContigBatch) instead of
    mutating the input."""

    def __init__(self, batch: ContigBatch, size: int, recombrate: float = 1.26, effective_N=25000.0,
                 add_reference: bool = False, allele_penalty: int = 10, device: int = 0):
        self.batch = batch
        self.best_scores: list[int] = []
        self._paths = SampledPaths()
        self.kernel_ms = (0.0, 0.0, 0.0)
        self.kernel = 0
        self.panel = batch
        if size < 1:
            return
        V = batch.n_variants
        sampled = np.zeros((size, max(V, 1)), np.uint32)
        best = np.zeros(size, np.uint32)
        err = C.create_string_buffer(512)
        lib = _hip()
        rc = lib.pg_sampler_run(C.byref(batch.as_c()), size, float(recombrate), _c_ld(effective_N), int(allele_penalty),
                                device, sampled.ctypes.data_as(u32p), best.ctypes.data_as(u32p), err, 512)
        if rc:
            raise RuntimeError(f"pg_sampler_run: {err.value.decode()} (error {rc})")
        self.kernel_ms, self.kernel = last_ms()
        sampled = sampled[:, :V]
        self.best_scores = [int(x) for x in best] if V else []
        if add_reference:
            sampled = np.vstack([sampled, np.zeros((1, V), np.uint32)])
        self.sampled = sampled
        self._paths = SampledPaths(sampled.tolist()) if V else SampledPaths()
        if V:
            self.panel = batch.update_paths(sampled)

    def get_sampled_paths(self) -> SampledPaths:
        return self._paths
