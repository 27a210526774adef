"""Python face of the C ABI (include/pangenie_hmm.h): ProbabilityTable, HMM runs, resident jobs.

All compute happens in libpangenie_hmm.so (HIP kernels, gfx950).  This module only
marshals numpy arrays and rebuilds the reference's `long double` likelihoods from
(lik, lik_exp) — `np.longdouble` is the x87 80-bit type on x86-64.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (PG_N_KERNEL_CLASSES, PgContigBatch, PgContigResult, PgHmmParams, PgSampleCounts, f64p, i32p,
                   ldp, u8p, u16p, u64p)
from .genotyping_result import GenotypingResult, results_from_flat
from .panel import ContigBatch

LD = np.longdouble
_ERRLEN = 512


class PanGenieError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def make_params(recombrate: float = 1.26, uniform: bool = False, effective_N=25000.0,
                run_genotyping: bool = True, run_phasing: bool = False) -> PgHmmParams:
    """HMM constructor arguments (reference src/hmm.hpp:38)."""
    p = PgHmmParams()
    p.effective_N = _lib.c_ld(effective_N)
    p.recombrate = float(recombrate)
    p.uniform = int(bool(uniform))
    p.run_genotyping = int(bool(run_genotyping))
    p.run_phasing = int(bool(run_phasing))
    return p


class ProbabilityTable:
    """Mirror of the reference ProbabilityTable (src/probabilitytable.hpp:13-29)."""

    def __init__(self, cov_min: int = 0, cov_max: int = 0, count_max: int = 0,
                 regularization=0.0, default: bool = False):
        self._lib = _lib.load_hip()
        if default:
            self.h = self._lib.pg_table_create_default()
        else:
            self.h = self._lib.pg_table_create(cov_min, cov_max, count_max, _lib.c_ld(regularization))
        if not self.h:
            raise MemoryError("pg_table_create failed")

    def modify(self, coverage: int, count: int, p0, p1, p2) -> None:
        rc = self._lib.pg_table_modify(self.h, coverage, count, _lib.c_ld(p0), _lib.c_ld(p1), _lib.c_ld(p2))
        if rc:
            raise RuntimeError("ProbabilityTable::modify_probability: no precomputed values for these parameters.")

    def get(self, coverage: int, count: int) -> np.ndarray:
        out, ptr = _lib.ld_out(3)
        self._lib.pg_table_get(self.h, coverage, count, ptr)
        return out

    def __del__(self):
        try:
            if self.h:
                self._lib.pg_table_destroy(self.h)
                self.h = None
        except Exception:
            pass


class ContigResult:
    """Host buffers of one pg_contig_result + long double reconstruction."""

    def __init__(self, batch: ContigBatch):
        V = batch.n_variants
        self.batch = batch
        self.geno_off = batch.geno_off
        n = int(self.geno_off[-1])
        self.lik = np.zeros(max(n, 1), np.float64)[:n]
        self.lik_exp = np.zeros(max(n, 1), np.int32)[:n]  # one exponent per genotype bin
        self.kept = np.zeros(max(V, 1), np.uint8)[:V]
        nA = int(batch.allele_off[-1]) if V else 0
        self.allele_present = np.zeros(max(nA, 1), np.uint8)[:nA]
        self.n_kmers = np.zeros(max(V, 1), np.uint16)[:V]
        self.coverage = np.zeros(max(V, 1), np.uint16)[:V]
        self.n_columns = 0
        # run_phasing: alleles of the Viterbi path's two haplotypes at kept variants
        self.haplotype_1 = np.zeros(max(V, 1), np.uint16)[:V]
        self.haplotype_2 = np.zeros(max(V, 1), np.uint16)[:V]
        self.run_genotyping = True
        self._c = PgContigResult()
        self._c.lik = self.lik.ctypes.data_as(f64p)
        self._c.lik_exp = self.lik_exp.ctypes.data_as(i32p)
        self._c.kept = self.kept.ctypes.data_as(u8p)
        self._c.allele_present = self.allele_present.ctypes.data_as(u8p)
        self._c.n_kmers = self.n_kmers.ctypes.data_as(u16p)
        self._c.coverage = self.coverage.ctypes.data_as(u16p)
        self._c.haplotype_1 = self.haplotype_1.ctypes.data_as(u16p)
        self._c.haplotype_2 = self.haplotype_2.ctypes.data_as(u16p)

    def likelihoods_ld(self) -> np.ndarray:
        """Unnormalised genotype likelihoods as 80-bit long double: lik[g] * 2^lik_exp[g]."""
        return np.ldexp(self.lik.astype(LD), self.lik_exp.astype(np.int64))

    def genotyping_results(self) -> List[GenotypingResult]:
        return results_from_flat(self.batch, self.likelihoods_ld(), self.kept, self.allele_present,
                                 self.n_kmers, self.coverage, self.haplotype_1, self.haplotype_2,
                                 with_likelihoods=self.run_genotyping)


def genotype_contig(batch: ContigBatch, table: ProbabilityTable, params: Optional[PgHmmParams] = None,
                    device: int = 0, announced: bool = False, into: Optional[ContigResult] = None) -> ContigResult:
    """One blocking call = the body of HMM::HMM for one (contig, path subset)
    (reference src/hmm.cpp:25-63 with normalize=false, as run_genotyping calls it,
    src/commands.cpp:160).  Thread-safe (ctypes drops the GIL for the call); calls in flight together are merged
    into one device job.  `announced`: the caller has called announce(device) for this call (what the C++ adapter's
    constructor does before it flattens).  `into`: result buffers to reuse."""
    lib = _lib.load_hip()
    params = params or make_params()
    if announced:
        q = PgHmmParams()
        C.memmove(C.byref(q), C.byref(params), C.sizeof(PgHmmParams))
        q.reserved = _lib.PG_CALL_ANNOUNCED
        params = q
    try:
        res = into if into is not None else ContigResult(batch)
        err = C.create_string_buffer(_ERRLEN)
        cb, th = batch.as_c(), table.h
    except Exception:
        if announced:   # the C call that would have consumed the announcement is never made: take it back (a leader would
            lib.pg_hmm_retract(device)   # otherwise wait PG_COALESCE_WAIT_MS for a caller that is not coming)
        raise
    rc = lib.pg_hmm_genotype_contig(C.byref(cb), th, C.byref(params), device, C.byref(res._c), err, _ERRLEN)
    if rc:
        raise PanGenieError(rc, err.value.decode(errors="replace"))
    res.n_columns = int(res._c.n_columns)
    res.run_genotyping = bool(params.run_genotyping)
    return res


def announce(device: int = 0) -> None:
    """pg_hmm_announce: a genotype_contig(..., announced=True) call on `device` will follow shortly."""
    _lib.load_hip().pg_hmm_announce(device)


def coalesce_stats() -> dict:
    out = (C.c_uint64 * 3)()
    _lib.load_hip().pg_hmm_coalesce_stats(out)
    return {"merged_jobs": int(out[0]), "calls": int(out[1]), "largest_merge": int(out[2])}


def genotype_contigs_threaded(batches: Sequence[ContigBatch], table: ProbabilityTable, params=None, device: int = 0,
                              n_threads: Optional[int] = None, into: Optional[Sequence[ContigResult]] = None):
    """The reference's calling pattern (src/commands.cpp:949-978): one one-shot call per contig from `n_threads`
    worker threads (default: one per batch).  `params` may be a list (one per batch).  Returns the list of
    ContigResult / raised exceptions, in batch order."""
    import threading
    n = len(batches)
    n_threads = n_threads or n
    plist = list(params) if isinstance(params, (list, tuple)) else [params] * n
    out: list = [None] * n
    nxt = [0]
    lock = threading.Lock()

    n_workers = min(n_threads, n)
    for _ in range(n_workers):  # the pool's workers all pick up their first job at once: announce those calls up front
        announce(device)

    def worker():
        first = True
        while True:
            with lock:
                i = nxt[0]
                nxt[0] += 1
            if i >= n:
                if first:
                    _lib.load_hip().pg_hmm_retract(device)
                return
            if not first:
                announce(device)
            first = False
            try:
                out[i] = genotype_contig(batches[i], table, plist[i], device, announced=True, into=into[i] if into else None)
            except Exception as e:  # noqa: BLE001 - handed to the caller
                out[i] = e

    ts = [threading.Thread(target=worker) for _ in range(n_workers)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return out


class Job:
    """Resident multi-chain job: upload once, run many times (bench / pipelines).

    Job(batches, ...)                      one chain per batch (contig x path subset)
    Job.cohort(index, samples, ...)        chains = samples x contigs over ONE shared index
                                           (include/pangenie_hmm.h: pg_cohort_new); chain id =
                                           sample * n_contigs + contig
    """

    def __init__(self, batches: Sequence[ContigBatch], table: ProbabilityTable,
                 params: Optional[PgHmmParams] = None, device: int = 0, _cohort=None):
        self._lib = _lib.load_hip()
        self.table = table
        self.params = params or make_params()
        self.index = list(batches)
        self._arr = (PgContigBatch * len(self.index))(*[b.as_c() for b in self.index])
        err = C.create_string_buffer(_ERRLEN)
        h = C.c_void_p()
        if _cohort is None:
            self.batches = self.index
            self._samples = None
            rc = self._lib.pg_job_new(device, len(self.index), self._arr, table.h, C.byref(self.params),
                                      C.byref(h), err, _ERRLEN)
        else:
            self._samples, self._keep = self._marshal_samples(_cohort)
            self.batches = [b.with_counts(kc, cov) for (kcs, covs) in _cohort for b, kc, cov in zip(self.index, kcs, covs)]
            rc = self._lib.pg_cohort_new(device, len(self.index), self._arr, len(_cohort), self._samples, table.h,
                                         C.byref(self.params), C.byref(h), err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))
        self.h = h.value

    @classmethod
    def from_handle(cls, handle: int, table: ProbabilityTable, params: PgHmmParams, positions: Optional[Sequence[np.ndarray]] = None) -> "Job":
        """A job made elsewhere behind the C ABI (pg_sampler_then_job): its panels are read back from the device
        (pg_job_fetch_panel) so that results can be fetched and interpreted like any other job's."""
        self = cls.__new__(cls)
        self._lib = _lib.load_hip()
        self.table, self.params, self.h = table, params, handle
        self._samples = None
        self.batches = [self.fetch_panel(c) for c in range(self.n_chains)]
        self.index = self.batches
        return self

    def fetch_panel(self, contig: int) -> ContigBatch:
        """pg_job_fetch_panel: the inputs chain `contig` holds on the device as a ContigBatch (positions and coverage are
        not part of what the C ABI returns here: zeros)."""
        V, H, sK, sA = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        if self._lib.pg_job_panel_sizes(self.h, contig, C.byref(V), C.byref(H), C.byref(sK), C.byref(sA)):
            raise PanGenieError(-1, "pg_job_panel_sizes")
        V, H, sK, sA = V.value, H.value, sK.value, sA.value
        z = lambda n, dt: np.zeros(max(int(n), 1), dt)
        koff, aoff = z(V + 1, np.uint32), z(V + 1, np.uint32)
        kc, aid, afl, ako, akm, pa = z(sK, np.uint16), z(sA, np.uint16), z(sA, np.uint8), z(sA, np.uint16), z(sA, np.uint32), z(V * H, np.uint16)
        err = C.create_string_buffer(_ERRLEN)
        p = lambda a, t: a.ctypes.data_as(t)
        rc = self._lib.pg_job_fetch_panel(self.h, contig, p(koff, _lib.u32p), p(kc, u16p), p(aoff, _lib.u32p), p(aid, u16p), p(afl, u8p),
                                          p(ako, u16p), p(akm, _lib.u32p), p(pa, u16p), err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))
        return ContigBatch(H, np.zeros(V, np.uint64), np.zeros(V, np.uint16), koff[:V + 1], kc[:sK], aoff[:V + 1], aid[:sA], afl[:sA],
                           ako[:sA], akm[:sA], pa[:V * H])

    @classmethod
    def cohort(cls, index: Sequence[ContigBatch], samples, table: ProbabilityTable,
               params: Optional[PgHmmParams] = None, device: int = 0) -> "Job":
        """samples: list (one entry per sample) of (kmer_counts, coverages), each a list with one uint16
        array per index contig."""
        return cls(index, table, params, device, _cohort=list(samples))

    def _marshal_samples(self, samples):
        n, nc = len(samples), len(self.index)
        arr = (PgSampleCounts * n)()
        keep = []
        for s, (kcs, covs) in enumerate(samples):
            assert len(kcs) == nc and len(covs) == nc
            kc = [np.ascontiguousarray(a, np.uint16) if len(a) else np.zeros(1, np.uint16) for a in kcs]
            cv = [np.ascontiguousarray(a, np.uint16) if len(a) else np.zeros(1, np.uint16) for a in covs]
            pk = (u16p * nc)(*[a.ctypes.data_as(u16p) for a in kc])
            pc = (u16p * nc)(*[a.ctypes.data_as(u16p) for a in cv])
            arr[s].kmer_count = pk
            arr[s].coverage = pc
            keep += [kc, cv, pk, pc]
        return arr, keep

    @property
    def n_chains(self) -> int:
        return int(self._lib.pg_job_n_chains(self.h))

    def upload(self, samples=None) -> None:
        """Re-upload the inputs (same shapes): all arrays of a plain job; for a cohort job the given
        per-sample counts (index stays resident)."""
        err = C.create_string_buffer(_ERRLEN)
        if self._samples is None:
            rc = self._lib.pg_job_upload(self.h, self._arr, None, err, _ERRLEN)
        else:
            if samples is not None:
                self._samples, self._keep = self._marshal_samples(list(samples))
            rc = self._lib.pg_job_upload(self.h, None, self._samples, err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))

    def upload_run(self) -> None:
        """pg_job_upload_run: re-upload every input and run, in one call (the upload of the shorter chains hides behind the long
        chains' phase 1 where the job can do that); a plain (non-cohort) job."""
        if self._samples is not None:
            raise PanGenieError(-2, "upload_run: a cohort job uploads samples with upload() / upload_begin()")
        err = C.create_string_buffer(_ERRLEN)
        rc = self._lib.pg_job_upload_run(self.h, self._arr, None, err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))

    def upload_begin(self, samples=None) -> None:
        """pg_job_upload_begin: start copying the next batch of samples of a cohort job into the job's second set of
        per-sample arrays while the current batch is genotyped (run()); upload_end() makes it the current one.  Fetch
        the previous run's results before upload_end()."""
        if self._samples is None:
            raise PanGenieError(-2, "upload_begin: not a cohort job")
        # marshalled into locals: when an upload is already in flight the C side refuses this call, and the uploader thread
        # is still reading the FIRST call's arrays — which only self._next_* keep alive
        if samples is not None:
            nxt, keep = self._marshal_samples(list(samples))
        else:
            nxt, keep = self._samples, self._keep
        err = C.create_string_buffer(_ERRLEN)
        rc = self._lib.pg_job_upload_begin(self.h, nxt, err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))
        self._next_samples, self._next_keep = nxt, keep

    def upload_end(self) -> None:
        err = C.create_string_buffer(_ERRLEN)
        rc = self._lib.pg_job_upload_end(self.h, err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))
        self._samples, self._keep = self._next_samples, self._next_keep

    def host_seconds(self) -> dict:
        out = (C.c_double * 4)()
        self._lib.pg_job_host_seconds(self.h, out)
        return {"alloc_s": out[0], "upload_s": out[1], "run_s": out[2], "fetch_s": out[3]}

    def upload_bytes(self) -> dict:
        out = (C.c_uint64 * 2)()
        self._lib.pg_job_upload_bytes(self.h, out)
        return {"index": int(out[0]), "samples": int(out[1])}

    def packed_results(self):
        """(lik_ptr, lik_exp_ptr, n_lik_total): the posteriors of all chains as two packed device ranges."""
        d_lik, d_exp, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._lib.pg_job_packed_results(self.h, C.byref(d_lik), C.byref(d_exp), C.byref(n))
        return d_lik.value, d_exp.value, int(n.value)

    def run(self, stream: int = 0) -> None:
        err = C.create_string_buffer(_ERRLEN)
        rc = self._lib.pg_job_run(self.h, C.c_void_p(stream) if stream else None, err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))

    def fetch(self, contig: int) -> ContigResult:
        res = ContigResult(self.batches[contig])
        err = C.create_string_buffer(_ERRLEN)
        rc = self._lib.pg_job_fetch(self.h, contig, C.byref(res._c), err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))
        res.n_columns = int(res._c.n_columns)
        res.run_genotyping = bool(self.params.run_genotyping)
        return res

    def fetch_all(self, into: Optional[Sequence[ContigResult]] = None) -> List[ContigResult]:
        """pg_job_fetch_all: every chain's results with one synchronisation; `into` = buffers to reuse."""
        res = list(into) if into is not None else [ContigResult(b) for b in self.batches]
        arr = (PgContigResult * len(res))(*[r._c for r in res])
        err = C.create_string_buffer(_ERRLEN)
        rc = self._lib.pg_job_fetch_all(self.h, arr, err, _ERRLEN)
        if rc:
            raise PanGenieError(rc, err.value.decode(errors="replace"))
        for r, c in zip(res, arr):
            r.n_columns = int(c.n_columns)
            r.run_genotyping = bool(self.params.run_genotyping)
        return res

    def calls(self, contig: Optional[int] = None):
        """pg_job_calls + pg_job_fetch_calls[_all]: GT and GQ per variant formed on the device (pangenie_amd/calls.py,
        DESIGN.md 4e) — 8 bytes per variant cross PCIe instead of every bin.  Returns one record array (calls.CALL_DTYPE)
        per chain, or chain `contig`'s alone."""
        from . import calls as _calls
        return _calls.job_calls(self, contig)

    def calls_ms(self) -> float:
        """elapsed ms of the kernels of the last calls()"""
        return float(self._lib.pg_job_calls_ms(self.h))

    def record_plan(self, contig: int, plan) -> None:
        """pg_job_record_plan: checks and uploads the record plan (calls.RecordPlan) of INDEX contig `contig`; every chain
        over that contig shares it, a second plan replaces the first."""
        from . import calls as _calls
        _calls.job_record_plan(self, contig, plan)

    def record_calls(self, contig: Optional[int] = None):
        """pg_job_record_calls + pg_job_fetch_record_calls[_all]: GT and GQ per VCF RECORD formed on the device (DESIGN.md 4e
        "Records").  Returns one record array (calls.CALL_DTYPE) per chain — empty for a chain whose index contig has no
        plan — or chain `contig`'s alone."""
        from . import calls as _calls
        return _calls.job_record_calls(self, contig)

    def record_calls_ms(self) -> float:
        """elapsed ms of the kernels of the last record_calls()"""
        return float(self._lib.pg_job_record_calls_ms(self.h))

    def record_gl(self, contig: Optional[int] = None):
        """pg_job_record_gl + pg_job_fetch_record_gl[_all]: the GL column per VCF RECORD formed on the device:
        four digits of log10 of every genotype's likelihood over the record's defined alleles.  Returns one value array
        (calls.GL_DTYPE) per chain, laid out by calls.record_gl_offsets(plan) — empty for a chain whose index contig has no
        plan — or chain `contig`'s alone."""
        from . import calls as _calls
        return _calls.job_record_gl(self, contig)

    def record_gl_ms(self) -> float:
        """elapsed ms of the kernels of the last record_gl()"""
        return float(self._lib.pg_job_record_gl_ms(self.h))

    def record_plan_strided(self, contig: int, n_contigs: int, plan) -> None:
        """pg_job_record_plan_strided: ONE plan, checked and uploaded once, for every index contig ix with ix % n_contigs ==
        contig — the chains sample * n_contigs + contig of a sampled cohort job, where every chain is its own index contig
        (DESIGN.md 4e-3)."""
        from . import calls as _calls
        _calls.job_record_plan_strided(self, contig, n_contigs, plan)

    def record_first(self):
        """pg_job_record_first: (calls_first, gl_first), [n_chains + 1] offsets in elements into the packed records / GL values
        (after record_calls(); gl_first is None until record_gl() has run)."""
        from . import calls as _calls
        return _calls.job_record_first(self)

    def record_calls_packed(self):
        """pg_job_fetch_record_calls_packed: (all chains' records as one calls.CALL_DTYPE array from ONE copy, calls_first);
        after record_calls()."""
        from . import calls as _calls
        return _calls.fetch_record_calls_packed(self)

    def record_gl_packed(self):
        """pg_job_fetch_record_gl_packed: (all chains' GL values as one calls.GL_DTYPE array from ONE copy, gl_first); after
        record_gl()."""
        from . import calls as _calls
        return _calls.fetch_record_gl_packed(self)

    def record_text(self, contig: Optional[int] = None, ignore_imputed: bool = False):
        """pg_job_record_text + pg_job_fetch_record_text: the bytes of the GT:GQ:GL:KC column per VCF RECORD formed on the
        device, under the plans of record_plan().  (off, bytes) of chain `contig` — record r's text is
        bytes[off[r]:off[r + 1]], empty for a record left to the host — or a list of them, one per chain."""
        from . import calls as _calls
        return _calls.job_record_text(self, contig, ignore_imputed)

    def record_text_packed(self, ignore_imputed: bool = False):
        """pg_job_record_text + pg_job_fetch_record_text_packed: (off [R_total + 1] absolute, all chains' bytes from ONE copy,
        text_first [n_chains + 1])."""
        from . import calls as _calls
        _calls.form_record_text(self, ignore_imputed)
        return _calls.fetch_record_text_packed(self)

    def record_text_ms(self) -> float:
        """elapsed ms of the kernels of the last record_text()"""
        return float(self._lib.pg_job_record_text_ms(self.h))

    def line_prefix(self, contig: int, off, data, slot=None) -> None:
        """pg_job_line_prefix: the fixed columns (CHROM .. FORMAT, no trailing tab) of the records of INDEX contig `contig`,
        record r's = data[off[r]:off[r + 1]]; after record_plan().  A second call replaces them.  With
        slot [R] (pg_job_line_prefix_slotted) the decimal UK of the record's bubble in the contig's first
        member chain is printed on the device in front of byte slot[r] of record r's columns."""
        from . import calls as _calls
        _calls.job_line_prefix(self, contig, off, data, slot)

    def line_prefix_strided(self, contig: int, n_contigs: int, off, data, slot=None) -> None:
        """pg_job_line_prefix_strided: ONE prefix, checked and uploaded once, for every index contig ix with ix % n_contigs ==
        contig — the chains of one chromosome in a sampled cohort; after record_plan_strided().  A later
        line_prefix() on one member replaces that member's alone."""
        from . import calls as _calls
        _calls.job_line_prefix_strided(self, contig, n_contigs, off, data, slot)

    def record_lines(self, contig: Optional[int] = None):
        """pg_job_record_lines + pg_job_fetch_record_lines: whole VCF lines — the prefix, every member's text behind a tab, a
        newline — joined on the device from the text of the last record_text().  (off, bytes) of index
        contig `contig`, or a list of them, one per index contig; a line of length 0 is the host's."""
        from . import calls as _calls
        return _calls.job_record_lines(self, contig)

    def record_lines_packed(self):
        """pg_job_record_lines + pg_job_fetch_record_lines_packed: (off [n_lines + 1] absolute, all bytes from ONE copy,
        line_first, byte_first [n_index_contigs + 1])."""
        from . import calls as _calls
        _calls.form_record_lines(self)
        return _calls.fetch_record_lines_packed(self)

    def record_lines_ms(self) -> float:
        """elapsed ms of the kernels of the last record_lines()"""
        return float(self._lib.pg_job_record_lines_ms(self.h))

    def record_phase(self, contig: Optional[int] = None):
        """pg_job_record_phase + the fetches: of a run_phasing job, per VCF RECORD the two GT numbers of the phasing column
        (calls.PHASE_DTYPE; PG_PHASE_UNDEFINED prints `.`) from the Viterbi haplotypes on the device.  One
        array per chain (empty for a chain whose index contig has no plan), or chain `contig`'s."""
        from . import calls as _calls
        return _calls.job_record_phase(self, contig)

    def record_phase_ms(self) -> float:
        """elapsed ms of the kernel of the last record_phase()"""
        return float(self._lib.pg_job_record_phase_ms(self.h))

    def phased_text(self, contig: Optional[int] = None, ignore_imputed: bool = False):
        """pg_job_phased_text + pg_job_fetch_phased_text: the bytes of the GT:KC column per VCF RECORD (`a|b:KC`, `./.:KC` for a
        bubble without unique k-mers under ignore_imputed).  (off [R + 1], bytes) per chain, or chain `contig`'s."""
        from . import calls as _calls
        return _calls.job_phased_text(self, contig, ignore_imputed)

    def phased_text_packed(self, ignore_imputed: bool = False):
        """pg_job_phased_text + pg_job_fetch_phased_text_packed: (off [R_total + 1] absolute, all chains' bytes from ONE copy,
        record_first, text_first [n_chains + 1])."""
        from . import calls as _calls
        _calls.form_phased_text(self, ignore_imputed)
        return _calls.fetch_phased_text_packed(self)

    def phased_text_ms(self) -> float:
        """elapsed ms of the kernels of the last phased_text()"""
        return float(self._lib.pg_job_phased_text_ms(self.h))

    def phased_line_prefix(self, contig: int, off, data) -> None:
        """pg_job_phased_line_prefix: the fixed columns (CHROM .. INFO, GT:KC, no trailing tab) of the records of INDEX contig
        `contig` for the phased lines: a family of prefixes of its own beside line_prefix()'s."""
        from . import calls as _calls
        _calls.job_phased_line_prefix(self, contig, off, data)

    def phased_lines(self, contig: Optional[int] = None):
        """pg_job_phased_lines + pg_job_fetch_phased_lines: whole lines of the phasing VCF joined on the device from the text
        of the last phased_text().  (off, bytes) of index contig `contig`, or of all."""
        from . import calls as _calls
        return _calls.job_phased_lines(self, contig)

    def phased_lines_packed(self):
        """pg_job_phased_lines + pg_job_fetch_phased_lines_packed: (off [n_lines + 1] absolute, all bytes from ONE copy,
        line_first, byte_first [n_index_contigs + 1])."""
        from . import calls as _calls
        _calls.form_phased_lines(self)
        return _calls.fetch_phased_lines_packed(self)

    def phased_lines_ms(self) -> float:
        """elapsed ms of the kernels of the last phased_lines()"""
        return float(self._lib.pg_job_phased_lines_ms(self.h))

    def panel_text(self, contig: Optional[int] = None):
        """pg_job_panel_text + pg_job_fetch_panel_text: the sample columns of the sampled-panel VCF per VCF RECORD — one cell
        per path of the chain's panel, joined by tabs — formed on the device from the panel the job holds;
        needs a record plan, no run().  (off [R + 1], bytes) per chain, or chain `contig`'s."""
        from . import calls as _calls
        return _calls.job_panel_text(self, contig)

    def panel_text_packed(self):
        """pg_job_panel_text + pg_job_fetch_panel_text_packed: (off [R_total + 1] absolute, all chains' bytes from ONE copy,
        record_first, text_first [n_chains + 1])."""
        from . import calls as _calls
        _calls.form_panel_text(self)
        return _calls.fetch_panel_text_packed(self)

    def panel_text_ms(self) -> float:
        """elapsed ms of the kernels of the last panel_text()"""
        return float(self._lib.pg_job_panel_text_ms(self.h))

    def panel_line_prefix(self, contig: int, off, data, slot=None) -> None:
        """pg_job_panel_line_prefix[_slotted]: the fixed columns (CHROM .. INFO, GT, no trailing tab) of the records of INDEX
        contig `contig` for the panel lines; with slot [R] the panel's own UK is printed in front of byte slot[r]."""
        from . import calls as _calls
        _calls.job_panel_line_prefix(self, contig, off, data, slot)

    def panel_line_prefix_strided(self, contig: int, n_contigs: int, off, data, slot=None) -> None:
        """pg_job_panel_line_prefix_strided: ONE prefix for every index contig ix with ix % n_contigs == contig."""
        from . import calls as _calls
        _calls.job_panel_line_prefix_strided(self, contig, n_contigs, off, data, slot)

    def panel_lines(self, contig: Optional[int] = None):
        """pg_job_panel_lines + pg_job_fetch_panel_lines: whole lines of the sampled-panel VCF joined on the device from the
        text of the last panel_text().  (off, bytes) of index contig `contig`, or of all."""
        from . import calls as _calls
        return _calls.job_panel_lines(self, contig)

    def panel_lines_packed(self):
        """pg_job_panel_lines + pg_job_fetch_panel_lines_packed: (off [n_lines + 1] absolute, all bytes from ONE copy,
        line_first, byte_first [n_index_contigs + 1])."""
        from . import calls as _calls
        _calls.form_panel_lines(self)
        return _calls.fetch_panel_lines_packed(self)

    def panel_lines_ms(self) -> float:
        """elapsed ms of the kernels of the last panel_lines()"""
        return float(self._lib.pg_job_panel_lines_ms(self.h))

    def combine_plan(self, groups) -> None:
        """pg_job_combine_plan: groups = per group the chains (contig x path subset) that genotype the same index objects, in the
        order they are to be added up; a second plan replaces the first."""
        from . import calls as _calls
        _calls.job_combine_plan(self, groups)

    def combine(self) -> None:
        """pg_job_combine: adds up every group's chains key by key on the device, from the bins of the last run()."""
        from . import calls as _calls
        _calls.job_combine(self)

    def combined(self, group: Optional[int] = None):
        """pg_job_fetch_combined[_all]: the combined bins of `group` (or of every group) as a structured array m, e, flags
        (calls.COMBINED_DTYPE; calls.combined_to_longdouble gives the values); after combine()."""
        from . import calls as _calls
        return _calls.fetch_combined(self, group)

    def combined_calls(self, group: Optional[int] = None):
        """pg_job_combined_calls + pg_job_fetch_combined_calls[_all]: GT and GQ per variant of every group from its combined
        bins (calls.CALL_DTYPE per group, or `group`'s alone); after combine()."""
        from . import calls as _calls
        return _calls.job_combined_calls(self, group)

    def combine_ms(self) -> float:
        """elapsed ms of the kernels of the last combine()"""
        return float(self._lib.pg_job_combine_ms(self.h))

    def combined_calls_ms(self) -> float:
        """elapsed ms of the kernels of the last combined_calls()"""
        return float(self._lib.pg_job_combined_calls_ms(self.h))

    def combined_record_calls(self, group: Optional[int] = None):
        """pg_job_combined_record_calls + pg_job_fetch_combined_record_calls[_all]: GT and GQ per VCF RECORD of every group from
        its combined bins, under the record plan of the group's first chain's index contig.  One record array
        (calls.CALL_DTYPE) per group — empty for a group without a plan — or `group`'s alone; after combine()."""
        from . import calls as _calls
        return _calls.job_combined_record_calls(self, group)

    def combined_record_gl(self, group: Optional[int] = None):
        """pg_job_combined_record_gl + pg_job_fetch_combined_record_gl[_all]: the GL column per VCF RECORD of every group from its
        combined bins (calls.GL_DTYPE per group, laid out by calls.record_gl_offsets(plan), or `group`'s alone); after combine()."""
        from . import calls as _calls
        return _calls.job_combined_record_gl(self, group)

    def combined_record_calls_ms(self) -> float:
        """elapsed ms of the kernels of the last combined_record_calls()"""
        return float(self._lib.pg_job_combined_record_calls_ms(self.h))

    def combined_record_gl_ms(self) -> float:
        """elapsed ms of the kernels of the last combined_record_gl()"""
        return float(self._lib.pg_job_combined_record_gl_ms(self.h))

    def viterbi_ms(self) -> float:
        """elapsed ms of the Viterbi kernels (run_phasing) of the last run"""
        return float(self._lib.pg_job_viterbi_ms(self.h))

    def device_results(self, contig: int):
        """(lik_ptr, n_lik, lik_exp_ptr, n_variants): device pointers for an RCCL gather."""
        d_lik, d_exp = C.c_void_p(), C.c_void_p()
        n_lik, n_var = C.c_uint64(), C.c_uint64()
        self._lib.pg_job_device_results(self.h, contig, C.byref(d_lik), C.byref(n_lik),
                                        C.byref(d_exp), C.byref(n_var))
        return d_lik.value, n_lik.value, d_exp.value, n_var.value

    def index_ms(self) -> float:
        """pg_job_index_ms: hipEvent time of the last index pass (what the index alone decides, formed once per uploaded index)"""
        return float(self._lib.pg_job_index_ms(self.h))

    def plan(self) -> str:
        """pg_job_plan: which kernels run for which chains of this job"""
        n = int(self._lib.pg_job_plan(self.h, None, 0))
        buf = C.create_string_buffer(n)
        self._lib.pg_job_plan(self.h, buf, n)
        return buf.value.decode(errors="replace")

    def kernel_ms(self) -> dict:
        ms = (C.c_double * PG_N_KERNEL_CLASSES)()
        self._lib.pg_job_kernel_ms(self.h, ms)
        return {self._lib.pg_job_kernel_name(i).decode(): ms[i] for i in range(PG_N_KERNEL_CLASSES)}

    def profile_counters(self, contig: int = 0) -> np.ndarray:
        out = np.zeros(64, np.uint64)
        self._lib.pg_job_profile_counters(self.h, contig, out.ctypes.data_as(u64p))
        return out

    def device_bytes(self) -> int:
        return int(self._lib.pg_job_device_bytes(self.h))

    def sweep_mode(self):
        """("fused" | "chunked", chunk_cols) — see include/pangenie_hmm.h:pg_job_sweep_mode."""
        k = C.c_uint32(0)
        m = self._lib.pg_job_sweep_mode(self.h, C.byref(k))
        return ("chunked" if m == 1 else "fused"), int(k.value)

    def triangle_chains(self) -> int:
        """chains whose columns are stored as upper triangles (fused jobs, lean chains)"""
        return int(self._lib.pg_job_triangle_chains(self.h))

    def close(self):
        if getattr(self, "h", None):
            self._lib.pg_job_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def emission_table(batch: ContigBatch, table: ProbabilityTable, v: int, device: int = 0):
    """EmissionProbabilityComputer of variant v on the device (A x A over all allele slots)."""
    lib = _lib.load_hip()
    A = int(batch.allele_off[v + 1] - batch.allele_off[v])
    out = np.zeros(A * A, dtype=LD)
    az = C.c_int32(0)
    err = C.create_string_buffer(_ERRLEN)
    rc = lib.pg_emission_table(C.byref(batch.as_c()), table.h, v, device, out.ctypes.data_as(ldp),
                               C.byref(az), err, _ERRLEN)
    if rc:
        raise PanGenieError(rc, err.value.decode(errors="replace"))
    return out.reshape(A, A), bool(az.value)


def transition_probs(from_pos: int, to_pos: int, recombrate: float, nr_paths: int, uniform: bool,
                     effective_N, device: int = 0) -> np.ndarray:
    """TransitionProbabilityComputer on the device: {no switch, one switch, two switches}."""
    lib = _lib.load_hip()
    out = (C.c_double * 3)()
    err = C.create_string_buffer(_ERRLEN)
    rc = lib.pg_transition_probs(from_pos, to_pos, recombrate, nr_paths, int(uniform), _lib.c_ld(effective_N),
                                 device, out, err, _ERRLEN)
    if rc:
        raise PanGenieError(rc, err.value.decode(errors="replace"))
    return np.array([out[0], out[1], out[2]])
