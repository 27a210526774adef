"""Genotype calls formed on the device (include/pangenie_hmm.h: pg_job_calls, pg_calls_from_bins).

One 8-byte record per variant — allele ids of the likeliest genotype, genotype quality, a flag — holding what
GenotypingResult.normalize / get_likeliest_genotype / get_genotype_quality (genotyping_result.py, the reference's
src/genotypingresult.cpp:118-210) give on the same bins.  The kernels are pangenie_amd/csrc/pg_calls.hip; nothing is
computed here.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from . import _lib

CALL_DTYPE = np.dtype([("allele_1", "<u2"), ("allele_2", "<u2"), ("gq", "<u2"), ("flags", "<u2")])
PG_CALL_OK = 0          # a unique likeliest genotype
PG_CALL_NONE = 1        # ./. : not a kept column, no key, every bin zero
PG_CALL_NOT_UNIQUE = 2  # ./. : another genotype within 1e-10 of the best
PG_CALL_DEFERRED = 3    # largest bin below 2^-16300: to be decided on the host from this variant's bins
PG_CALL_EMPTY = 0x100   # record calls, with PG_CALL_OK: 0/0 and GQ 10000 of a bubble without any likelihood
_ERRLEN = 512


def _error(rc: int, err) -> Exception:
    from .hmm import PanGenieError
    return PanGenieError(rc, err.value.decode(errors="replace") if err is not None else "pg_calls_from_bins")


def job_calls(job, contig: Optional[int] = None):
    """Job.calls(): forms the calls of every chain, fetches all of them (or chain `contig`'s)."""
    lib = job._lib
    err = C.create_string_buffer(_ERRLEN)
    rc = lib.pg_job_calls(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    if contig is not None:
        return fetch_calls(job, contig)
    return fetch_calls_all(job)


def fetch_calls(job, contig: int) -> np.ndarray:
    out = np.zeros(max(job.batches[contig].n_variants, 1), CALL_DTYPE)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_calls(job.h, contig, out.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return out[:job.batches[contig].n_variants]


def fetch_calls_all(job) -> List[np.ndarray]:
    outs = [np.zeros(max(b.n_variants, 1), CALL_DTYPE) for b in job.batches]
    arr = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_calls_all(job.h, arr, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return [o[:b.n_variants] for o, b in zip(outs, job.batches)]


def calls_from_bins(allele_off, allele_id, kept, allele_present, lik, lik_exp, device: int = 0) -> np.ndarray:
    """pg_calls_from_bins: the calls of V variants from host arrays in the layout of ContigBatch / ContigResult
    (allele_off [V+1], allele_id / allele_present [sumA], kept [V], lik / lik_exp [sum A (A + 1) / 2])."""
    lib = _lib.load_hip()
    aoff = np.ascontiguousarray(allele_off, np.uint32)
    V = len(aoff) - 1
    pad = lambda a, dt: np.ascontiguousarray(a, dt) if len(a) else np.zeros(1, dt)
    aid, kp, pres = pad(allele_id, np.uint16), pad(kept, np.uint8), pad(allele_present, np.uint8)
    lk, le = pad(lik, np.float64), pad(lik_exp, np.int32)
    A = np.diff(aoff.astype(np.int64))
    if len(allele_id) != int(aoff[-1]) or len(allele_present) != int(aoff[-1]) or len(kept) != V or len(lik) != int((A * (A + 1) // 2).sum()) \
            or len(lik_exp) != len(lik):
        raise ValueError("calls_from_bins: array lengths do not match allele_off")
    out = np.zeros(max(V, 1), CALL_DTYPE)
    rc = lib.pg_calls_from_bins(device, V, aoff.ctypes.data_as(_lib.u32p), aid.ctypes.data_as(_lib.u16p), kp.ctypes.data_as(_lib.u8p),
                                pres.ctypes.data_as(_lib.u8p), lk.ctypes.data_as(_lib.f64p), le.ctypes.data_as(_lib.i32p), out.ctypes.data)
    if rc:
        raise _error(rc, None)
    return out[:V]



# ---------------------------------------------------------------------------------------------------------------
#  Calls per VCF record (pg_job_record_plan, pg_job_record_calls, pg_record_calls_from_bins; DESIGN.md 4e "Records")
# ---------------------------------------------------------------------------------------------------------------
class PgRecordPlan(C.Structure):
    _fields_ = [("n_variants", C.c_uint32), ("n_records", C.c_uint32), ("rec_off", _lib.u32p), ("map_off", _lib.u32p), ("map", _lib.u16p),
                ("n_alleles", _lib.u16p), ("vcf_off", _lib.u32p), ("vcf_index", _lib.u16p)]


class RecordPlan:
    """What the bubbles of one index contig mean for their VCF records (pg_record_plan): rec_off [V+1] the records of every
    bubble; per record r the map from bubble allele ID to record allele (map[map_off[r] + id]), its number of alleles, and
    for every record allele its index among the defined ones (vcf_index, 0xFFFF: undefined sequence).  Nothing is checked
    here: the library does that."""

    def __init__(self, rec_off, map_off, map, n_alleles, vcf_off, vcf_index):
        self.rec_off = np.ascontiguousarray(rec_off, np.uint32)
        self.map_off = np.ascontiguousarray(map_off, np.uint32)
        self.n_alleles = np.ascontiguousarray(n_alleles, np.uint16)
        self.vcf_off = np.ascontiguousarray(vcf_off, np.uint32)
        pad = lambda a: np.ascontiguousarray(a, np.uint16) if len(a) else np.zeros(1, np.uint16)
        self.map, self.vcf_index = pad(map), pad(vcf_index)
        if len(self.n_alleles) == 0:
            self.n_alleles = np.zeros(1, np.uint16)

    @property
    def n_variants(self) -> int:
        return len(self.rec_off) - 1

    @property
    def n_records(self) -> int:
        return len(self.map_off) - 1

    @classmethod
    def from_records(cls, bubbles) -> "RecordPlan":
        """bubbles: per bubble a list of records, each (own, defined) — own[id] the record allele of bubble allele id,
        defined[a] whether record allele a has a defined sequence."""
        rec_off, map_off, mp, nal, vcf_off, vcf = [0], [0], [], [], [0], []
        for records in bubbles:
            for own, defined in records:
                mp += [int(x) for x in own]
                map_off.append(len(mp))
                nal.append(len(defined))
                d = 0
                for ok in defined:
                    vcf.append(d if ok else 0xFFFF)
                    d += 1 if ok else 0
                vcf_off.append(len(vcf))
            rec_off.append(len(nal))
        return cls(rec_off, map_off, mp, nal, vcf_off, vcf)

    def record(self, r: int):
        """(own, vcf_index) of record r"""
        return (self.map[int(self.map_off[r]):int(self.map_off[r + 1])], self.vcf_index[int(self.vcf_off[r]):int(self.vcf_off[r + 1])])

    def as_c(self) -> PgRecordPlan:
        p = lambda a, t: a.ctypes.data_as(t)
        return PgRecordPlan(self.n_variants, self.n_records, p(self.rec_off, _lib.u32p), p(self.map_off, _lib.u32p), p(self.map, _lib.u16p),
                            p(self.n_alleles, _lib.u16p), p(self.vcf_off, _lib.u32p), p(self.vcf_index, _lib.u16p))


def job_record_plan(job, contig: int, plan: RecordPlan) -> None:
    err = C.create_string_buffer(_ERRLEN)
    c = plan.as_c()
    rc = job._lib.pg_job_record_plan(job.h, contig, C.addressof(c), err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    if not hasattr(job, "_record_plans"):
        job._record_plans = {}
    job._record_plans[contig] = plan


def job_record_plan_strided(job, contig: int, n_contigs: int, plan: RecordPlan) -> None:
    """pg_job_record_plan_strided: one plan, checked and uploaded once, for every index contig ix with ix % n_contigs ==
    contig — the chains sample * n_contigs + contig of a sampled cohort job."""
    err = C.create_string_buffer(_ERRLEN)
    c = plan.as_c()
    rc = job._lib.pg_job_record_plan_strided(job.h, contig, n_contigs, C.addressof(c), err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    if not hasattr(job, "_record_plans"):
        job._record_plans = {}
    for ix in range(contig, len(job.index), n_contigs):
        job._record_plans[ix] = plan


def job_record_first(job):
    """pg_job_record_first: (calls_first, gl_first), [n_chains + 1] each — every chain's offset, in elements, in the packed
    records and the packed GL values; gl_first is None until record_gl() has run."""
    cf, gf = _record_first(job, True), None
    try:
        gf = _record_first(job, False)
    except Exception:   # (record_gl() has not run: the records' offsets alone)
        pass
    return cf, gf


def _record_first(job, calls: bool) -> np.ndarray:
    first = np.zeros(job.n_chains + 1, np.uint64)
    err = C.create_string_buffer(_ERRLEN)
    p = first.ctypes.data_as(_lib.u64p)
    rc = job._lib.pg_job_record_first(job.h, p if calls else None, None if calls else p, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return first


def fetch_record_calls_packed(job):
    """pg_job_fetch_record_calls_packed: (records of all chains as ONE array from one copy, calls_first)."""
    first = _record_first(job, True)
    out = np.zeros(max(int(first[-1]), 1), CALL_DTYPE)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_calls_packed(job.h, out.ctypes.data, int(first[-1]), err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return out[:int(first[-1])], first


def fetch_record_gl_packed(job):
    """pg_job_fetch_record_gl_packed: (GL values of all chains as ONE array from one copy, gl_first)."""
    first = _record_first(job, False)
    out = np.zeros(max(int(first[-1]), 1), GL_DTYPE)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_gl_packed(job.h, out.ctypes.data, int(first[-1]), err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return out[:int(first[-1])], first


def _n_records(job) -> List[int]:
    plans, nc = getattr(job, "_record_plans", {}), len(job.index)
    return [plans[c % nc].n_records if (c % nc) in plans else 0 for c in range(len(job.batches))]


def job_record_calls(job, contig: Optional[int] = None):
    """Job.record_calls(): forms the record calls of every chain that has a plan, fetches all of them (or chain `contig`'s)."""
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_record_calls(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    if contig is not None:
        return fetch_record_calls(job, contig)
    return fetch_record_calls_all(job)


def fetch_record_calls(job, contig: int) -> np.ndarray:
    R = _n_records(job)[contig]
    out = np.zeros(max(R, 1), CALL_DTYPE)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_calls(job.h, contig, out.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return out[:R]


def fetch_record_calls_all(job) -> List[np.ndarray]:
    Rs = _n_records(job)
    outs = [np.zeros(max(R, 1), CALL_DTYPE) for R in Rs]
    arr = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_calls_all(job.h, arr, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return [o[:R] for o, R in zip(outs, Rs)]


def record_calls_from_bins(allele_off, allele_id, kept, allele_present, lik, lik_exp, plan: RecordPlan, device: int = 0) -> np.ndarray:
    """pg_record_calls_from_bins: the calls of the plan's records from host arrays laid out as for calls_from_bins."""
    lib = _lib.load_hip()
    aoff = np.ascontiguousarray(allele_off, np.uint32)
    V = len(aoff) - 1
    pad = lambda a, dt: np.ascontiguousarray(a, dt) if len(a) else np.zeros(1, dt)
    aid, kp, pres = pad(allele_id, np.uint16), pad(kept, np.uint8), pad(allele_present, np.uint8)
    lk, le = pad(lik, np.float64), pad(lik_exp, np.int32)
    A = np.diff(aoff.astype(np.int64))
    if len(allele_id) != int(aoff[-1]) or len(allele_present) != int(aoff[-1]) or len(kept) != V or len(lik) != int((A * (A + 1) // 2).sum()) \
            or len(lik_exp) != len(lik):
        raise ValueError("record_calls_from_bins: array lengths do not match allele_off")
    out = np.zeros(max(plan.n_records, 1), CALL_DTYPE)
    c = plan.as_c()
    rc = lib.pg_record_calls_from_bins(device, V, aoff.ctypes.data_as(_lib.u32p), aid.ctypes.data_as(_lib.u16p), kp.ctypes.data_as(_lib.u8p),
                                       pres.ctypes.data_as(_lib.u8p), lk.ctypes.data_as(_lib.f64p), le.ctypes.data_as(_lib.i32p), C.addressof(c),
                                       out.ctypes.data)
    if rc:
        raise _error(rc, None)
    return out[:plan.n_records]


# ---------------------------------------------------------------------------------------------------------------
#  The GL column per VCF record (pg_job_record_gl, pg_record_gl_from_bins, pg_gl_from_values, pg_gl_text)
# ---------------------------------------------------------------------------------------------------------------
GL_DTYPE = np.dtype([("mant", "<i2"), ("exp10", "<i2")])
PG_GL_NEG_INF = -32768   # in exp10 (mant 0): likelihood 0 or no such key, prints "-inf"
PG_GL_DEFERRED = -32767  # in exp10 (mant 0): not decided on the device, to be formed on the host from the bins


def record_gl_offsets(plan: RecordPlan) -> np.ndarray:
    """pg_record_gl_offsets: gl_off [R + 1]; record r owns the values gl_off[r] .. gl_off[r + 1] - 1 of a chain, genotype
    (a <= b) over its defined alleles at b (b + 1) / 2 + a.  Host only."""
    lib = _lib.load_hip()
    off = np.zeros(plan.n_records + 1, np.uint64)
    c = plan.as_c()
    rc = lib.pg_record_gl_offsets(C.addressof(c), off.ctypes.data_as(_lib.u64p))
    if rc:
        raise _error(rc, None)
    return off


def _n_gl(job) -> List[int]:
    plans, nc = getattr(job, "_record_plans", {}), len(job.index)
    cache = job.__dict__.setdefault("_gl_counts", {})
    out = []
    for c in range(len(job.batches)):
        plan = plans.get(c % nc)
        if plan is None:
            out.append(0)
            continue
        if cache.get(c % nc, (None, 0))[0] is not plan:
            cache[c % nc] = (plan, int(record_gl_offsets(plan)[-1]))
        out.append(cache[c % nc][1])
    return out


def job_record_gl(job, contig: Optional[int] = None):
    """Job.record_gl(): forms the GL values of every chain that has a plan, fetches all of them (or chain `contig`'s)."""
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_record_gl(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    if contig is not None:
        return fetch_record_gl(job, contig)
    return fetch_record_gl_all(job)


def fetch_record_gl(job, contig: int) -> np.ndarray:
    N = _n_gl(job)[contig]
    out = np.zeros(max(N, 1), GL_DTYPE)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_gl(job.h, contig, out.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return out[:N]


def fetch_record_gl_all(job) -> List[np.ndarray]:
    Ns = _n_gl(job)
    outs = [np.zeros(max(N, 1), GL_DTYPE) for N in Ns]
    arr = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_gl_all(job.h, arr, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return [o[:N] for o, N in zip(outs, Ns)]


def record_gl_from_bins(allele_off, allele_id, kept, allele_present, lik, lik_exp, plan: RecordPlan, device: int = 0) -> np.ndarray:
    """pg_record_gl_from_bins: the GL values of the plan's records from host arrays laid out as for calls_from_bins; record
    r's values at record_gl_offsets(plan)[r] ..."""
    lib = _lib.load_hip()
    aoff = np.ascontiguousarray(allele_off, np.uint32)
    V = len(aoff) - 1
    pad = lambda a, dt: np.ascontiguousarray(a, dt) if len(a) else np.zeros(1, dt)
    aid, kp, pres = pad(allele_id, np.uint16), pad(kept, np.uint8), pad(allele_present, np.uint8)
    lk, le = pad(lik, np.float64), pad(lik_exp, np.int32)
    A = np.diff(aoff.astype(np.int64))
    if len(allele_id) != int(aoff[-1]) or len(allele_present) != int(aoff[-1]) or len(kept) != V or len(lik) != int((A * (A + 1) // 2).sum()) \
            or len(lik_exp) != len(lik):
        raise ValueError("record_gl_from_bins: array lengths do not match allele_off")
    N = int(record_gl_offsets(plan)[-1])
    out = np.zeros(max(N, 1), GL_DTYPE)
    c = plan.as_c()
    rc = lib.pg_record_gl_from_bins(device, V, aoff.ctypes.data_as(_lib.u32p), aid.ctypes.data_as(_lib.u16p), kp.ctypes.data_as(_lib.u8p),
                                    pres.ctypes.data_as(_lib.u8p), lk.ctypes.data_as(_lib.f64p), le.ctypes.data_as(_lib.i32p), C.addressof(c),
                                    out.ctypes.data)
    if rc:
        raise _error(rc, None)
    return out[:N]


def gl_from_values(m, e, device: int = 0) -> np.ndarray:
    """pg_gl_from_values: the GL of every likelihood m[i] * 2^e[i] (m[i] in [2^63, 2^64), or 0 with e[i] == 0) by the device's
    own log10 / log1p."""
    lib = _lib.load_hip()
    mm, ee = np.ascontiguousarray(m, np.uint64), np.ascontiguousarray(e, np.int32)
    if mm.shape != ee.shape or mm.ndim != 1:
        raise ValueError("gl_from_values: m and e must be one-dimensional and of one length")
    out = np.zeros(max(len(mm), 1), GL_DTYPE)
    if len(mm):
        rc = lib.pg_gl_from_values(device, len(mm), mm.ctypes.data_as(_lib.u64p), ee.ctypes.data_as(_lib.i32p), out.ctypes.data)
        if rc:
            raise _error(rc, None)
    return out[:len(mm)]


def gl_text(value) -> Optional[str]:
    """pg_gl_text: what the VCF shows of one value (a GL_DTYPE element or a (mant, exp10) pair); None for PG_GL_DEFERRED and
    for an encoding that is no value."""
    lib = _lib.load_hip()
    buf = C.create_string_buffer(32)
    n = lib.pg_gl_text(_lib.PgGl(int(value[0]), int(value[1])), buf, 32)
    return buf.value.decode() if n >= 0 else None


# ---------------------------------------------------------------------------------------------------------------
#  The sample column as text (pg_job_record_text, pg_record_text_from_fields)
# ---------------------------------------------------------------------------------------------------------------
def record_text_bound(n_records: int, n_gl_total: int) -> int:
    """pg_record_text_bound: bytes that always suffice for the text of n_records records with n_gl_total values."""
    return int(_lib.load_hip().pg_record_text_bound(int(n_records), int(n_gl_total)))


def _record_text_first(job) -> np.ndarray:
    first = np.zeros(job.n_chains + 1, np.uint64)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_record_text_first(job.h, first.ctypes.data_as(_lib.u64p), err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return first


def form_record_text(job, ignore_imputed: bool = False) -> None:
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_record_text(job.h, 1 if ignore_imputed else 0, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def fetch_record_text(job, contig: int):
    """pg_job_fetch_record_text: (off [R + 1], bytes) of chain `contig`; record r's text is bytes[off[r]:off[r + 1]]."""
    first = _record_text_first(job)
    n = int(first[contig + 1] - first[contig])
    off = np.zeros(_n_records(job)[contig] + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_text(job.h, contig, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes()


def fetch_record_text_packed(job):
    """pg_job_fetch_record_text_packed: (off [R_total + 1] absolute in the packed text, bytes, text_first [n_chains + 1])."""
    first = _record_text_first(job)
    n = int(first[-1])
    off = np.zeros(sum(_n_records(job)) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_text_packed(job.h, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes(), first


def job_record_text(job, contig: Optional[int] = None, ignore_imputed: bool = False):
    """Job.record_text(): forms the text of every chain that has a plan; (off, bytes) of chain `contig`, or of every chain."""
    form_record_text(job, ignore_imputed)
    if contig is not None:
        return fetch_record_text(job, contig)
    return [fetch_record_text(job, c) for c in range(job.n_chains)]


def record_text_from_fields(calls, gl_off, gl, kc, no_call=None, device: int = 0):
    """pg_record_text_from_fields: (off [R + 1], bytes) — the text of R records from their calls (CALL_DTYPE), their GL values
    (GL_DTYPE, record r's at gl_off[r] .. gl_off[r + 1]), kc [R] and no_call [R] (or None), through the job's kernels.  A
    record of length 0 is the host's."""
    lib = _lib.load_hip()
    cc, go = np.ascontiguousarray(calls, CALL_DTYPE), np.ascontiguousarray(gl_off, np.uint64)
    gg, kk = np.ascontiguousarray(gl, GL_DTYPE), np.ascontiguousarray(kc, np.uint16)
    nc = None if no_call is None else np.ascontiguousarray(no_call, np.uint8)
    R = len(cc)
    if len(go) != R + 1 or len(kk) != R or (nc is not None and len(nc) != R) or (R and int(go[-1]) != len(gg)):
        raise ValueError("record_text_from_fields: array lengths do not match")
    cap = record_text_bound(R, len(gg))
    off = np.zeros(R + 1, np.uint64)
    text = np.zeros(max(cap, 1), np.uint8)
    rc = lib.pg_record_text_from_fields(device, R, cc.ctypes.data, go.ctypes.data, gg.ctypes.data, kk.ctypes.data,
                                        None if nc is None else nc.ctypes.data, off.ctypes.data, text.ctypes.data, cap)
    if rc:
        raise _error(rc, None)
    return off, text[:int(off[-1])].tobytes()


# ---------------------------------------------------------------------------------------------------------------
#  Whole VCF lines of a cohort (pg_job_line_prefix, pg_job_record_lines, pg_record_lines_from_text)
# ---------------------------------------------------------------------------------------------------------------
def record_lines_bound(n_records: int, n_members: int, prefix_bytes: int, text_bytes: int) -> int:
    """pg_record_lines_bound: prefix_bytes + text_bytes + n_records (n_members + 1), reached when no line is the host's."""
    return int(_lib.load_hip().pg_record_lines_bound(int(n_records), int(n_members), int(prefix_bytes), int(text_bytes)))


def _as_bytes(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), np.uint8)
    return np.ascontiguousarray(data, np.uint8)


def record_lines_bound_slotted(n_records: int, n_members: int, prefix_bytes: int, text_bytes: int) -> int:
    """pg_record_lines_bound_slotted: record_lines_bound + 5 n_records, an upper bound (UK has at most 5 digits)."""
    return int(_lib.load_hip().pg_record_lines_bound_slotted(int(n_records), int(n_members), int(prefix_bytes), int(text_bytes)))


def _prefix_arrays(job, what: str, contig: int, off, data, slot):
    """the arrays of a prefix as the C ABI reads them (it reads R + 1 offsets and R slots: it cannot see a wrong R)"""
    oo, bb = np.ascontiguousarray(off, np.uint64), _as_bytes(data)
    plans = getattr(job, "_record_plans", {})
    if contig in plans and len(oo) != plans[contig].n_records + 1:
        raise ValueError("%s: %d offsets for a plan of %d records" % (what, len(oo), plans[contig].n_records))
    if len(oo) and int(oo[-1]) > len(bb):
        raise ValueError("%s: the offsets end behind the bytes" % what)
    ss = None
    if slot is not None:
        ss = np.ascontiguousarray(slot, np.uint32)
        if len(ss) + 1 != len(oo):
            raise ValueError("%s: %d slots for %d offsets" % (what, len(ss), len(oo)))
        ss = np.concatenate([ss, np.zeros(1, np.uint32)])   # (never empty: a null pointer means a plain prefix)
    return oo, bb, ss


def job_line_prefix(job, contig: int, off, data, slot=None) -> None:
    """pg_job_line_prefix[_slotted]: the fixed columns of index contig `contig`, record r's = data[off[r]:off[r + 1]]; with
    slot [R], the digits of the chain's UK go in front of byte slot[r] of it."""
    oo, bb, ss = _prefix_arrays(job, "line_prefix", contig, off, data, slot)
    err = C.create_string_buffer(_ERRLEN)
    po, pb = oo.ctypes.data if len(oo) else None, bb.ctypes.data if len(bb) else None
    if ss is None:
        rc = job._lib.pg_job_line_prefix(job.h, contig, po, pb, err, _ERRLEN)
    else:
        rc = job._lib.pg_job_line_prefix_slotted(job.h, contig, po, pb, ss.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def job_line_prefix_strided(job, contig: int, n_contigs: int, off, data, slot=None) -> None:
    """pg_job_line_prefix_strided: ONE prefix, checked and uploaded once, for every index contig ix with ix % n_contigs ==
    contig; slot as for job_line_prefix."""
    oo, bb, ss = _prefix_arrays(job, "line_prefix_strided", contig, off, data, slot)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_line_prefix_strided(job.h, contig, n_contigs, oo.ctypes.data if len(oo) else None, bb.ctypes.data if len(bb) else None,
                                             None if ss is None else ss.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def form_record_lines(job) -> None:
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_record_lines(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def record_lines_first(job):
    """pg_job_record_lines_first: (line_first, byte_first), each [n_index_contigs + 1]."""
    n = C.c_uint64(0)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_record_lines_first(job.h, C.byref(n), None, None, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    lf, bf = np.zeros(n.value + 1, np.uint64), np.zeros(n.value + 1, np.uint64)
    rc = job._lib.pg_job_record_lines_first(job.h, C.byref(n), lf.ctypes.data, bf.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return lf, bf


def fetch_record_lines(job, contig: int):
    """pg_job_fetch_record_lines: (off [R + 1], bytes) of index contig `contig`; line r is bytes[off[r]:off[r + 1]]."""
    lf, bf = record_lines_first(job)
    n = int(bf[contig + 1] - bf[contig])
    off = np.zeros(int(lf[contig + 1] - lf[contig]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_lines(job.h, contig, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes()


def fetch_record_lines_packed(job):
    """pg_job_fetch_record_lines_packed: (off [n_lines + 1] absolute, bytes, line_first, byte_first) from ONE copy."""
    lf, bf = record_lines_first(job)
    n = int(bf[-1])
    off = np.zeros(int(lf[-1]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_lines_packed(job.h, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes(), lf, bf


def job_record_lines(job, contig: Optional[int] = None):
    """Job.record_lines(): forms the lines from the record text as it is; (off, bytes) of index contig `contig`, or of all."""
    form_record_lines(job)
    if contig is not None:
        return fetch_record_lines(job, contig)
    return [fetch_record_lines(job, k) for k in range(len(record_lines_first(job)[0]) - 1)]


def record_lines_from_text(texts, prefix, device: int = 0):
    """pg_record_lines_from_text: (off [R + 1], bytes) — the lines of R records joined through the job's kernels.  texts = per
    member (off [R + 1], bytes), prefix = (off [R + 1], bytes): any bytes.  A line of length 0 is the host's."""
    lib = _lib.load_hip()
    po, pb = np.ascontiguousarray(prefix[0], np.uint64), _as_bytes(prefix[1])
    R, S = len(po) - 1, len(texts)
    offs = [np.ascontiguousarray(t[0], np.uint64) for t in texts]
    data = [_as_bytes(t[1]) for t in texts]
    if R < 0 or any(len(o) != R + 1 for o in offs) or any(int(o[-1]) > len(b) for o, b in zip(offs + [po], data + [pb])):
        raise ValueError("record_lines_from_text: array lengths do not match")
    cap = record_lines_bound(R, S, int(po[-1]), sum(int(o[-1]) for o in offs))
    op = (C.c_void_p * max(S, 1))(*[o.ctypes.data for o in offs])
    tp = (C.c_void_p * max(S, 1))(*[b.ctypes.data if len(b) else None for b in data])
    off = np.zeros(R + 1, np.uint64)
    out = np.zeros(max(cap, 1), np.uint8)
    rc = lib.pg_record_lines_from_text(device, R, S, op, tp, po.ctypes.data, pb.ctypes.data if len(pb) else None, off.ctypes.data, out.ctypes.data, cap)
    if rc:
        raise _error(rc, None)
    return off, out[:int(off[-1])].tobytes()


def record_lines_from_text_slotted(texts, prefix, slot=None, uk=None, device: int = 0):
    """pg_record_lines_from_text_slotted: record_lines_from_text over a slotted prefix — the digits of uk[r] in front of byte
    slot[r] of record r's prefix — through the slotted kernels of pg_record_lines.hip.  slot=None: a plain prefix, the bytes of
    record_lines_from_text through those kernels."""
    lib = _lib.load_hip()
    po, pb = np.ascontiguousarray(prefix[0], np.uint64), _as_bytes(prefix[1])
    R, S = len(po) - 1, len(texts)
    offs = [np.ascontiguousarray(t[0], np.uint64) for t in texts]
    data = [_as_bytes(t[1]) for t in texts]
    if R < 0 or any(len(o) != R + 1 for o in offs) or any(int(o[-1]) > len(b) for o, b in zip(offs + [po], data + [pb])):
        raise ValueError("record_lines_from_text_slotted: array lengths do not match")
    ss = uu = None
    if slot is not None:
        if uk is None:
            raise ValueError("record_lines_from_text_slotted: slots without UK values")
        ss, uu = np.ascontiguousarray(slot, np.uint32), np.ascontiguousarray(uk, np.uint16)
        if len(ss) != R or len(uu) != R:
            raise ValueError("record_lines_from_text_slotted: array lengths do not match")
        ss, uu = np.concatenate([ss, np.zeros(1, np.uint32)]), np.concatenate([uu, np.zeros(1, np.uint16)])   # (never empty)
    bound = record_lines_bound if ss is None else record_lines_bound_slotted
    cap = bound(R, S, int(po[-1]), sum(int(o[-1]) for o in offs))
    op = (C.c_void_p * max(S, 1))(*[o.ctypes.data for o in offs])
    tp = (C.c_void_p * max(S, 1))(*[b.ctypes.data if len(b) else None for b in data])
    off = np.zeros(R + 1, np.uint64)
    out = np.zeros(max(cap, 1), np.uint8)
    rc = lib.pg_record_lines_from_text_slotted(device, R, S, op, tp, po.ctypes.data, pb.ctypes.data if len(pb) else None,
                                               None if ss is None else ss.ctypes.data, None if uu is None else uu.ctypes.data, off.ctypes.data,
                                               out.ctypes.data, cap)
    if rc:
        raise _error(rc, None)
    return off, out[:int(off[-1])].tobytes()


# ---------------------------------------------------------------------------------------------------------------
#  The phasing column of a run_phasing job (pg_job_record_phase, pg_job_phased_text, pg_job_phased_lines and the unit entry
#  points)
# ---------------------------------------------------------------------------------------------------------------
PHASE_DTYPE = np.dtype([("allele_1", "<u2"), ("allele_2", "<u2")])
PG_PHASE_UNDEFINED = 0xFFFF   # the haplotype carries an allele of undefined sequence: printed `.`


def phase_text_bound(n_records: int) -> int:
    """pg_phase_text_bound: 13 bytes a record (255|255:65535)."""
    return int(_lib.load_hip().pg_phase_text_bound(int(n_records)))


def form_record_phase(job) -> None:
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_record_phase(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def fetch_record_phase(job, contig: int) -> np.ndarray:
    R = _n_records(job)[contig]
    out = np.zeros(max(R, 1), PHASE_DTYPE)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_phase(job.h, contig, out.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return out[:R]


def fetch_record_phase_all(job) -> List[np.ndarray]:
    Rs = _n_records(job)
    outs = [np.zeros(max(R, 1), PHASE_DTYPE) for R in Rs]
    arr = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_record_phase_all(job.h, arr, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return [o[:R] for o, R in zip(outs, Rs)]


def job_record_phase(job, contig: Optional[int] = None):
    """Job.record_phase(): forms the record phase of every chain that has a plan, fetches all of them (or chain `contig`'s)."""
    form_record_phase(job)
    if contig is not None:
        return fetch_record_phase(job, contig)
    return fetch_record_phase_all(job)


def form_phased_text(job, ignore_imputed: bool = False) -> None:
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_phased_text(job.h, 1 if ignore_imputed else 0, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def phased_text_first(job):
    """pg_job_phased_text_first: (record_first, text_first), each [n_chains + 1]."""
    rf, tf = np.zeros(job.n_chains + 1, np.uint64), np.zeros(job.n_chains + 1, np.uint64)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_phased_text_first(job.h, rf.ctypes.data, tf.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return rf, tf


def fetch_phased_text(job, contig: int):
    """pg_job_fetch_phased_text: (off [R + 1], bytes) of chain `contig`; record r's text is bytes[off[r]:off[r + 1]]."""
    rf, tf = phased_text_first(job)
    n = int(tf[contig + 1] - tf[contig])
    off = np.zeros(int(rf[contig + 1] - rf[contig]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_phased_text(job.h, contig, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes()


def fetch_phased_text_packed(job):
    """pg_job_fetch_phased_text_packed: (off [R_total + 1] absolute in the packed text, bytes, record_first, text_first)."""
    rf, tf = phased_text_first(job)
    n = int(tf[-1])
    off = np.zeros(int(rf[-1]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_phased_text_packed(job.h, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes(), rf, tf


def job_phased_text(job, contig: Optional[int] = None, ignore_imputed: bool = False):
    """Job.phased_text(): forms the text of every chain that has a plan; (off, bytes) of chain `contig`, or of every chain."""
    form_phased_text(job, ignore_imputed)
    if contig is not None:
        return fetch_phased_text(job, contig)
    return [fetch_phased_text(job, c) for c in range(job.n_chains)]


def job_phased_line_prefix(job, contig: int, off, data) -> None:
    """pg_job_phased_line_prefix: the fixed columns (CHROM .. INFO, GT:KC) of index contig `contig` for the phased lines."""
    oo, bb, _ = _prefix_arrays(job, "phased_line_prefix", contig, off, data, None)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_phased_line_prefix(job.h, contig, oo.ctypes.data if len(oo) else None, bb.ctypes.data if len(bb) else None, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def form_phased_lines(job) -> None:
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_phased_lines(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def phased_lines_first(job):
    """pg_job_phased_lines_first: (line_first, byte_first), each [n_index_contigs + 1]."""
    n = C.c_uint64(0)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_phased_lines_first(job.h, C.byref(n), None, None, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    lf, bf = np.zeros(n.value + 1, np.uint64), np.zeros(n.value + 1, np.uint64)
    rc = job._lib.pg_job_phased_lines_first(job.h, C.byref(n), lf.ctypes.data, bf.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return lf, bf


def fetch_phased_lines(job, contig: int):
    """pg_job_fetch_phased_lines: (off [R + 1], bytes) of index contig `contig`; line r is bytes[off[r]:off[r + 1]]."""
    lf, bf = phased_lines_first(job)
    n = int(bf[contig + 1] - bf[contig])
    off = np.zeros(int(lf[contig + 1] - lf[contig]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_phased_lines(job.h, contig, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes()


def fetch_phased_lines_packed(job):
    """pg_job_fetch_phased_lines_packed: (off [n_lines + 1] absolute, bytes, line_first, byte_first) from ONE copy."""
    lf, bf = phased_lines_first(job)
    n = int(bf[-1])
    off = np.zeros(int(lf[-1]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_phased_lines_packed(job.h, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes(), lf, bf


def job_phased_lines(job, contig: Optional[int] = None):
    """Job.phased_lines(): forms the lines from the phased text as it is; (off, bytes) of index contig `contig`, or of all."""
    form_phased_lines(job)
    if contig is not None:
        return fetch_phased_lines(job, contig)
    return [fetch_phased_lines(job, k) for k in range(len(phased_lines_first(job)[0]) - 1)]


def record_phase_from_haplotypes(plan: RecordPlan, hap1, hap2, keyed, device: int = 0) -> np.ndarray:
    """pg_record_phase_from_haplotypes: one PHASE_DTYPE record per record of the plan from the haplotypes' allele ids
    (hap1, hap2 [V]) and keyed [V] — whether the bubble's result holds likelihoods — through the job's kernel."""
    lib = _lib.load_hip()
    pad = lambda a, dt: np.ascontiguousarray(a, dt) if len(a) else np.zeros(1, dt)
    V = plan.n_variants
    if len(hap1) != V or len(hap2) != V or len(keyed) != V:
        raise ValueError("record_phase_from_haplotypes: array lengths do not match the plan")
    h1, h2, kd = pad(hap1, np.uint16), pad(hap2, np.uint16), pad(keyed, np.uint8)
    out = np.zeros(max(plan.n_records, 1), PHASE_DTYPE)
    c = plan.as_c()
    rc = lib.pg_record_phase_from_haplotypes(device, C.addressof(c), h1.ctypes.data, h2.ctypes.data, kd.ctypes.data, out.ctypes.data)
    if rc:
        raise _error(rc, None)
    return out[:plan.n_records]


def phase_text_from_fields(phase, kc, no_call=None, device: int = 0):
    """pg_phase_text_from_fields: (off [R + 1], bytes) — the text of R records from their phase (PHASE_DTYPE), kc [R] and
    no_call [R] (or None), through the job's kernels."""
    lib = _lib.load_hip()
    pp, kk = np.ascontiguousarray(phase, PHASE_DTYPE), np.ascontiguousarray(kc, np.uint16)
    nc = None if no_call is None else np.ascontiguousarray(no_call, np.uint8)
    R = len(pp)
    if len(kk) != R or (nc is not None and len(nc) != R):
        raise ValueError("phase_text_from_fields: array lengths do not match")
    cap = phase_text_bound(R)
    off = np.zeros(R + 1, np.uint64)
    text = np.zeros(max(cap, 1), np.uint8)
    rc = lib.pg_phase_text_from_fields(device, R, pp.ctypes.data if R else None, kk.ctypes.data if R else None, None if nc is None or not R else nc.ctypes.data,
                                       off.ctypes.data, text.ctypes.data, cap)
    if rc:
        raise _error(rc, None)
    return off, text[:int(off[-1])].tobytes()


# ---------------------------------------------------------------------------------------------------------------
#  The sample columns of the sampled-panel VCF (pg_job_panel_text, pg_job_panel_lines and the unit entry point;
#  DESIGN.md 4e-10).  No run is needed: the text is formed from the panel the job holds.
# ---------------------------------------------------------------------------------------------------------------
PG_PANEL_MAX_PATHS = 64   # the device's limit: above it PG_ERR_UNSUPPORTED and the host route


def panel_text_bound(n_records: int, n_paths: int) -> int:
    """pg_panel_text_bound: R (4 P - 1) for P >= 1 (a cell is at most `255`, a tab in front of every cell but the first)."""
    return int(_lib.load_hip().pg_panel_text_bound(int(n_records), int(n_paths)))


def form_panel_text(job) -> None:
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_panel_text(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def panel_text_first(job):
    """pg_job_panel_text_first: (record_first, text_first), each [n_chains + 1]."""
    rf, tf = np.zeros(job.n_chains + 1, np.uint64), np.zeros(job.n_chains + 1, np.uint64)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_panel_text_first(job.h, rf.ctypes.data, tf.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return rf, tf


def fetch_panel_text(job, contig: int):
    """pg_job_fetch_panel_text: (off [R + 1], bytes) of chain `contig`; record r's text is bytes[off[r]:off[r + 1]]."""
    rf, tf = panel_text_first(job)
    n = int(tf[contig + 1] - tf[contig])
    off = np.zeros(int(rf[contig + 1] - rf[contig]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_panel_text(job.h, contig, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes()


def fetch_panel_text_packed(job):
    """pg_job_fetch_panel_text_packed: (off [R_total + 1] absolute in the packed text, bytes, record_first, text_first)."""
    rf, tf = panel_text_first(job)
    n = int(tf[-1])
    off = np.zeros(int(rf[-1]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_panel_text_packed(job.h, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes(), rf, tf


def fetch_panel_uk_packed(job) -> np.ndarray:
    """pg_job_fetch_panel_uk_packed: the UK of every record's line — the panel's own count of its bubble — all chains' from ONE copy."""
    rf, _ = panel_text_first(job)
    uk = np.zeros(max(int(rf[-1]), 1), np.uint16)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_panel_uk_packed(job.h, uk.ctypes.data, int(rf[-1]), err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return uk[:int(rf[-1])]


def job_panel_text(job, contig: Optional[int] = None):
    """Job.panel_text(): forms the text of every chain that has a plan; (off, bytes) of chain `contig`, or of every chain."""
    form_panel_text(job)
    if contig is not None:
        return fetch_panel_text(job, contig)
    return [fetch_panel_text(job, c) for c in range(job.n_chains)]


def job_panel_line_prefix(job, contig: int, off, data, slot=None) -> None:
    """pg_job_panel_line_prefix[_slotted]: the fixed columns (CHROM .. INFO, GT) of index contig `contig` for the panel lines;
    with slot [R], the digits of the panel's own UK go in front of byte slot[r] of record r's."""
    oo, bb, ss = _prefix_arrays(job, "panel_line_prefix", contig, off, data, slot)
    err = C.create_string_buffer(_ERRLEN)
    po, pb = oo.ctypes.data if len(oo) else None, bb.ctypes.data if len(bb) else None
    if ss is None:
        rc = job._lib.pg_job_panel_line_prefix(job.h, contig, po, pb, err, _ERRLEN)
    else:
        rc = job._lib.pg_job_panel_line_prefix_slotted(job.h, contig, po, pb, ss.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def job_panel_line_prefix_strided(job, contig: int, n_contigs: int, off, data, slot=None) -> None:
    """pg_job_panel_line_prefix_strided: ONE prefix for every index contig ix with ix % n_contigs == contig."""
    oo, bb, ss = _prefix_arrays(job, "panel_line_prefix_strided", contig, off, data, slot)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_panel_line_prefix_strided(job.h, contig, n_contigs, oo.ctypes.data if len(oo) else None, bb.ctypes.data if len(bb) else None,
                                                   None if ss is None else ss.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def form_panel_lines(job) -> None:
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_panel_lines(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def panel_lines_first(job):
    """pg_job_panel_lines_first: (line_first, byte_first), each [n_index_contigs + 1]."""
    n = C.c_uint64(0)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_panel_lines_first(job.h, C.byref(n), None, None, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    lf, bf = np.zeros(n.value + 1, np.uint64), np.zeros(n.value + 1, np.uint64)
    rc = job._lib.pg_job_panel_lines_first(job.h, C.byref(n), lf.ctypes.data, bf.ctypes.data, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return lf, bf


def fetch_panel_lines(job, contig: int):
    """pg_job_fetch_panel_lines: (off [R + 1], bytes) of index contig `contig`; line r is bytes[off[r]:off[r + 1]]."""
    lf, bf = panel_lines_first(job)
    n = int(bf[contig + 1] - bf[contig])
    off = np.zeros(int(lf[contig + 1] - lf[contig]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_panel_lines(job.h, contig, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes()


def fetch_panel_lines_packed(job):
    """pg_job_fetch_panel_lines_packed: (off [n_lines + 1] absolute, bytes, line_first, byte_first) from ONE copy."""
    lf, bf = panel_lines_first(job)
    n = int(bf[-1])
    off = np.zeros(int(lf[-1]) + 1, np.uint64)
    text = np.zeros(max(n, 1), np.uint8)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_fetch_panel_lines_packed(job.h, off.ctypes.data, text.ctypes.data, n, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return off, text[:n].tobytes(), lf, bf


def job_panel_lines(job, contig: Optional[int] = None):
    """Job.panel_lines(): forms the lines from the panel text as it is; (off, bytes) of index contig `contig`, or of all."""
    form_panel_lines(job)
    if contig is not None:
        return fetch_panel_lines(job, contig)
    return [fetch_panel_lines(job, k) for k in range(len(panel_lines_first(job)[0]) - 1)]


def panel_text_from_paths(plan: RecordPlan, n_paths: int, path_allele, device: int = 0):
    """pg_panel_text_from_paths: (off [R + 1], bytes) — the text of the plan's records from path_allele [V x n_paths] (the
    allele id of every path at every bubble), through the job's kernels."""
    lib = _lib.load_hip()
    pa = np.ascontiguousarray(path_allele, np.uint16).reshape(-1)
    if len(pa) != plan.n_variants * int(n_paths):
        raise ValueError("panel_text_from_paths: path_allele does not hold n_variants x n_paths ids")
    if len(pa) == 0:
        pa = np.zeros(1, np.uint16)
    R = plan.n_records
    cap = panel_text_bound(R, n_paths)
    off = np.zeros(R + 1, np.uint64)
    text = np.zeros(max(cap, 1), np.uint8)
    c = plan.as_c()
    rc = lib.pg_panel_text_from_paths(device, C.addressof(c), int(n_paths), pa.ctypes.data, off.ctypes.data, text.ctypes.data, cap)
    if rc:
        raise _error(rc, None)
    return off, text[:int(off[-1])].tobytes()


# ---------------------------------------------------------------------------------------------------------------
#  Path subsets combined on the device (pg_job_combine_plan, pg_job_combine, pg_job_combined_calls, pg_combine_bins,
#  pg_calls_from_combined)
# ---------------------------------------------------------------------------------------------------------------
COMBINED_DTYPE = np.dtype([("m", "<u8"), ("e", "<i4"), ("flags", "<u4")])
PG_COMBINED_PRESENT = 1   # the key exists in the combined map
PG_COMBINED_DEFERRED = 2  # present, not formed on the device: add this key on the host from the chains' bins


def combined_to_longdouble(bins) -> np.ndarray:
    """ldexpl((long double)m, e) of every bin, which is exact (0 for an absent or deferred bin: ask `flags`)."""
    b = np.asarray(bins)
    return np.ldexp(b["m"].astype(np.longdouble), b["e"].astype(np.int64))


def job_combine_plan(job, groups) -> None:
    """pg_job_combine_plan: groups = the chains of every group, in combine order."""
    groups = [[int(c) for c in g] for g in groups]
    off = np.zeros(len(groups) + 1, np.uint32)
    if groups:
        off[1:] = np.cumsum([len(g) for g in groups])
    flat = np.array([c for g in groups for c in g] or [0], np.uint32)
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_combine_plan(job.h, len(groups), off.ctypes.data_as(_lib.u32p), flat.ctypes.data_as(_lib.u32p), err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    job._combine_groups = groups


def job_combine(job) -> None:
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_combine(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)


def _group_batch(job, group: int):
    groups = getattr(job, "_combine_groups", None)
    if groups is None or not 0 <= group < len(groups):
        from .hmm import PanGenieError
        raise PanGenieError(_lib.PG_ERR_INVALID, f"group {group}: the job has no such group")
    return job.batches[groups[group][0]]


def fetch_combined(job, group: Optional[int] = None):
    """pg_job_fetch_combined[_all]: the combined bins (COMBINED_DTYPE) of `group`, or of every group."""
    err = C.create_string_buffer(_ERRLEN)
    if group is not None:
        n = int(_group_batch(job, group).geno_off[-1])
        out = np.zeros(max(n, 1), COMBINED_DTYPE)
        rc = job._lib.pg_job_fetch_combined(job.h, group, out.ctypes.data, err, _ERRLEN)
        if rc:
            raise _error(rc, err)
        return out[:n]
    ns = [int(_group_batch(job, g).geno_off[-1]) for g in range(len(getattr(job, "_combine_groups", [])))]
    outs = [np.zeros(max(n, 1), COMBINED_DTYPE) for n in ns]
    arr = (C.c_void_p * max(len(outs), 1))(*[o.ctypes.data for o in outs])
    rc = job._lib.pg_job_fetch_combined_all(job.h, arr, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return [o[:n] for o, n in zip(outs, ns)]


def job_combined_calls(job, group: Optional[int] = None):
    """Job.combined_calls(): forms the calls of every group from its combined bins, fetches all of them (or `group`'s)."""
    err = C.create_string_buffer(_ERRLEN)
    rc = job._lib.pg_job_combined_calls(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    if group is not None:
        V = _group_batch(job, group).n_variants
        out = np.zeros(max(V, 1), CALL_DTYPE)
        rc = job._lib.pg_job_fetch_combined_calls(job.h, group, out.ctypes.data, err, _ERRLEN)
        if rc:
            raise _error(rc, err)
        return out[:V]
    Vs = [_group_batch(job, g).n_variants for g in range(len(getattr(job, "_combine_groups", [])))]
    outs = [np.zeros(max(V, 1), CALL_DTYPE) for V in Vs]
    arr = (C.c_void_p * max(len(outs), 1))(*[o.ctypes.data for o in outs])
    rc = job._lib.pg_job_fetch_combined_calls_all(job.h, arr, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return [o[:V] for o, V in zip(outs, Vs)]


def combine_bins(allele_off, kept, allele_present, lik, lik_exp, device: int = 0) -> np.ndarray:
    """pg_combine_bins: the combined bins (COMBINED_DTYPE) of S chains over one layout — kept[s] [V], allele_present[s]
    [sumA], lik[s] / lik_exp[s] [sum A (A + 1) / 2] of chain s — added up in the order given."""
    lib = _lib.load_hip()
    aoff = np.ascontiguousarray(allele_off, np.uint32)
    V, S = len(aoff) - 1, len(kept)
    A = np.diff(aoff.astype(np.int64))
    n_lik = int((A * (A + 1) // 2).sum())
    if S == 0 or not (len(allele_present) == len(lik) == len(lik_exp) == S):
        raise ValueError("combine_bins: one kept / allele_present / lik / lik_exp per chain, at least one chain")
    pad = lambda a, dt: np.ascontiguousarray(a, dt) if len(a) else np.zeros(1, dt)
    cols = []
    for s in range(S):
        if len(kept[s]) != V or len(allele_present[s]) != int(aoff[-1]) or len(lik[s]) != n_lik or len(lik_exp[s]) != n_lik:
            raise ValueError(f"combine_bins: the arrays of chain {s} do not match allele_off")
        cols.append((pad(kept[s], np.uint8), pad(allele_present[s], np.uint8), pad(lik[s], np.float64), pad(lik_exp[s], np.int32)))
    ptrs = [(C.c_void_p * S)(*[c[k].ctypes.data for c in cols]) for k in range(4)]
    out = np.zeros(max(n_lik, 1), COMBINED_DTYPE)
    rc = lib.pg_combine_bins(device, V, aoff.ctypes.data_as(_lib.u32p), S, ptrs[0], ptrs[1], ptrs[2], ptrs[3], out.ctypes.data)
    if rc:
        raise _error(rc, None)
    return out[:n_lik]


def calls_from_combined(allele_off, allele_id, bins, device: int = 0) -> np.ndarray:
    """pg_calls_from_combined: the calls (CALL_DTYPE) of V variants from their combined bins (COMBINED_DTYPE)."""
    lib = _lib.load_hip()
    aoff = np.ascontiguousarray(allele_off, np.uint32)
    V = len(aoff) - 1
    A = np.diff(aoff.astype(np.int64))
    b = np.ascontiguousarray(bins, COMBINED_DTYPE)
    if len(allele_id) != int(aoff[-1]) or len(b) != int((A * (A + 1) // 2).sum()):
        raise ValueError("calls_from_combined: array lengths do not match allele_off")
    aid = np.ascontiguousarray(allele_id, np.uint16) if len(allele_id) else np.zeros(1, np.uint16)
    if len(b) == 0:
        b = np.zeros(1, COMBINED_DTYPE)
    out = np.zeros(max(V, 1), CALL_DTYPE)
    rc = lib.pg_calls_from_combined(device, V, aoff.ctypes.data_as(_lib.u32p), aid.ctypes.data_as(_lib.u16p), b.ctypes.data, out.ctypes.data)
    if rc:
        raise _error(rc, None)
    return out[:V]


# ---------------------------------------------------------------------------------------------------------------
#  GT, GQ and GL per VCF record of the combined groups (pg_job_combined_record_calls, pg_job_combined_record_gl,
#  pg_record_calls_from_combined, pg_record_gl_from_combined)
# ---------------------------------------------------------------------------------------------------------------
def _group_plans(job) -> list:
    """the record plan of every group: that of its first chain's index contig, or None"""
    plans, nc = getattr(job, "_record_plans", {}), len(job.index)
    return [plans.get(g[0] % nc) for g in getattr(job, "_combine_groups", [])]


def _combined_records(job, group: Optional[int], gl: bool):
    lib, err = job._lib, C.create_string_buffer(_ERRLEN)
    form, fetch, fetch_all = ((lib.pg_job_combined_record_gl, lib.pg_job_fetch_combined_record_gl, lib.pg_job_fetch_combined_record_gl_all) if gl else
                              (lib.pg_job_combined_record_calls, lib.pg_job_fetch_combined_record_calls, lib.pg_job_fetch_combined_record_calls_all))
    rc = form(job.h, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    dtype = GL_DTYPE if gl else CALL_DTYPE
    cache = job.__dict__.setdefault("_group_gl_counts", {})   # (pg_record_gl_offsets checks the whole plan: once per plan, not per fetch)

    def count(p):
        if p is None:
            return 0
        if not gl:
            return p.n_records
        if cache.get(id(p), (None, 0))[0] is not p:
            cache[id(p)] = (p, int(record_gl_offsets(p)[-1]))
        return cache[id(p)][1]
    plans = _group_plans(job)
    if group is not None:
        _group_batch(job, group)   # (raises for a group the job does not have)
        n = count(plans[group])
        out = np.zeros(max(n, 1), dtype)
        rc = fetch(job.h, group, out.ctypes.data, err, _ERRLEN)
        if rc:
            raise _error(rc, err)
        return out[:n]
    ns = [count(p) for p in plans]
    outs = [np.zeros(max(n, 1), dtype) for n in ns]
    arr = (C.c_void_p * max(len(outs), 1))(*[o.ctypes.data for o in outs])
    rc = fetch_all(job.h, arr, err, _ERRLEN)
    if rc:
        raise _error(rc, err)
    return [o[:n] for o, n in zip(outs, ns)]


def job_combined_record_calls(job, group: Optional[int] = None):
    """Job.combined_record_calls(): forms GT and GQ per VCF record of every group that has a plan, fetches all of them (or `group`'s)."""
    return _combined_records(job, group, False)


def job_combined_record_gl(job, group: Optional[int] = None):
    """Job.combined_record_gl(): forms the GL values per VCF record of every group that has a plan, fetches all of them (or `group`'s)."""
    return _combined_records(job, group, True)


def _records_from_combined(name: str, allele_off, allele_id, bins, plan: RecordPlan, n_out: int, dtype, device: int) -> np.ndarray:
    lib = _lib.load_hip()
    aoff = np.ascontiguousarray(allele_off, np.uint32)
    V = len(aoff) - 1
    A = np.diff(aoff.astype(np.int64))
    b = np.ascontiguousarray(bins, COMBINED_DTYPE)
    if len(allele_id) != int(aoff[-1]) or len(b) != int((A * (A + 1) // 2).sum()):
        raise ValueError(f"{name}: array lengths do not match allele_off")
    aid = np.ascontiguousarray(allele_id, np.uint16) if len(allele_id) else np.zeros(1, np.uint16)
    if len(b) == 0:
        b = np.zeros(1, COMBINED_DTYPE)
    out = np.zeros(max(n_out, 1), dtype)
    c = plan.as_c()
    rc = getattr(lib, "pg_" + name)(device, V, aoff.ctypes.data_as(_lib.u32p), aid.ctypes.data_as(_lib.u16p), b.ctypes.data, C.addressof(c), out.ctypes.data)
    if rc:
        raise _error(rc, None)
    return out[:n_out]


def record_calls_from_combined(allele_off, allele_id, bins, plan: RecordPlan, device: int = 0) -> np.ndarray:
    """pg_record_calls_from_combined: the calls (CALL_DTYPE) of the plan's records from one contig's combined bins (COMBINED_DTYPE)."""
    return _records_from_combined("record_calls_from_combined", allele_off, allele_id, bins, plan, plan.n_records, CALL_DTYPE, device)


def record_gl_from_combined(allele_off, allele_id, bins, plan: RecordPlan, device: int = 0) -> np.ndarray:
    """pg_record_gl_from_combined: the GL values (GL_DTYPE) of the plan's records from one contig's combined bins; record r's
    values at record_gl_offsets(plan)[r] ..."""
    return _records_from_combined("record_gl_from_combined", allele_off, allele_id, bins, plan, int(record_gl_offsets(plan)[-1]), GL_DTYPE, device)
