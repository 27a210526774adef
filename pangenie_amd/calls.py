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

