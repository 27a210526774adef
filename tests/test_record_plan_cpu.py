"""The checks of a record plan (include/pangenie_hmm.h: pg_record_plan) through the unit entry point, on the CPU: the plan
is checked on the host before anything reaches a device, so every malformed plan answers PG_ERR_INVALID whether a device
exists or not; a valid plan then answers PG_ERR_DEVICE without one (no host fallback) and the calls with one."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib, calls
from pangenie_amd.hmm import PanGenieError

# two bubbles: three alleles (ids 0, 1, 2) merged from two records, and a biallelic one with one record
AOFF = np.array([0, 3, 5], np.uint32)
AID = np.array([0, 1, 2, 0, 1], np.uint16)
KEPT = np.array([1, 1], np.uint8)
PRES = np.ones(5, np.uint8)
LIK = np.array([0.5, 0.25, 0.125, 0.0625, 0.03125, 0.03125, 0.25, 0.5, 0.25])
EXP = np.zeros(9, np.int32)


def good():
    return dict(rec_off=[0, 2, 3], map_off=[0, 3, 6, 8], map=[0, 1, 0, 0, 0, 1, 0, 1], n_alleles=[2, 2, 2], vcf_off=[0, 2, 4, 6],
                vcf_index=[0, 1, 0, 0xFFFF, 0, 1])


def code_of(**changes):
    p = good()
    p.update(changes)
    try:
        calls.record_calls_from_bins(AOFF, AID, KEPT, PRES, LIK, EXP, calls.RecordPlan(**p))
    except PanGenieError as e:
        return e.code
    return _lib.PG_OK


BAD = {
    "rec_off shrinks": dict(rec_off=[0, 3, 2]),
    "a bubble without a record": dict(rec_off=[0, 0, 3]),
    "rec_off does not start at 0": dict(rec_off=[1, 2, 3]),
    "rec_off ends beyond the records": dict(rec_off=[0, 2, 4]),
    "map_off shrinks": dict(map_off=[0, 3, 2, 8]),
    "vcf_off does not follow n_alleles": dict(vcf_off=[0, 2, 5, 6]),
    "a record without alleles": dict(n_alleles=[2, 0, 2], vcf_off=[0, 2, 2, 4]),
    "a map entry that is no allele of the record": dict(map=[0, 1, 2, 0, 0, 1, 0, 1]),
    "vcf_index is not the running count": dict(vcf_index=[0, 1, 0, 0xFFFF, 0, 2]),
    "vcf_index counts an undefined allele": dict(n_alleles=[3, 2, 2], vcf_off=[0, 3, 5, 7], vcf_index=[0, 0xFFFF, 2, 0, 1, 0, 1]),
    "allele 0 is undefined": dict(vcf_index=[0xFFFF, 0, 0, 0xFFFF, 0, 1]),
    "an allele id outside a record's map": dict(map_off=[0, 3, 5, 7], map=[0, 1, 0, 0, 0, 0, 1]),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_a_malformed_plan_is_refused_before_any_device_is_asked_for(what):
    assert code_of(**BAD[what]) == _lib.PG_ERR_INVALID


def test_the_number_of_variants_must_be_the_contigs_and_a_record_has_at_most_256_alleles():
    lib = _lib.load_hip()
    plan = calls.RecordPlan(**good()).as_c()
    plan.n_variants = 3
    out = np.zeros(3, calls.CALL_DTYPE)
    p = lambda a, t: a.ctypes.data_as(t)
    args = (0, 2, p(AOFF, _lib.u32p), p(AID, _lib.u16p), p(KEPT, _lib.u8p), p(PRES, _lib.u8p), p(LIK, _lib.f64p), p(EXP, _lib.i32p))
    assert lib.pg_record_calls_from_bins(*args, C.addressof(plan), out.ctypes.data) == _lib.PG_ERR_INVALID
    assert lib.pg_record_calls_from_bins(*args, None, out.ctypes.data) == _lib.PG_ERR_INVALID
    big = dict(n_alleles=[2, 2, 257], vcf_off=[0, 2, 4, 261], vcf_index=[0, 1, 0, 0xFFFF] + list(range(257)))
    assert code_of(**big) == _lib.PG_ERR_UNSUPPORTED


def test_a_valid_plan_without_a_device_is_a_device_error_not_a_host_answer():
    lib = _lib.load_hip()
    if lib.pg_hmm_device_count() > 0:
        rec = calls.record_calls_from_bins(AOFF, AID, KEPT, PRES, LIK, EXP, calls.RecordPlan(**good()))
        # record 0 (own 0, 1, 0): F(0,0) = 0.5 + 0.125 + 0.03125, F(0,1) = 0.25 + 0.03125, F(1,1) = 0.0625
        assert [(int(r["allele_1"]), int(r["allele_2"]), int(r["flags"])) for r in rec] == [(0, 0, 0), (0, 0, 0), (0, 1, 0)]
    else:
        assert code_of() == _lib.PG_ERR_DEVICE
    # a null job is refused before any device is asked for
    err = C.create_string_buffer(64)
    assert lib.pg_job_record_plan(None, 0, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_calls(None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_record_calls(None, 0, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_record_calls_all(None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_device_record_calls(None, 0, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_calls_ms(None) == 0.0
