"""The C ABI of the records of combined groups without a device (include/pangenie_hmm.h): the symbols resolve,
and the unit entry points check the layout, the plan, every allele id against the plan's maps, the bins and `out` on the host
— PG_ERR_INVALID / PG_ERR_UNSUPPORTED — before any device is asked for; a well-formed call answers PG_ERR_DEVICE where there
is no device (with one, the answer).  Null jobs are invalid."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd import _lib, calls
from pangenie_amd.hmm import PanGenieError

NEW_SYMBOLS = [
    "pg_job_combined_record_calls", "pg_job_combined_record_gl", "pg_job_fetch_combined_record_calls", "pg_job_fetch_combined_record_gl",
    "pg_job_fetch_combined_record_calls_all", "pg_job_fetch_combined_record_gl_all", "pg_job_device_combined_record_calls",
    "pg_job_device_combined_record_gl", "pg_job_combined_record_calls_ms", "pg_job_combined_record_gl_ms",
    "pg_record_calls_from_combined", "pg_record_gl_from_combined",
]
ENTRIES = [calls.record_calls_from_combined, calls.record_gl_from_combined]


def test_the_symbols_resolve_and_are_listed():
    lib = _lib.load_hip()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_ABI_SYMBOLS, name
    header = (Path(__file__).resolve().parent.parent / "include" / "pangenie_hmm.h").read_text()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name


def case():
    """one bubble of three alleles (ids 0, 1, 2) and one of two, two records on the first"""
    aoff = np.array([0, 3, 5], np.uint32)
    ids = np.array([0, 1, 2, 0, 1], np.uint16)
    bins = np.zeros(9, calls.COMBINED_DTYPE)
    bins["flags"] = calls.PG_COMBINED_PRESENT
    bins["m"] = 1 << 63
    bins["e"] = [-64, -65, -66, -67, -66, -65, -64, -66, -65]
    plan = calls.RecordPlan.from_records([[([0, 1, 0], [True, True]), ([0, 1, 2], [True, False, True])], [([0, 1], [True, True])]])
    return aoff, ids, bins, plan


def code_of(fn, *args):
    with pytest.raises(PanGenieError) as e:
        fn(*args)
    return e.value.code


@pytest.mark.parametrize("fn", ENTRIES)
def test_a_well_formed_call_answers_a_device_error_without_a_device(fn):
    aoff, ids, bins, plan = case()
    if _lib.load_hip().pg_hmm_device_count() > 0:
        out = fn(aoff, ids, bins, plan)
        assert len(out) == (plan.n_records if fn is calls.record_calls_from_combined else int(calls.record_gl_offsets(plan)[-1]))
    else:
        assert code_of(fn, aoff, ids, bins, plan) == _lib.PG_ERR_DEVICE


@pytest.mark.parametrize("fn", ENTRIES)
def test_what_is_malformed_is_refused_before_any_device_is_asked_for(fn):
    aoff, ids, bins, plan = case()
    # an allele id outside a map: the plan's maps have three and two entries
    far = ids.copy()
    far[2] = 3
    assert code_of(fn, aoff, far, bins, plan) == _lib.PG_ERR_INVALID
    # a plan for another number of variants
    short = calls.RecordPlan.from_records([[([0, 1, 0], [True, True])]])
    assert code_of(fn, aoff, ids, bins, short) == _lib.PG_ERR_INVALID
    # a map one entry short for the first bubble's ids
    tight = calls.RecordPlan.from_records([[([0, 1], [True, True])], [([0, 1], [True, True])]])
    assert code_of(fn, aoff, ids, bins, tight) == _lib.PG_ERR_INVALID
    # a bin that is no pg_combined_bin: a mantissa that is not normalised, a value on an absent bin, unknown flags, deferred without present
    for field, at, value in (("m", 1, 5), ("flags", 2, 0), ("flags", 3, 4), ("flags", 4, calls.PG_COMBINED_DEFERRED)):
        bad = bins.copy()
        bad[field][at] = value
        assert code_of(fn, aoff, ids, bad, plan) == _lib.PG_ERR_INVALID, (field, at, value)
    # a layout that is none: a variant without alleles
    assert code_of(fn, np.array([0, 3, 3], np.uint32), ids[:3], bins[:6], plan) == _lib.PG_ERR_INVALID


def test_a_malformed_plan_and_null_arguments_give_the_documented_codes():
    lib = _lib.load_hip()
    aoff, ids, bins, plan = case()
    out = np.zeros(64, np.uint64)
    a, i = aoff.ctypes.data_as(_lib.u32p), ids.ctypes.data_as(_lib.u16p)
    for fn in (lib.pg_record_calls_from_combined, lib.pg_record_gl_from_combined):
        c = plan.as_c()
        assert fn(0, 2, a, i, bins.ctypes.data, None, out.ctypes.data) == _lib.PG_ERR_INVALID            # no plan
        assert fn(0, 2, None, i, bins.ctypes.data, C.addressof(c), out.ctypes.data) == _lib.PG_ERR_INVALID   # no layout
        assert fn(0, 2, a, None, bins.ctypes.data, C.addressof(c), out.ctypes.data) == _lib.PG_ERR_INVALID   # no ids
        assert fn(0, 2, a, i, None, C.addressof(c), out.ctypes.data) == _lib.PG_ERR_INVALID                  # no bins
        assert fn(0, 2, a, i, bins.ctypes.data, C.addressof(c), None) == _lib.PG_ERR_INVALID                 # no room for the answer
    # vcf_index that is not the running count of defined alleles; a map entry that is no allele of its record; more than 256 alleles
    vcf = plan.vcf_index.copy()
    vcf[1] = 7
    broken = calls.RecordPlan(plan.rec_off, plan.map_off, plan.map, plan.n_alleles, plan.vcf_off, vcf)
    mp = plan.map.copy()
    mp[1] = 2
    stray = calls.RecordPlan(plan.rec_off, plan.map_off, mp, plan.n_alleles, plan.vcf_off, plan.vcf_index)
    for fn in ENTRIES:
        assert code_of(fn, aoff, ids, bins, broken) == _lib.PG_ERR_INVALID
        assert code_of(fn, aoff, ids, bins, stray) == _lib.PG_ERR_INVALID
    wide = calls.RecordPlan.from_records([[([0, 1, 0], [True] * 300)], [([0, 1], [True, True])]])
    for fn in ENTRIES:
        assert code_of(fn, aoff, ids, bins, wide) == _lib.PG_ERR_UNSUPPORTED
    # no variants: the plan is looked at, nothing else
    empty = calls.RecordPlan.from_records([])
    c = empty.as_c()
    assert lib.pg_record_calls_from_combined(0, 0, None, None, None, C.addressof(c), None) == _lib.PG_OK
    assert lib.pg_record_gl_from_combined(0, 0, None, None, None, None, None) == _lib.PG_ERR_INVALID


def test_null_jobs_are_invalid():
    lib = _lib.load_hip()
    err = C.create_string_buffer(64)
    assert lib.pg_job_combined_record_calls(None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_combined_record_gl(None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_combined_record_calls(None, 0, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_combined_record_gl(None, 0, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_combined_record_calls_all(None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_combined_record_gl_all(None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_device_combined_record_calls(None, 0, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_job_device_combined_record_gl(None, 0, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_job_combined_record_calls_ms(None) == 0.0 and lib.pg_job_combined_record_gl_ms(None) == 0.0
