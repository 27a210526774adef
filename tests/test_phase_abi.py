"""The C ABI of the phasing column without a device (include/pangenie_hmm.h): the symbols resolve, the bound is
13 R, and the two unit entry points refuse null arrays, a plan whose offsets do not start at 0 or shrink or that is malformed in
any other way, a buffer below the bound, alleles the bound does not cover and a haplotype id outside the map of one of its
bubble's records — PG_ERR_INVALID, before any device is asked for — while a well-formed call answers PG_ERR_DEVICE where there
is no device (with one, the values).  Null jobs are invalid."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd import _lib, calls
from pangenie_amd.hmm import PanGenieError

NEW_SYMBOLS = [
    "pg_job_record_phase", "pg_job_fetch_record_phase", "pg_job_fetch_record_phase_all", "pg_job_device_record_phase", "pg_job_record_phase_ms",
    "pg_job_phased_text", "pg_job_phased_text_first", "pg_job_fetch_phased_text", "pg_job_fetch_phased_text_packed", "pg_job_device_phased_text",
    "pg_job_phased_text_ms", "pg_job_phased_line_prefix", "pg_job_phased_lines", "pg_job_phased_lines_first", "pg_job_fetch_phased_lines",
    "pg_job_fetch_phased_lines_packed", "pg_job_device_phased_lines", "pg_job_phased_lines_ms", "pg_phase_text_bound",
    "pg_record_phase_from_haplotypes", "pg_phase_text_from_fields",
]
INV = _lib.PG_ERR_INVALID


def test_the_symbols_resolve_and_are_listed():
    lib = _lib.load_hip()
    header = (Path(__file__).resolve().parent.parent / "include" / "pangenie_hmm.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_ABI_SYMBOLS, name
        assert name + "(" in header, name
    assert "typedef struct pg_phase { uint16_t allele_1, allele_2; } pg_phase;" in header and "#define PG_PHASE_UNDEFINED 0xFFFFu" in header
    assert calls.PHASE_DTYPE.itemsize == 4 and calls.PG_PHASE_UNDEFINED == 0xFFFF


def test_the_bound_needs_no_device():
    assert calls.phase_text_bound(0) == 0
    assert calls.phase_text_bound(1) == 13 == len("255|255:65535")
    assert calls.phase_text_bound(2_055_680) == 13 * 2_055_680
    assert calls.phase_text_bound(1 << 40) == 13 << 40   # 64 bits


# ---- pg_phase_text_from_fields --------------------------------------------------------------------------------------
def text_case():
    ph = np.zeros(3, calls.PHASE_DTYPE)
    ph["allele_1"], ph["allele_2"] = [0, 1, 0xFFFF], [1, 255, 2]
    return ph, np.array([17, 0, 65535], np.uint16)


def raw_text(ph, kc, no_call=None, off="own", text="own", cap=None, n=None):
    lib = _lib.load_hip()
    n = 3 if n is None else n
    cap = calls.phase_text_bound(n) if cap is None else cap
    o, t = np.zeros(min(n, 16) + 1, np.uint64), np.zeros(min(max(cap, 1), 1 << 16), np.uint8)   # (a refusal comes before any of it is written)
    p = lambda a: None if a is None else a.ctypes.data
    return lib.pg_phase_text_from_fields(0, n, p(ph), p(kc), p(no_call), o.ctypes.data if off == "own" else None, t.ctypes.data if text == "own" else None, cap)


def test_a_well_formed_text_call_answers_a_device_error_without_a_device():
    ph, kc = text_case()
    if _lib.load_hip().pg_hmm_device_count() > 0:
        off, text = calls.phase_text_from_fields(ph, kc)
        assert text == b"0|1:171|255:0.|2:65535" and off.tolist() == [0, 6, 13, 22]
    else:
        with pytest.raises(PanGenieError) as e:
            calls.phase_text_from_fields(ph, kc)
        assert e.value.code == _lib.PG_ERR_DEVICE
        assert raw_text(ph, kc, no_call=np.zeros(3, np.uint8)) == _lib.PG_ERR_DEVICE


def test_a_malformed_text_call_is_refused_before_any_device_is_asked_for():
    ph, kc = text_case()
    assert raw_text(None, kc) == INV and raw_text(ph, None) == INV
    assert raw_text(ph, kc, off=None) == INV and raw_text(ph, kc, text=None) == INV
    assert raw_text(ph, kc, cap=calls.phase_text_bound(3) - 1) == INV and raw_text(ph, kc, cap=0) == INV
    for field, value in (("allele_1", 256), ("allele_2", 0xFFFE)):   # what the bound does not cover
        bad = ph.copy()
        bad[field][1] = value
        assert raw_text(bad, kc) == INV, field
    assert raw_text(ph, kc, n=1 << 31) == INV
    # no records: the offsets alone
    off = np.ones(1, np.uint64)
    assert _lib.load_hip().pg_phase_text_from_fields(0, 0, None, None, None, off.ctypes.data, None, 0) == _lib.PG_OK
    assert off[0] == 0


# ---- pg_record_phase_from_haplotypes --------------------------------------------------------------------------------
def phase_case():
    """two bubbles: one record of three alleles (the last undefined); two records over four bubble alleles"""
    plan = calls.RecordPlan.from_records([[([0, 1, 2], [True, True, False])], [([0, 1, 0, 1], [True, True]), ([0, 0, 1, 2], [True, False, True])]])
    return plan, np.array([2, 3], np.uint16), np.array([1, 0], np.uint16), np.array([1, 0], np.uint8)


def raw_phase(plan, h1, h2, keyed, out="own"):
    lib = _lib.load_hip()
    c = plan.as_c() if plan is not None else None
    o = np.zeros(8, calls.PHASE_DTYPE)
    p = lambda a: None if a is None else a.ctypes.data
    return lib.pg_record_phase_from_haplotypes(0, C.addressof(c) if c is not None else None, p(h1), p(h2), p(keyed), o.ctypes.data if out == "own" else None)


def test_a_well_formed_phase_call_answers_a_device_error_without_a_device():
    plan, h1, h2, keyed = phase_case()
    if _lib.load_hip().pg_hmm_device_count() > 0:
        got = calls.record_phase_from_haplotypes(plan, h1, h2, keyed)
        # bubble 0, keyed: allele 2 is undefined, allele 1 maps onto itself; bubble 1, not keyed: record 1 is all defined (1|0),
        # record 2 has an undefined allele: the defined haplotypes come out as 0
        assert [tuple(int(x) for x in r) for r in got] == [(0xFFFF, 1), (1, 0), (0, 0)]
    else:
        with pytest.raises(PanGenieError) as e:
            calls.record_phase_from_haplotypes(plan, h1, h2, keyed)
        assert e.value.code == _lib.PG_ERR_DEVICE


def test_a_malformed_phase_call_is_refused_before_any_device_is_asked_for():
    plan, h1, h2, keyed = phase_case()
    assert raw_phase(None, h1, h2, keyed) == INV
    assert raw_phase(plan, None, h2, keyed) == INV and raw_phase(plan, h1, None, keyed) == INV and raw_phase(plan, h1, h2, None) == INV
    assert raw_phase(plan, h1, h2, keyed, out=None) == INV
    # a haplotype id outside the map of one of its bubble's records (bubble 0: 3 entries; bubble 1: 4)
    assert raw_phase(plan, np.array([3, 3], np.uint16), h2, keyed) == INV
    assert raw_phase(plan, h1, np.array([1, 4], np.uint16), keyed) == INV
    # offsets that do not start at 0 or shrink, and other malformed plans
    def broken(**kw):
        p = calls.RecordPlan(plan.rec_off.copy(), plan.map_off.copy(), plan.map.copy(), plan.n_alleles.copy(), plan.vcf_off.copy(), plan.vcf_index.copy())
        for name, (at, value) in kw.items():
            getattr(p, name)[at] = value
        return p
    for bad in (broken(rec_off=(0, 1)), broken(map_off=(0, 1)), broken(vcf_off=(0, 1)), broken(rec_off=(1, 0)), broken(map_off=(2, 1)), broken(vcf_off=(2, 1)),
                broken(n_alleles=(0, 4)), broken(map=(2, 3)), broken(vcf_index=(1, 2)), broken(vcf_index=(0, 0xFFFF))):
        assert raw_phase(bad, h1, h2, keyed) == INV
    # a plan without variants: nothing to do, whatever the arrays
    empty = calls.RecordPlan.from_records([])
    assert raw_phase(empty, None, None, None, out=None) == _lib.PG_OK


def test_null_jobs_are_invalid():
    lib = _lib.load_hip()
    err = C.create_string_buffer(64)
    assert lib.pg_job_record_phase(None, err, 64) == INV and lib.pg_job_record_phase(None, None, 0) == INV
    assert lib.pg_job_fetch_record_phase(None, 0, None, err, 64) == INV
    assert lib.pg_job_fetch_record_phase_all(None, None, err, 64) == INV
    assert lib.pg_job_device_record_phase(None, 0, None, None) == INV
    assert lib.pg_job_phased_text(None, 0, err, 64) == INV and lib.pg_job_phased_text(None, 1, None, 0) == INV
    assert lib.pg_job_phased_text_first(None, None, None, err, 64) == INV
    assert lib.pg_job_fetch_phased_text(None, 0, None, None, 0, err, 64) == INV
    assert lib.pg_job_fetch_phased_text_packed(None, None, None, 0, err, 64) == INV
    assert lib.pg_job_device_phased_text(None, 0, None, None, None, None) == INV
    assert lib.pg_job_phased_line_prefix(None, 0, None, None, err, 64) == INV
    assert lib.pg_job_phased_lines(None, err, 64) == INV
    assert lib.pg_job_phased_lines_first(None, None, None, None, err, 64) == INV
    assert lib.pg_job_fetch_phased_lines(None, 0, None, None, 0, err, 64) == INV
    assert lib.pg_job_fetch_phased_lines_packed(None, None, None, 0, err, 64) == INV
    assert lib.pg_job_device_phased_lines(None, 0, None, None, None, None) == INV
    assert lib.pg_job_record_phase_ms(None) == 0.0 and lib.pg_job_phased_text_ms(None) == 0.0 and lib.pg_job_phased_lines_ms(None) == 0.0
