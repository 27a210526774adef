"""The C ABI of the record text without a device (include/pangenie_hmm.h): the symbols resolve, the bound is
19 R + 11 N, pg_record_text_from_fields refuses null arrays, offsets that do not start at 0 or shrink, a buffer below the bound
and calls the bound does not cover — PG_ERR_INVALID, before any device is asked for — and a well-formed call answers
PG_ERR_DEVICE where there is no device (with one, the text).  Null jobs are invalid."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd import _lib, calls
from pangenie_amd.hmm import PanGenieError

NEW_SYMBOLS = [
    "pg_record_text_bound", "pg_job_record_text", "pg_job_record_text_first", "pg_job_fetch_record_text", "pg_job_fetch_record_text_packed",
    "pg_job_device_record_text", "pg_job_record_text_ms", "pg_job_record_text_emit_ms", "pg_record_text_from_fields",
]


def test_the_symbols_resolve_and_are_listed():
    lib = _lib.load_hip()
    header = (Path(__file__).resolve().parent.parent / "include" / "pangenie_hmm.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_ABI_SYMBOLS, name
        assert name + "(" in header, name


def test_the_bound_needs_no_device():
    assert calls.record_text_bound(0, 0) == 0
    assert calls.record_text_bound(1, 3) == 19 + 33
    assert calls.record_text_bound(2_055_680, 5_022_528) == 19 * 2_055_680 + 11 * 5_022_528
    assert calls.record_text_bound(1 << 33, 1 << 34) == 19 * (1 << 33) + 11 * (1 << 34)   # 64 bits


def case():
    """two records of three values, one of six"""
    cl = np.zeros(3, calls.CALL_DTYPE)
    cl["allele_1"], cl["allele_2"], cl["gq"] = [0, 1, 0], [1, 1, 2], [37, 10000, 5]
    gl_off = np.array([0, 3, 6, 12], np.uint64)
    gl = np.zeros(12, calls.GL_DTYPE)
    gl["mant"], gl["exp10"] = -1234, -1
    kc = np.array([17, 0, 65535], np.uint16)
    return cl, gl_off, gl, kc


def raw(cl, gl_off, gl, kc, no_call=None, off="own", text="own", cap=None, n=None):
    lib = _lib.load_hip()
    n = (3 if cl is None else len(cl)) if n is None else n
    bound = calls.record_text_bound(n, 12 if gl is None else len(gl))
    cap = bound if cap is None else cap
    o, t = np.zeros(min(n, 16) + 1, np.uint64), np.zeros(min(max(cap, 1), 1 << 16), np.uint8)   # (a refusal comes before any of it is written)
    p = lambda a: None if a is None else a.ctypes.data
    return lib.pg_record_text_from_fields(0, n, p(cl), p(gl_off), p(gl), p(kc), p(no_call), o.ctypes.data if off == "own" else None,
                                          t.ctypes.data if text == "own" else None, cap)


def test_a_well_formed_call_answers_a_device_error_without_a_device():
    cl, gl_off, gl, kc = case()
    if _lib.load_hip().pg_hmm_device_count() > 0:
        off, text = calls.record_text_from_fields(cl, gl_off, gl, kc)
        assert text[:int(off[1])] == b"0/1:37:-0.1234,-0.1234,-0.1234:17"
    else:
        with pytest.raises(PanGenieError) as e:
            calls.record_text_from_fields(cl, gl_off, gl, kc)
        assert e.value.code == _lib.PG_ERR_DEVICE
        assert raw(cl, gl_off, gl, kc, no_call=np.zeros(3, np.uint8)) == _lib.PG_ERR_DEVICE


def test_what_is_malformed_is_refused_before_any_device_is_asked_for():
    cl, gl_off, gl, kc = case()
    INV = _lib.PG_ERR_INVALID
    assert raw(None, gl_off, gl, kc) == INV and raw(cl, None, gl, kc) == INV and raw(cl, gl_off, None, kc) == INV and raw(cl, gl_off, gl, None) == INV
    assert raw(cl, gl_off, gl, kc, off=None) == INV and raw(cl, gl_off, gl, kc, text=None) == INV
    assert raw(cl, np.array([1, 3, 6, 12], np.uint64), gl, kc) == INV          # does not start at 0
    assert raw(cl, np.array([0, 6, 3, 12], np.uint64), gl, kc) == INV          # does not grow
    assert raw(cl, gl_off, gl, kc, cap=calls.record_text_bound(3, 12) - 1) == INV
    assert raw(cl, gl_off, gl, kc, cap=0) == INV
    for field, value in (("allele_1", 256), ("allele_2", 300), ("gq", 10001)):   # what the bound does not cover
        bad = cl.copy()
        bad[field][1] = value
        assert raw(bad, gl_off, gl, kc) == INV, field
    none = cl.copy()   # ... but a call that prints .:.: may hold anything
    none["allele_1"][1], none["allele_2"][1], none["flags"][1] = 0xFFFF, 0xFFFF, calls.PG_CALL_NONE
    assert raw(none, gl_off, gl, kc) in (_lib.PG_OK, _lib.PG_ERR_DEVICE)
    assert raw(cl, gl_off, gl, kc, n=1 << 31) == INV
    # no records: the offsets alone
    off = np.ones(1, np.uint64)
    assert _lib.load_hip().pg_record_text_from_fields(0, 0, None, np.zeros(1, np.uint64).ctypes.data, None, None, None, off.ctypes.data, None, 0) == _lib.PG_OK
    assert off[0] == 0


def test_null_jobs_are_invalid():
    lib = _lib.load_hip()
    err = C.create_string_buffer(64)
    assert lib.pg_job_record_text(None, 0, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_text(None, 1, None, 0) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_text_first(None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_record_text(None, 0, None, None, 0, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_record_text_packed(None, None, None, 0, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_device_record_text(None, 0, None, None, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_text_ms(None) == 0.0 and lib.pg_job_record_text_emit_ms(None) == 0.0
