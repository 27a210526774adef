"""The C ABI of the record lines without a device (include/pangenie_hmm.h): the symbols resolve, the bound is
prefix_bytes + text_bytes + R (S + 1), pg_record_lines_from_text refuses null arrays, offsets that do not start at 0 or shrink,
no members, a buffer below the bound and 2^31 records — PG_ERR_INVALID, before any device is asked for — and a well-formed call
answers PG_ERR_DEVICE where there is no device (with one, the lines).  Null jobs are invalid."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd import _lib, calls
from pangenie_amd.hmm import PanGenieError

NEW_SYMBOLS = [
    "pg_record_lines_bound", "pg_job_line_prefix", "pg_job_record_lines", "pg_job_record_lines_first", "pg_job_fetch_record_lines",
    "pg_job_fetch_record_lines_packed", "pg_job_device_record_lines", "pg_job_record_lines_ms", "pg_record_lines_from_text",
]


def test_the_symbols_resolve_and_are_listed():
    lib = _lib.load_hip()
    header = (Path(__file__).resolve().parent.parent / "include" / "pangenie_hmm.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_ABI_SYMBOLS, name
        assert name + "(" in header, name


def test_the_bound_needs_no_device():
    assert calls.record_lines_bound(0, 0, 0, 0) == 0
    assert calls.record_lines_bound(0, 7, 0, 0) == 0
    assert calls.record_lines_bound(1, 1, 0, 0) == 2                  # a tab and a newline
    assert calls.record_lines_bound(3, 2, 10, 12) == 10 + 12 + 3 * 3
    assert calls.record_lines_bound(1 << 31, 512, 1 << 36, 1 << 40) == (1 << 36) + (1 << 40) + (1 << 31) * 513   # 64 bits


def case():
    """three records, two members"""
    prefix = (np.array([0, 2, 2, 5], np.uint64), np.frombuffer(b"abcde", np.uint8))
    texts = [(np.array([0, 1, 3, 6], np.uint64), np.frombuffer(b"ABBCCC", np.uint8)),
             (np.array([0, 3, 5, 6], np.uint64), np.frombuffer(b"xxxyyz", np.uint8))]
    return prefix, texts


def raw(prefix, texts, cap=None, n=3, members=None, off="own", out="own", null_member_off=False, null_member_text=False, null_off_array=False,
        null_text_array=False):
    lib = _lib.load_hip()
    S = len(texts) if members is None else members
    bound = calls.record_lines_bound(3, len(texts), 5, 12)
    cap = bound if cap is None else cap
    op = (C.c_void_p * max(len(texts), 1))(*[None if null_member_off and s == 1 else t[0].ctypes.data for s, t in enumerate(texts)])
    tp = (C.c_void_p * max(len(texts), 1))(*[None if null_member_text and s == 1 else t[1].ctypes.data for s, t in enumerate(texts)])
    o, b = np.zeros(4, np.uint64), np.zeros(max(min(cap, 1 << 16), 1), np.uint8)   # (a refusal comes before any of it is written)
    p = lambda a: None if a is None else a.ctypes.data
    return lib.pg_record_lines_from_text(0, n, S, None if null_off_array else op, None if null_text_array else tp, p(prefix[0]), p(prefix[1]),
                                         o.ctypes.data if off == "own" else None, b.ctypes.data if out == "own" else None, cap)


def test_a_well_formed_call_answers_a_device_error_without_a_device():
    prefix, texts = case()
    if _lib.load_hip().pg_hmm_device_count() > 0:
        off, lines = calls.record_lines_from_text(texts, prefix)
        assert lines == b"ab\tA\txxx\n\tBB\tyy\ncde\tCCC\tz\n" and off.tolist() == [0, 9, 16, 26]
    else:
        with pytest.raises(PanGenieError) as e:
            calls.record_lines_from_text(texts, prefix)
        assert e.value.code == _lib.PG_ERR_DEVICE
        assert raw(prefix, texts) == _lib.PG_ERR_DEVICE


def test_what_is_malformed_is_refused_before_any_device_is_asked_for():
    prefix, texts = case()
    INV = _lib.PG_ERR_INVALID
    # null arrays
    assert raw((None, prefix[1]), texts) == INV and raw((prefix[0], None), texts) == INV
    assert raw(prefix, texts, null_off_array=True) == INV and raw(prefix, texts, null_text_array=True) == INV
    assert raw(prefix, texts, null_member_off=True) == INV and raw(prefix, texts, null_member_text=True) == INV
    assert raw(prefix, texts, off=None) == INV and raw(prefix, texts, out=None) == INV
    # offsets that do not start at 0 or shrink: the prefix's and a member's
    assert raw((np.array([1, 2, 2, 5], np.uint64), prefix[1]), texts) == INV
    assert raw((np.array([0, 3, 2, 5], np.uint64), prefix[1]), texts) == INV
    assert raw(prefix, [texts[0], (np.array([1, 3, 5, 6], np.uint64), texts[1][1])]) == INV
    assert raw(prefix, [(np.array([0, 4, 3, 6], np.uint64), texts[0][1]), texts[1]]) == INV
    # no members, a buffer below the bound, too many records
    assert raw(prefix, texts, members=0) == INV
    assert raw(prefix, texts, cap=calls.record_lines_bound(3, 2, 5, 12) - 1) == INV and raw(prefix, texts, cap=0) == INV
    assert raw(prefix, texts, n=1 << 31) == INV
    # no records: the offsets alone
    off, zero = np.ones(1, np.uint64), np.zeros(1, np.uint64)
    op, tp = (C.c_void_p * 1)(zero.ctypes.data), (C.c_void_p * 1)(None)
    assert _lib.load_hip().pg_record_lines_from_text(0, 0, 1, op, tp, zero.ctypes.data, None, off.ctypes.data, None, 0) == _lib.PG_OK
    assert off[0] == 0


def test_null_jobs_are_invalid():
    lib = _lib.load_hip()
    err = C.create_string_buffer(64)
    zero = np.zeros(1, np.uint64)
    assert lib.pg_job_line_prefix(None, 0, zero.ctypes.data, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_line_prefix(None, 0, None, None, None, 0) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_lines(None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_lines(None, None, 0) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_lines_first(None, None, None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_record_lines(None, 0, None, None, 0, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_record_lines_packed(None, None, None, 0, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_device_record_lines(None, 0, None, None, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_job_record_lines_ms(None) == 0.0
