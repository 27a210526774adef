"""The C ABI of the record lines over slotted prefixes without a device (include/pangenie_hmm.h): the symbols
resolve, pg_record_lines_bound_slotted is the plain bound plus 5 R, pg_record_lines_from_text_slotted refuses what
pg_record_lines_from_text refuses, a slot beyond its prefix, slots without UK values and a buffer below the slotted bound —
PG_ERR_INVALID, before any device is asked for — and a well-formed call answers PG_ERR_DEVICE where there is no device (with
one, the lines).  Null jobs are invalid."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd import _lib, calls
from pangenie_amd.hmm import PanGenieError

NEW_SYMBOLS = ["pg_record_lines_bound_slotted", "pg_job_line_prefix_slotted", "pg_job_line_prefix_strided", "pg_record_lines_from_text_slotted"]


def test_the_symbols_resolve_and_are_listed():
    lib = _lib.load_hip()
    header = (Path(__file__).resolve().parent.parent / "include" / "pangenie_hmm.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_ABI_SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(lib, name).argtypes is not None, name


def test_the_slotted_bound_is_the_plain_bound_and_five_bytes_a_record():
    for args in [(0, 0, 0, 0), (0, 7, 0, 0), (1, 1, 0, 0), (3, 2, 10, 12), (1025, 65, 123456, 7654321), (1 << 31, 512, 1 << 36, 1 << 40)]:
        assert calls.record_lines_bound_slotted(*args) == calls.record_lines_bound(*args) + 5 * args[0], args
    assert calls.record_lines_bound_slotted(1, 1, 0, 0) == 7          # five digits, a tab and a newline


def case():
    """three records, two members; the slots at a prefix's end, in an empty prefix and inside"""
    prefix = (np.array([0, 2, 2, 5], np.uint64), np.frombuffer(b"abcde", np.uint8))
    texts = [(np.array([0, 1, 3, 6], np.uint64), np.frombuffer(b"ABBCCC", np.uint8)),
             (np.array([0, 3, 5, 6], np.uint64), np.frombuffer(b"xxxyyz", np.uint8))]
    return prefix, texts, np.array([2, 0, 1], np.uint32), np.array([0, 65535, 10], np.uint16)


def raw(prefix, texts, slot, uk, cap=None, n=3, members=None, off="own", out="own"):
    lib = _lib.load_hip()
    S = len(texts) if members is None else members
    bound = (calls.record_lines_bound if slot is None else calls.record_lines_bound_slotted)(3, len(texts), 5, 12)
    cap = bound if cap is None else cap
    op = (C.c_void_p * max(len(texts), 1))(*[t[0].ctypes.data for t in texts])
    tp = (C.c_void_p * max(len(texts), 1))(*[t[1].ctypes.data for t in texts])
    o, b = np.zeros(4, np.uint64), np.zeros(max(min(cap, 1 << 16), 1), np.uint8)   # (a refusal comes before any of it is written)
    p = lambda a: None if a is None else a.ctypes.data
    return lib.pg_record_lines_from_text_slotted(0, n, S, op, tp, p(prefix[0]), p(prefix[1]), p(slot), p(uk), o.ctypes.data if off == "own" else None,
                                                 b.ctypes.data if out == "own" else None, cap)


def test_a_well_formed_call_answers_a_device_error_without_a_device():
    prefix, texts, slot, uk = case()
    if _lib.load_hip().pg_hmm_device_count() > 0:
        off, lines = calls.record_lines_from_text_slotted(texts, prefix, slot, uk)
        assert lines == b"ab0\tA\txxx\n65535\tBB\tyy\nc10de\tCCC\tz\n" and off.tolist() == [0, 10, 22, 34]
        off, lines = calls.record_lines_from_text_slotted(texts, prefix)
        assert lines == b"ab\tA\txxx\n\tBB\tyy\ncde\tCCC\tz\n" and off.tolist() == [0, 9, 16, 26]
    else:
        with pytest.raises(PanGenieError) as e:
            calls.record_lines_from_text_slotted(texts, prefix, slot, uk)
        assert e.value.code == _lib.PG_ERR_DEVICE
        assert raw(prefix, texts, slot, uk) == _lib.PG_ERR_DEVICE
        assert raw(prefix, texts, None, None) == _lib.PG_ERR_DEVICE


def test_what_is_malformed_is_refused_before_any_device_is_asked_for():
    prefix, texts, slot, uk = case()
    INV = _lib.PG_ERR_INVALID
    # a slot beyond its prefix (record 1's prefix is empty: only 0 fits), slots without UK values
    for r, at in ((0, 3), (1, 1), (2, 4), (2, 0xFFFFFFFF)):
        bad = slot.copy()
        bad[r] = at
        assert raw(prefix, texts, bad, uk) == INV, (r, at)
    assert raw(prefix, texts, slot, None) == INV
    # a buffer below the slotted bound: the plain bound is enough only without slots
    plain, slotted = calls.record_lines_bound(3, 2, 5, 12), calls.record_lines_bound_slotted(3, 2, 5, 12)
    assert raw(prefix, texts, slot, uk, cap=slotted - 1) == INV and raw(prefix, texts, slot, uk, cap=plain) == INV and raw(prefix, texts, slot, uk, cap=0) == INV
    assert raw(prefix, texts, None, None, cap=plain - 1) == INV
    # what pg_record_lines_from_text refuses: null arrays, offsets that do not start at 0 or shrink, no members, too many records
    assert raw((None, prefix[1]), texts, slot, uk) == INV and raw((prefix[0], None), texts, slot, uk) == INV
    assert raw(prefix, texts, slot, uk, off=None) == INV and raw(prefix, texts, slot, uk, out=None) == INV
    assert raw((np.array([1, 2, 2, 5], np.uint64), prefix[1]), texts, np.zeros(3, np.uint32), uk) == INV
    assert raw((np.array([0, 3, 2, 5], np.uint64), prefix[1]), texts, np.zeros(3, np.uint32), uk) == INV
    assert raw(prefix, [texts[0], (np.array([1, 3, 5, 6], np.uint64), texts[1][1])], slot, uk) == INV
    assert raw(prefix, texts, slot, uk, members=0) == INV
    assert raw(prefix, texts, None, None, n=1 << 31) == INV
    # no records: the offsets alone
    off, zero = np.ones(1, np.uint64), np.zeros(1, np.uint64)
    op, tp = (C.c_void_p * 1)(zero.ctypes.data), (C.c_void_p * 1)(None)
    none = np.zeros(1, np.uint32)
    assert _lib.load_hip().pg_record_lines_from_text_slotted(0, 0, 1, op, tp, zero.ctypes.data, None, none.ctypes.data, none.ctypes.data, off.ctypes.data,
                                                             None, 0) == _lib.PG_OK
    assert off[0] == 0


def test_null_jobs_are_invalid():
    lib = _lib.load_hip()
    err = C.create_string_buffer(64)
    zero, none = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    assert lib.pg_job_line_prefix_slotted(None, 0, zero.ctypes.data, None, none.ctypes.data, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_line_prefix_slotted(None, 0, None, None, None, None, 0) == _lib.PG_ERR_INVALID
    assert lib.pg_job_line_prefix_strided(None, 0, 1, zero.ctypes.data, None, none.ctypes.data, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_line_prefix_strided(None, 0, 1, None, None, None, None, 0) == _lib.PG_ERR_INVALID
