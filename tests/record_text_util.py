"""Shared by the GPU tests of the record text (tests/test_record_text_*_gpu.py): the expected bytes of the GT:GQ:GL:KC column,
put together in Python from the fields — the call's numbers, calls.gl_text of every value (the host's pg_gl_text, one library
call per distinct value), KC — and which records are the host's (length 0), predicted from the inputs alone: a deferred call, a
value that has no text, fewer than three values.  No kernel of pg_record_text.hip is involved."""
import numpy as np

from pangenie_amd import calls
from tests.record_gl_util import texts_of_values

OK, NONE, NOT_UNIQUE, DEFERRED, EMPTY = calls.PG_CALL_OK, calls.PG_CALL_NONE, calls.PG_CALL_NOT_UNIQUE, calls.PG_CALL_DEFERRED, calls.PG_CALL_EMPTY
GL_DEFERRED = (0, calls.PG_GL_DEFERRED)
GL_NEG_INF = (0, -32768)


def make_calls(rows):
    """rows of (allele_1, allele_2, gq, flags)"""
    out = np.zeros(len(rows), calls.CALL_DTYPE)
    for i, (a, b, q, f) in enumerate(rows):
        out[i] = (a, b, q, f)
    return out


def make_gl(pairs):
    out = np.zeros(len(pairs), calls.GL_DTYPE)
    if len(pairs):
        p = np.asarray(pairs, np.int64).reshape(-1, 2)
        out["mant"], out["exp10"] = p[:, 0], p[:, 1]
    return out


def expected_text(cl, gl_off, gl, kc, no_call=None):
    """(off [R + 1], bytes, hosts [R]): the packed text, every record's first byte, and which records are the host's"""
    gl_off = np.asarray(gl_off).astype(np.int64)
    texts = texts_of_values(gl)
    R = len(cl)
    off = np.zeros(R + 1, np.uint64)
    hosts = np.zeros(R, bool)
    parts = []
    total = 0
    for r in range(R):
        vals = texts[gl_off[r]:gl_off[r + 1]]
        fl = int(cl["flags"][r])
        if (fl & 0xFF) == DEFERRED or len(vals) < 3 or any(t is None for t in vals):
            hosts[r] = True
        else:
            nc = no_call is not None and bool(no_call[r])
            head = "%d/%d:%d:" % (int(cl["allele_1"][r]), int(cl["allele_2"][r]), int(cl["gq"][r])) if (fl & 0xFF) == OK and not nc else ".:.:"
            t = (head + ",".join(vals) + ":%d" % int(kc[r])).encode()
            parts.append(t)
            total += len(t)
        off[r + 1] = total
    return off, b"".join(parts), hosts


def assert_text(got_off, got_text, want_off, want_text, what=""):
    """byte for byte; names the first record that differs"""
    got_off, want_off = np.asarray(got_off).astype(np.int64), np.asarray(want_off).astype(np.int64)
    assert len(got_off) == len(want_off), (what, len(got_off), len(want_off))
    if not np.array_equal(got_off, want_off) or got_text != want_text:
        for r in range(len(want_off) - 1):
            g, w = got_text[got_off[r]:got_off[r + 1]], want_text[want_off[r]:want_off[r + 1]]
            assert got_off[r] == want_off[r] and g == w, (what, "record", r, int(got_off[r]), int(want_off[r]), g[:80], w[:80])
        assert got_off[-1] == want_off[-1] and len(got_text) == len(want_text), (what, int(got_off[-1]), int(want_off[-1]), len(got_text))
        raise AssertionError((what, "the texts differ although every record agrees"))
