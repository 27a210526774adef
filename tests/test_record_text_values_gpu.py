"""The record text through the unit entry point, pg_record_text_from_fields, on every value the GL column can hold (GPU):

  every exponent -99 .. 99 x both signs x the mantissas {1000, 1200, 1230, 1234, 1204, 9000, 9999, 5050};
  every mantissa 1000 .. 9999 x both signs at exp10 in {-5, -4, -1, 0, 3, 4} (both sides of the change of notation);
  -inf; 0

as records of three values each, against the joins of calls.gl_text (tests/record_text_util.py), byte for byte.  The calls take
turns — a call, 255/255:10000, OK | EMPTY, NONE, NOT_UNIQUE, DEFERRED — as do KC's widths and no_call.  The records left to the
host are predicted from the inputs and asserted: a deferred call, a deferred value, a single value; they are put in the
middle of a block of 256 records and at both of its ends.  One launch, computed once for the module."""
import numpy as np
import pytest

from pangenie_amd import calls
from tests.record_text_util import DEFERRED, EMPTY, GL_DEFERRED, NONE, NOT_UNIQUE, OK, assert_text, expected_text, make_calls, make_gl

pytestmark = pytest.mark.gpu

MANTS = (1000, 1200, 1230, 1234, 1204, 9000, 9999, 5050)
EXPS = (-5, -4, -1, 0, 3, 4)
CALLS = ((0, 1, 37, OK), (255, 255, 10000, OK), (0, 0, 10000, OK | EMPTY), (0xFFFF, 0xFFFF, 0, NONE), (0xFFFF, 0xFFFF, 0, NOT_UNIQUE),
         (12, 107, 192, OK))
KCS = (0, 7, 42, 999, 1000, 65535)
# records left to the host: first, middle and last of block 0, first of block 1, the middle and end of block 2, the last record
HOSTS_DEFERRED_CALL = (0, 255, 256, 700)
HOSTS_DEFERRED_VALUE = (100, 767, -1)
HOSTS_ONE_VALUE = (101, 511, 512)


def all_values():
    v = [(s * m, x) for x in range(-99, 100) for s in (-1, 1) for m in MANTS]
    v += [(s * m, x) for x in EXPS for s in (-1, 1) for m in range(1000, 10000)]
    v[30:30] = [(0, -32768), (0, 0), (0, 0)]   # (record 10: not one of the host's)
    while len(v) % 3:
        v.append((0, -32768))
    return v


@pytest.fixture(scope="module")
def world():
    vals = all_values()
    R = len(vals) // 3
    rows = [CALLS[r % len(CALLS)] for r in range(R)]
    for r in HOSTS_DEFERRED_CALL:
        rows[r] = (0xFFFF, 0xFFFF, 0, DEFERRED)
    pairs, gl_off = [], [0]
    one = set(HOSTS_ONE_VALUE)
    bad = {r % R for r in HOSTS_DEFERRED_VALUE}
    for r in range(R):
        mine = vals[3 * r:3 * r + 3]
        if r in one:
            mine = mine[:1]
        if r in bad:
            mine = [mine[0], GL_DEFERRED, mine[2]]
        pairs += mine
        gl_off.append(len(pairs))
    cl, gl, gl_off = make_calls(rows), make_gl(pairs), np.array(gl_off, np.uint64)
    kc = np.array([KCS[(r // 2) % len(KCS)] for r in range(R)], np.uint16)
    no_call = np.array([(r // 7) % 2 for r in range(R)], np.uint8)
    want = expected_text(cl, gl_off, gl, kc, no_call)
    got = calls.record_text_from_fields(cl, gl_off, gl, kc, no_call)
    return dict(cl=cl, gl=gl, gl_off=gl_off, kc=kc, no_call=no_call, want=want, got=got, R=R)


def test_the_records_left_to_the_host_are_the_predicted_ones(world):
    R, (off, _, hosts) = world["R"], world["want"]
    predicted = sorted({r % R for r in HOSTS_DEFERRED_CALL + HOSTS_DEFERRED_VALUE + HOSTS_ONE_VALUE})
    assert np.flatnonzero(hosts).tolist() == predicted
    assert R > 3 * 256 and {0, 255, 256, R - 1} <= set(predicted)   # both ends of a block, the ends of the launch
    got_off = world["got"][0].astype(np.int64)
    assert np.flatnonzero(np.diff(got_off) == 0).tolist() == predicted


def test_every_value_prints_as_gl_text_joins_it(world):
    assert_text(world["got"][0], world["got"][1], world["want"][0], world["want"][1], "values")
    # every notation occurs, and every head
    text = world["want"][1]
    for piece in (b"e-99", b"e+99", b"-inf,0,0:", b"0.0001", b"e-05", b"9999:", b"255/255:10000:", b"0/0:10000:", b".:.:", b":65535"):
        assert piece in text, piece


def test_without_no_call_every_ok_call_is_printed(world):
    off, text = calls.record_text_from_fields(world["cl"], world["gl_off"], world["gl"], world["kc"])
    want_off, want_text, _ = expected_text(world["cl"], world["gl_off"], world["gl"], world["kc"], None)
    assert_text(off, text, want_off, want_text, "no_call = NULL")
    assert len(text) > len(world["want"][1])   # (a1/a2:gq: is longer than .:.:)


def test_the_bound_holds(world):
    assert len(world["got"][1]) <= calls.record_text_bound(world["R"], len(world["gl"]))
