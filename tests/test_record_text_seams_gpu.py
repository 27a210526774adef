"""The seams of the record text's kernels, through pg_record_text_from_fields (GPU), byte for byte against
tests/record_text_util.expected_text:

  counts   R in {1, 255, 256, 257, 1025} records of mixed widths — 3, 6, 10 and 21 values — with records of the host's among
           them: a block of 256 records is the smallest shape at which the scan of the lengths and the stage have a seam;
  stage    a block of 256 records of 21 values holds more text than the stage takes at once (32 KB less 16 bytes): a record's
           text crosses the end of the stage — which record is worked out from the expected offsets and asserted;
  residue  17 blocks whose lengths are made 1 mod 16: a block's byte range starts at every residue mod 16 (asserted on the
           expected offsets), so the unaligned head and tail of the 16-byte stores take every shape;
  wide     a record of 820 values (40 alleles) and one of 32 896 (256 alleles), each once between narrow neighbours, and a
           wide record that is the host's: the wave-per-record path and the windows that go around it."""
import numpy as np
import pytest

from pangenie_amd import _lib, calls
from tests.record_text_util import DEFERRED, GL_DEFERRED, NONE, OK, assert_text, expected_text, make_calls, make_gl

pytestmark = pytest.mark.gpu

BLOCK = 256
WINDOW = 32768 - 16


def random_values(rng, n):
    """values of every notation and length"""
    kind = rng.integers(0, 10, n)
    mant = rng.integers(1000, 10000, n)
    mant = np.where(kind < 3, mant // 100 * 100, mant) * rng.choice([-1, 1], n)   # trailing zeros: shorter texts
    exp = np.where(kind % 2 == 0, rng.integers(-5, 5, n), rng.integers(-99, 100, n))
    pairs = np.stack([mant, exp], 1)
    pairs[kind == 9] = (0, -32768)
    pairs[(kind == 8) & (rng.random(n) < 0.3)] = (0, 0)
    return [tuple(int(x) for x in p) for p in pairs]


def random_records(rng, widths, hosts=()):
    """one record per entry of `widths`; the records listed in `hosts` get a deferred call or a deferred value in turn"""
    rows, pairs, gl_off = [], [], [0]
    for r, w in enumerate(widths):
        vals = random_values(rng, w)
        row = (int(rng.integers(0, 3)), int(rng.integers(3, 256)), int(rng.choice([0, 9, 45, 192, 10000])), OK) if rng.random() < 0.8 else (0xFFFF, 0xFFFF, 0, NONE)
        if r in hosts:
            if list(hosts).index(r) % 2:
                vals[w // 2] = GL_DEFERRED
            else:
                row = (0xFFFF, 0xFFFF, 0, DEFERRED)
        rows.append(row)
        pairs += vals
        gl_off.append(len(pairs))
    kc = rng.choice([0, 3, 27, 311, 4096, 65535], len(widths)).astype(np.uint16)
    return make_calls(rows), np.array(gl_off, np.uint64), make_gl(pairs), kc


def run_and_compare(cl, gl_off, gl, kc, what, no_call=None):
    want_off, want_text, hosts = expected_text(cl, gl_off, gl, kc, no_call)
    off, text = calls.record_text_from_fields(cl, gl_off, gl, kc, no_call)
    assert_text(off, text, want_off, want_text, what)
    return want_off.astype(np.int64), hosts


@pytest.mark.parametrize("R", [1, 255, 256, 257, 1025])
def test_record_counts_around_a_block(R):
    rng = np.random.default_rng(1000 + R)
    widths = rng.choice([3, 6, 10, 21], R)
    hosts = sorted({0, R // 2, R - 1} | ({255, 256} if R > 256 else set())) if R > 1 else []
    cl, gl_off, gl, kc = random_records(rng, widths, hosts)
    no_call = (rng.random(R) < 0.2).astype(np.uint8)
    off, h = run_and_compare(cl, gl_off, gl, kc, "R = %d" % R, no_call)
    assert np.flatnonzero(h).tolist() == hosts
    if R == 1:
        assert off[1] > 0


def test_a_record_crosses_the_end_of_the_stage():
    rng = np.random.default_rng(7)
    cl, gl_off, gl, kc = random_records(rng, [21] * (2 * BLOCK + 40), hosts=[300])
    off, _ = run_and_compare(cl, gl_off, gl, kc, "stage")
    for b in (0, 1):   # both full blocks hold more than one window, and a record lies across the first window's end
        lo, hi = off[b * BLOCK], off[(b + 1) * BLOCK]
        assert hi - lo > WINDOW
        r = int(np.searchsorted(off, lo + WINDOW, "right")) - 1
        assert off[r] < lo + WINDOW < off[r + 1] and b * BLOCK <= r < (b + 1) * BLOCK, (b, r)


def test_a_block_starts_at_every_residue_mod_16():
    rng = np.random.default_rng(16)
    n_blocks = 17
    widths = rng.choice([3, 6, 10], n_blocks * BLOCK)
    widths[BLOCK - 1::BLOCK] = 3
    cl, gl_off, gl, kc = random_records(rng, widths)
    # the last record of every block gets the values that make the block's length 1 mod 16
    fill = [(1000, 0), (1200, 0), (-1000, 0), (-1200, 0), (-1230, 0), (-1234, 0), (-1234, 1), (-1234, -2), (-1234, -3), (-1234, -4), (-1234, -5)]   # 1, 3, 2, 4, 5, 6, 6, 8, 9, 10, 10 bytes
    for b in range(n_blocks):
        last = (b + 1) * BLOCK - 1
        g0 = int(gl_off[last])
        first = b * BLOCK
        before = int(expected_text(cl[first:last], gl_off[first:last + 1] - gl_off[first], gl[int(gl_off[first]):g0], kc[first:last])[0][-1])
        done = False
        for x in fill:
            for y in fill:
                gl[g0], gl[g0 + 1], gl[g0 + 2] = x, y, (0, 0)
                mine = int(expected_text(cl[last:last + 1], np.array([0, 3]), gl[g0:g0 + 3], kc[last:last + 1])[0][-1])
                if mine and (before + mine) % 16 == 1:
                    done = True
                    break
            if done:
                break
        assert done, b
    off, hosts = run_and_compare(cl, gl_off, gl, kc, "residues")
    assert not hosts.any()
    assert sorted(int(off[b * BLOCK]) % 16 for b in range(16)) == list(range(16))


@pytest.mark.parametrize("n_wide", [820, 32896])
def test_a_wide_record_between_narrow_neighbours(n_wide):
    lib = _lib.load_hip()
    rng = np.random.default_rng(n_wide)
    widths = [3, 6, n_wide, 10, 3]
    cl, gl_off, gl, kc = random_records(rng, widths)
    cl[2] = (17, 255, 10000, OK)
    off, hosts = run_and_compare(cl, gl_off, gl, kc, "wide %d" % n_wide)
    assert not hosts.any()
    assert off[3] - off[2] > 4 * n_wide
    assert off[-1] <= lib.pg_record_text_bound(len(widths), len(gl))


def test_wide_records_among_many_and_one_of_the_hosts():
    rng = np.random.default_rng(99)
    widths = [int(x) for x in rng.choice([3, 6, 10, 21], 300)]
    for at in (0, 128, 255, 256, 299):   # at both ends of a block, in the middle, two in a row across the seam
        widths[at] = 820
    cl, gl_off, gl, kc = random_records(rng, widths, hosts=[128, 200])   # (128: wide, a deferred call; 200: narrow, a deferred value)
    off, hosts = run_and_compare(cl, gl_off, gl, kc, "wide among many")
    assert np.flatnonzero(hosts).tolist() == [128, 200]
    gl[int(gl_off[255]) + 400] = GL_DEFERRED   # a wide record with one deferred value in its middle
    off, hosts = run_and_compare(cl, gl_off, gl, kc, "wide, deferred value")
    assert np.flatnonzero(hosts).tolist() == [128, 200, 255]
