"""The digits of the GL column by the DEVICE's own log10 / log1p (k_gl_values of pangenie_amd/csrc/pg_calls.hip through
pg_gl_from_values): 2^20 likelihoods m 2^e of four families — log-uniform over the whole exponent range, x in [2^-40, 1),
1 - d 2^-64 with d of every magnitude, 1 + d 2^-63 — and 200 constructed boundaries d.ddd5 10^k with their neighbours three
windows away, in ONE launch.  The yardstick is numpy's long double: log10l of the same value, its four significant digits.
Conditions, not measurements: every value that is not deferred equals the yardstick; at most 10^-6 of the random values are
deferred (about 2e-9 are expected: the window is 1e-9 on either side of a boundary); every constructed boundary is deferred and
its neighbours are not."""
import numpy as np
import pytest

from pangenie_amd import calls
from tests.record_gl_util import is_deferred, text_of_log, texts_of_values

pytestmark = pytest.mark.gpu
LD = np.longdouble
TOP = np.uint64(1) << np.uint64(63)
N = 1 << 20
WINDOW = 1e-9


def pair_of(x):
    """the pair (m, e) of long doubles x > 0: x = m 2^e exactly, m in [2^63, 2^64)"""
    f, ex = np.frexp(np.asarray(x, LD))
    return np.ldexp(f, 64).astype(np.uint64), (ex - 64).astype(np.int32)


def digits_of(v):
    """(mant, exp10) of long double logarithms v != 0, and where the long double product below is too close to a rounding
    boundary to say (those are read from the exact decimal expansion instead)"""
    a = np.abs(v)
    k = np.floor(np.log10(a)).astype(np.int64)
    s = a * np.power(LD(10), (3 - k).astype(LD))
    low, high = s < 1000, s >= 10000
    k = k - low + high
    s = a * np.power(LD(10), (3 - k).astype(LD))
    fl = np.floor(s)
    unsure = np.abs((s - fl) - LD(0.5)) < LD(1e-12)   # the product and the power are good to 1e-15 of s
    r = (fl + (s - fl > LD(0.5))).astype(np.int64)
    k = np.where(r == 10000, k + 1, k)
    r = np.where(r == 10000, 1000, r)
    return np.where(v < 0, -r, r), k, unsure


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(20261021)
    m = rng.integers(0, 1 << 63, N, dtype=np.uint64) | TOP
    e = np.zeros(N, np.int32)
    fam = np.arange(N) % 4
    e[fam == 0] = -64 - rng.integers(0, 16300, (fam == 0).sum())   # E in [-16299, 0]
    e[fam == 1] = -64 - rng.integers(0, 40, (fam == 1).sum())
    n2 = int((fam == 2).sum())
    d = np.maximum(rng.integers(0, 1 << 63, n2, dtype=np.uint64) >> rng.integers(0, 63, n2).astype(np.uint64), np.uint64(1))
    m[fam == 2] = np.uint64(0) - d                                  # 2^64 - d
    e[fam == 2] = -64
    n3 = int((fam == 3).sum())
    d = np.maximum(rng.integers(0, 1 << 63, n3, dtype=np.uint64) >> rng.integers(0, 63, n3).astype(np.uint64), np.uint64(1))
    m[fam == 3] = TOP + d
    e[fam == 3] = -63
    # the boundaries: t = d.ddd5 10^k; 10^-t, and 10^-(t -+ 3 windows)
    bm, be, bd, bk = [], [], [], []
    for k in range(-6, 4):
        for _ in range(20):
            dddd = int(rng.integers(1000, 4900 if k == 3 else 10000))
            t = LD(f"{dddd}5e{k - 4}")
            w = LD(3) * LD(WINDOW) * LD(10) ** LD(k - 3)
            mm, ee = pair_of(np.power(LD(10), -np.array([t, t - w, t + w], LD)))
            bm += mm.tolist()
            be += ee.tolist()
            bd.append(dddd)
            bk.append(k)
    m = np.concatenate([m, np.array(bm, np.uint64), np.array([TOP, 0, TOP, 0xFFFFFFFFFFFFFFFF], np.uint64)])
    e = np.concatenate([e, np.array(be, np.int32), np.array([-63, 0, -16300 - 63, -16300 - 64], np.int32)])
    got = calls.gl_from_values(m, e)
    return m, e, got, np.array(bd), np.array(bk)


def test_every_decided_value_is_the_long_doubles(case):
    m, e, got, _, _ = case
    x = np.ldexp(m[:N].astype(LD), e[:N].astype(np.int64))
    assert (x > 0).all() and np.array_equal(pair_of(x)[0], m[:N])   # the yardstick sees the very value
    mant, k, unsure = digits_of(np.log10(x))
    deferred = is_deferred(got[:N])
    print("random values", N, "deferred", int(deferred.sum()), "read from the exact expansion", int(unsure.sum()))
    assert deferred.sum() <= N * 1e-6
    ok = ~deferred & ~unsure
    bad = np.flatnonzero(ok & ((got["mant"][:N] != mant) | (got["exp10"][:N] != k)))
    assert len(bad) == 0, [(hex(int(m[i])), int(e[i]), got[i], int(mant[i]), int(k[i])) for i in bad[:10]]
    # ... those too close for the long double product, and a sample of the rest, through the exact decimal expansion
    rng = np.random.default_rng(1)
    for i in np.concatenate([np.flatnonzero(unsure & ~deferred), rng.choice(N, 4000, replace=False)]):
        if not deferred[i]:
            assert calls.gl_text(got[i]) == text_of_log(np.log10(x[i])), (hex(int(m[i])), int(e[i]), got[i])
    assert (got["mant"][:N] > 0).sum() == (np.arange(N) % 4 == 3).sum() - deferred[np.arange(N) % 4 == 3].sum()   # the sign is the logarithm's


def test_the_constructed_boundaries_are_deferred_and_their_neighbours_decided(case):
    m, e, got, bd, bk = case
    b = got[N:N + 600].reshape(200, 3)
    assert is_deferred(b[:, 0]).all(), np.flatnonzero(~is_deferred(b[:, 0]))
    assert not is_deferred(b[:, 1:]).any()
    assert np.array_equal(-b["mant"][:, 1], bd) and np.array_equal(-b["mant"][:, 2], bd + 1)
    assert np.array_equal(b["exp10"][:, 1], bk) and np.array_equal(b["exp10"][:, 2], bk)
    x = np.ldexp(m[N:N + 600].astype(LD), e[N:N + 600].astype(np.int64)).reshape(200, 3)
    texts = texts_of_values(b.reshape(-1)).reshape(200, 3)
    for i in range(200):
        for j in (1, 2):
            assert texts[i, j] == text_of_log(np.log10(x[i, j])), (i, j)


def test_one_zero_and_both_sides_of_the_cut(case):
    _, _, got, _, _ = case
    one, zero, at, below = got[N + 600:]
    assert (int(one["mant"]), int(one["exp10"])) == (0, 0) and calls.gl_text(one) == "0"
    assert (int(zero["mant"]), int(zero["exp10"])) == (0, calls.PG_GL_NEG_INF) and calls.gl_text(zero) == "-inf"
    assert calls.gl_text(at) == "-4907" == text_of_log(LD(-16300) * np.log10(LD(2)))
    assert is_deferred(got[N + 603:]).all()


def test_refusals():
    assert len(calls.gl_from_values(np.zeros(0, np.uint64), np.zeros(0, np.int32))) == 0
    from pangenie_amd.hmm import PanGenieError
    with pytest.raises(PanGenieError) as err:
        calls.gl_from_values(np.array([1 << 62], np.uint64), np.array([-63], np.int32))   # not normalised
    assert err.value.code == -1
    with pytest.raises(PanGenieError) as err:
        calls.gl_from_values(np.array([0], np.uint64), np.array([3], np.int32))           # zero has exponent 0
    assert err.value.code == -1
    with pytest.raises(ValueError):
        calls.gl_from_values(np.zeros(2, np.uint64), np.zeros(3, np.int32))
