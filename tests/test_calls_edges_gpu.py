"""Genotype calls on the device, edge by edge (pangenie_amd/csrc/pg_calls.hip through pg_calls_from_bins): constructed bins
whose call hangs on the last bit of the reference's long double arithmetic (src/genotypingresult.cpp:118-210), on the tie
threshold, on the order of the keys, on absent alleles, on the narrow / wide split and on the deferral cut.  ONE launch over
all constructed variants (more than one block, not a multiple of 64, a wide variant first and last); the yardstick is
pangenie_amd/genotyping_result.py on the same bins (tests/calls_util.py), computed once."""
import math

import numpy as np
import pytest

from pangenie_amd import calls
from tests.calls_util import DEFERRED, NONE, NOT_UNIQUE, OK, assert_calls, yardstick

pytestmark = pytest.mark.gpu


class Bins:
    """variants in the layout of ContigBatch / ContigResult; a bin is given as (mantissa in [0.5, 1) or 0, exponent)"""

    def __init__(self):
        self.aoff, self.ids, self.kept, self.pres, self.m, self.e, self.names = [0], [], [], [], [], [], []

    def add(self, name, bins, kept=1, present=None, ids=None):
        n = len(bins)
        A = (math.isqrt(8 * n + 1) - 1) // 2
        assert A * (A + 1) // 2 == n, (name, n)
        for x in bins:
            m, e = (0.0, 0) if x[0] == 0 else x
            assert m == 0 or 0.5 <= m < 1.0, (name, x)
            self.m.append(m)
            self.e.append(e)
        self.ids += list(ids) if ids is not None else list(range(A))
        self.pres += list(present) if present is not None else [1] * A
        self.kept.append(kept)
        self.aoff.append(self.aoff[-1] + A)
        self.names.append(name)
        return len(self.names) - 1

    def arrays(self):
        return (np.array(self.aoff, np.uint32), np.array(self.ids, np.uint16), np.array(self.kept, np.uint8), np.array(self.pres, np.uint8),
                np.array(self.m, np.float64), np.array(self.e, np.int32))


def fr(x, shift=0):
    """an exact double as (mantissa, exponent + shift)"""
    m, e = math.frexp(x)
    return (m, e + shift)


def rand_bins(rng, A, base=-40, spread=30, zero_frac=0.1):
    n = A * (A + 1) // 2
    out = []
    for _ in range(n):
        if rng.random() < zero_frac:
            out.append((0.0, 0))
        else:
            out.append((float(rng.uniform(0.5, 1.0)), int(base - rng.integers(0, spread + 1))))
    return out


TIE = 0.0000000001


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(20261018)
    b = Bins()
    tag = {}
    # 13: a wide variant first
    tag["wide_first"] = b.add("wide first", rand_bins(rng, 6))
    # 1: 1, 3, 6, 10, 15 bins for k_calls; 21, 45 and more for k_calls_wide
    for A in (1, 2, 3, 4, 5, 6, 9):
        for rep in range(6):
            b.add(f"A={A} #{rep}", rand_bins(rng, A, base=-int(rng.integers(0, 3000)), spread=int(rng.choice([2, 30, 90]))))
    # more alleles than lanes: the rows of k_calls_wide take a second stride; some alleles absent
    pres70 = [int(x) for x in (rng.random(70) < 0.8)]
    tag["A70"] = b.add("A=70", rand_bins(rng, 70, spread=12), present=pres70, ids=list(range(5, 75)))
    # 2: not kept (bins that would give a call)
    tag["not_kept"] = b.add("not kept", [fr(0.9), fr(0.05), fr(0.05)], kept=0)
    tag["not_kept_wide"] = b.add("not kept, wide", rand_bins(rng, 7), kept=0)
    # 3: kept, one present allele: one key, GT a/a, GQ 10000
    tag["one_key"] = b.add("one present allele", [fr(0.1), fr(0.7, -300), fr(0.2)], present=[0, 1], ids=[4, 8])
    tag["one_key_wide"] = b.add("one present allele, wide", rand_bins(rng, 8, zero_frac=0.0), present=[0, 0, 0, 1, 0, 0, 0, 0])
    tag["no_key"] = b.add("kept, no present allele", [fr(0.5), fr(0.25), fr(0.25)], present=[0, 0])
    # 4: all bins zero
    tag["all_zero"] = b.add("all zero", [(0.0, 0)] * 6)
    tag["all_zero_wide"] = b.add("all zero, wide", [(0.0, 0)] * 21)
    tag["one_zero_key"] = b.add("one key, zero", [(0.0, 0)], present=[1])
    # 5: two equal maxima
    tag["equal_max"] = b.add("two equal maxima", [fr(0.4, -77), fr(0.2, -77), fr(0.4, -77)])
    w = rand_bins(rng, 6, base=-20, spread=3, zero_frac=0.0)
    w[3] = w[17] = (0.99, -10)
    tag["equal_max_wide"] = b.add("two equal maxima, wide", w)
    # 6: a runner-up at best - 1e-10 (1 +- 2^-20): fifteen keys, best and runner-up near 0.1, thirteen near 0.0615
    for name, sign in (("tie_inside", -1.0), ("tie_outside", 1.0)):
        d = TIE * (1.0 + sign * 2.0 ** -20)
        rest = (1.0 - 0.1 - (0.1 - d)) / 13.0
        bins = [fr(rest, -500)] * 15
        bins[4], bins[9] = fr(0.1, -500), fr(0.1 - d, -500)
        tag[name] = b.add(name, bins)
        wb = [fr(rest * 13.0 / 19.0, -9)] * 21   # the same among 21 keys
        wb[20], wb[2] = fr(0.1, -9), fr(0.1 - d, -9)
        tag[name + "_wide"] = b.add(name + " wide", wb)
    # 7: the best bin at 1 - m 2^-64 of the sum: B = 2 - 2^-52, the other key m 2^-63 (sum exact in 64 bits, B / sum rounds to 1 - m 2^-64)
    B = fr(2.0 - 2.0 ** -52)
    for m in range(5):
        tag[f"top{m}"] = b.add(f"best = 1 - {m} 2^-64", [B, (0.0, 0), fr(float(m) * 2.0 ** -63) if m else (0.0, 0)])
        tag[f"top{m}_wide"] = b.add(f"best = 1 - {m} 2^-64, wide", [(0.0, 0)] * 11 + [B] + [(0.0, 0)] * 8 + [fr(float(m) * 2.0 ** -63) if m else (0.0, 0)])   # B = genotype 2/2
    # 8: bins 60, 64, 70, 300 binary orders below the largest, before and behind it; a sum that lands on a tie and just above one
    for gap in (60, 64, 70, 300):
        big = (float(rng.uniform(0.5, 1.0)), -100)
        small = (float(rng.uniform(0.5, 1.0)), -100 - gap)
        b.add(f"small bin {gap} orders below, behind", [big, small, small])
        b.add(f"small bin {gap} orders below, in front", [small, small, big])
        b.add(f"small bin {gap} orders below, wide", [small] * 10 + [big] + [small] * 10)
    b.add("sum on a tie", [fr(1.0), fr(2.0 ** -64), (0.0, 0)])
    b.add("sum just above a tie", [fr(1.0), fr(2.0 ** -64 + 2.0 ** -110), (0.0, 0)])
    b.add("sum on a tie, odd", [fr(1.0 + 2.0 ** -52), fr(2.0 ** -64), fr(2.0 ** -63)])
    # 9: exponents near -16300, both sides; small bins next to a decided variant
    tag["deferred"] = b.add("largest bin below 2^-16300", [(0.75, -16300), (0.5, -16310), (0.6, -16305)])
    tag["deferred_wide"] = b.add("largest bin below 2^-16300, wide", [(0.5, -16320)] * 20 + [(0.99, -16300)])
    tag["deferred_deep"] = b.add("largest bin a subnormal long double", [(0.75, -16400), (0.5, -16420), (0.0, 0)])
    tag["decided_edge"] = b.add("largest bin at 2^-16300", [(0.5, -16299), (0.75, -16310), (0.6, -16305)])
    tag["decided_edge_wide"] = b.add("largest bin just above 2^-16300, wide", [(0.5, -16320)] * 20 + [(0.51, -16299)])
    b.add("small bins beside a decided one", [(0.75, -16290), (0.75, -16390), (0.5, -16500)])
    b.add("a bin that reads 0 as long double", [(0.5, -16445), (0.75, -16200), (0.5, -16445)])
    # 10, 11: absent alleles in the middle of the slot list, ids that are not the slot numbers
    tag["absent_middle"] = b.add("absent alleles in the middle", rand_bins(rng, 5, zero_frac=0.0), present=[1, 0, 1, 0, 1], ids=[2, 3, 11, 12, 40])
    tag["absent_wide"] = b.add("absent alleles in the middle, wide", rand_bins(rng, 9, zero_frac=0.0), present=[1, 0, 0, 1, 1, 0, 1, 0, 1],
                               ids=[1, 3, 5, 7, 9, 100, 200, 300, 65000])
    # 12: many more, so that the launch has several blocks and a ragged last wave
    for i in range(560):
        A = int(rng.integers(1, 6)) if rng.random() > 0.04 else int(rng.integers(6, 13))
        ids = np.sort(rng.choice(300, A, replace=False)).tolist()
        pres = [int(x) for x in (rng.random(A) < 0.85)]
        style = int(rng.integers(0, 4))
        bins = rand_bins(rng, A, base=-int(rng.integers(0, 12000)), spread=(1, 8, 70, 200)[style])
        if style == 0 and A > 1 and rng.random() < 0.3:   # one genotype owns the sum: GQ in the upper range
            bins[int(rng.integers(0, len(bins)))] = (0.9, bins[0][1] + int(rng.integers(40, 75)) if bins[0][0] else -3)
        b.add(f"random #{i}", bins, kept=int(rng.random() < 0.95), present=pres, ids=ids)
    # 13: a wide variant last
    tag["wide_last"] = b.add("wide last", rand_bins(rng, 6, zero_frac=0.0))
    arrays = b.arrays()
    V = len(b.names)
    assert V % 64 != 0 and V > 512
    got = calls.calls_from_bins(*arrays)
    want = yardstick(*arrays)
    return b, tag, arrays, got, want


def test_every_constructed_variant_agrees_with_the_long_double_host_route(case):
    b, tag, arrays, got, want = case
    deferred = assert_calls(got, want, "edges")
    # a deferred variant is expected, and only there
    assert sorted(deferred) == sorted([tag["deferred"], tag["deferred_wide"], tag["deferred_deep"]]), [b.names[v] for v in deferred]
    # the comparison is not empty-handed: calls, no-calls and both kernels are in it
    A = np.diff(arrays[0].astype(np.int64))
    ok = np.array([w is not None for w in want])
    assert ok[A <= 5].sum() > 300 and ok[A > 5].sum() > 15 and (~ok).sum() > 20
    gq = np.array([w[2] if w else -1 for w in want])
    assert (gq == 10000).any() and ((gq > 100) & (gq <= 192)).any() and ((gq >= 0) & (gq < 10)).any()


def test_the_constructions_hit_what_they_aim_at(case):
    """the expected values of the edges that have a closed form, stated — so that a construction that silently misses its edge
    (and a yardstick and a kernel that agree on something easier) does not pass"""
    b, tag, arrays, got, want = case
    rec = lambda name: (int(got[tag[name]]["allele_1"]), int(got[tag[name]]["allele_2"]), int(got[tag[name]]["gq"]), int(got[tag[name]]["flags"]))
    assert rec("not_kept")[3] == NONE and rec("not_kept_wide")[3] == NONE and rec("no_key")[3] == NONE
    assert rec("one_key") == (8, 8, 10000, OK)
    assert rec("one_key_wide") == (3, 3, 10000, OK)
    assert rec("all_zero")[3] == NONE and rec("all_zero_wide")[3] == NONE and rec("one_zero_key")[3] == NONE
    assert rec("equal_max")[3] == NOT_UNIQUE and rec("equal_max_wide")[3] == NOT_UNIQUE
    for suffix in ("", "_wide"):
        assert want[tag["tie_inside" + suffix]] is None and rec("tie_inside" + suffix)[3] == NOT_UNIQUE
        assert want[tag["tie_outside" + suffix]] is not None and rec("tie_outside" + suffix)[3] == OK
        # GQ 10000, then 192 for 2^-64, 189 for 2^-63, ... as (size_t)(-10 log10l(m 2^-64)) says
        expect = [10000] + [int(-10 * np.log10(np.longdouble(m) * np.longdouble(2.0) ** -64)) for m in range(1, 5)]
        assert expect[:3] == [10000, 192, 189]
        for m in range(5):
            r = rec(f"top{m}{suffix}")
            assert r[3] == OK and r[2] == expect[m] and want[tag[f"top{m}{suffix}"]][2] == expect[m], (m, suffix, r)
    assert rec("top1")[:2] == (0, 0) and rec("top1_wide")[:2] == (2, 2)
    assert rec("deferred")[3] == DEFERRED and rec("deferred_wide")[3] == DEFERRED and rec("deferred_deep")[3] == DEFERRED
    assert rec("decided_edge")[3] != DEFERRED and rec("decided_edge_wide")[3] != DEFERRED
    a = rec("absent_middle")
    assert a[3] != OK or ({a[0], a[1]} <= {2, 11, 40})
    a = rec("absent_wide")
    assert a[3] != OK or ({a[0], a[1]} <= {1, 7, 9, 200, 65000})
    for v in (tag["wide_first"], tag["wide_last"]):
        assert v in (0, len(b.names) - 1) and int(got[v]["flags"]) in (OK, NOT_UNIQUE)


def test_argument_checks_and_the_empty_call():
    assert len(calls.calls_from_bins(np.zeros(1, np.uint32), [], [], [], [], [])) == 0
    with pytest.raises(ValueError):
        calls.calls_from_bins(np.array([0, 2], np.uint32), [0, 1], [1], [1, 1], [0.5], [0])   # three bins belong to two alleles
