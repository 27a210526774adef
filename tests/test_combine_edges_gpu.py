"""Path subsets combined on the device, edge by edge (pangenie_amd/csrc/pg_combine.hip through pg_combine_bins and
pg_calls_from_combined): constructed chains whose combined map hangs on the union of the key sets, on a key held with the
value 0, on the order of the additions and their last bit, on the deferral cut, on the narrow / wide split.  A handful of
launches over all constructed variants (more than one block, not a multiple of 64); the yardstick is
pangenie_amd/genotyping_result.py — GenotypingResult.combine over the chains in the same order, in np.longdouble, then
normalize / get_likeliest_genotype / get_genotype_quality — computed once per launch."""
import math

import numpy as np
import pytest

from pangenie_amd import calls
from tests.calls_util import DEFERRED, NONE, NOT_UNIQUE, OK, assert_calls, geno_off_of
from tests.combine_util import LD, assert_bins, calls_yardstick, combined_yardstick

pytestmark = pytest.mark.gpu


class Chains:
    """variants over S chains in the layout of ContigBatch / ContigResult; a bin is (mantissa in [0.5, 1) or 0, exponent)"""

    def __init__(self, S):
        self.S = S
        self.aoff, self.ids, self.names = [0], [], []
        self.kept = [[] for _ in range(S)]
        self.pres = [[] for _ in range(S)]
        self.m = [[] for _ in range(S)]
        self.e = [[] for _ in range(S)]

    def add(self, name, A, chains, ids=None):
        """chains: per chain None (not kept) or (present [A], bins [A (A + 1) / 2])"""
        assert len(chains) == self.S, name
        n = A * (A + 1) // 2
        for s, c in enumerate(chains):
            pres, bins = c if c is not None else ([1] * A, [(0.75, -5)] * n)   # (bins that would count if the variant were kept)
            assert len(pres) == A and len(bins) == n, (name, s)
            self.kept[s].append(0 if c is None else 1)
            self.pres[s] += [int(p) for p in pres]
            for x in bins:
                m, e = (0.0, 0) if x[0] == 0 else x
                assert m == 0 or 0.5 <= m < 1.0, (name, x)
                self.m[s].append(m)
                self.e[s].append(e)
        self.ids += list(ids) if ids is not None else list(range(A))
        self.aoff.append(self.aoff[-1] + A)
        self.names.append(name)
        return len(self.names) - 1

    def arrays(self, order=None):
        order = list(range(self.S)) if order is None else order
        return (np.array(self.aoff, np.uint32), [np.array(self.kept[s], np.uint8) for s in order], [np.array(self.pres[s], np.uint8) for s in order],
                [np.array(self.m[s], np.float64) for s in order], [np.array(self.e[s], np.int32) for s in order])


def fr(x, shift=0):
    m, e = math.frexp(x)
    return (m, e + shift)


def rand_bins(rng, A, base=-40, spread=30, zero_frac=0.1):
    return [(0.0, 0) if rng.random() < zero_frac else (float(rng.uniform(0.5, 1.0)), int(base - rng.integers(0, spread + 1))) for _ in range(A * (A + 1) // 2)]


def rand_chain(rng, A, p_kept=0.85, p_pres=0.8, **kw):
    if rng.random() > p_kept:
        return None
    return ([int(x) for x in (rng.random(A) < p_pres)], rand_bins(rng, A, **kw))


BIN_12_OF_3 = 4   # bins of three alleles: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(20261020)
    c = Chains(3)
    tag = {}
    big = lambda n, e=-20: [(0.75, e)] * n
    # a wide variant first
    tag["wide_first"] = c.add("wide first", 6, [rand_chain(rng, 6, p_kept=1.0) for _ in range(3)])
    # the union of {0, 1} and {0, 2}: (1, 2) is no key
    tag["union"] = c.add("union", 3, [([1, 1, 0], rand_bins(rng, 3, zero_frac=0.0)), ([1, 0, 1], rand_bins(rng, 3, zero_frac=0.0)), None], ids=[0, 1, 2])
    tag["union_wide"] = c.add("union, wide", 7, [([1, 1, 0, 0, 0, 0, 0], rand_bins(rng, 7, zero_frac=0.0)), ([1, 0, 1, 0, 0, 0, 0], rand_bins(rng, 7, zero_frac=0.0)),
                                               None])
    # held with the value 0 by one chain, absent in the others: present and 0
    tag["zero_held"] = c.add("zero held", 2, [([1, 1], [fr(0.5), (0.0, 0), (0.0, 0)]), ([1, 0], big(3)), ([1, 0], big(3))])
    # kept in no chain; kept in one chain only
    tag["no_chain"] = c.add("kept in no chain", 3, [None, None, None])
    tag["no_chain_wide"] = c.add("kept in no chain, wide", 8, [None, None, None])
    tag["one_chain"] = c.add("kept in one chain", 3, [None, ([1, 1, 1], rand_bins(rng, 3, zero_frac=0.0)), None], ids=[3, 9, 27])
    tag["one_chain_wide"] = c.add("kept in one chain, wide", 6, [None, None, ([1, 1, 0, 1, 1, 1], rand_bins(rng, 6, zero_frac=0.0))])
    # the order: (1 + 2^-64) + 2^-64 == 1, (2^-64 + 2^-64) + 1 == 1 + 2^-63
    one, t = ([1], [fr(1.0)]), ([1], [fr(2.0 ** -64)])
    tag["order_a"] = c.add("1, 2^-64, 2^-64", 1, [one, t, t])
    tag["order_b"] = c.add("2^-64, 2^-64, 1", 1, [t, t, one])
    # sums that need 54 .. 64 bits (kept exactly) and 65 (the last bit is the half bit)
    tag["widths"] = []
    for gap in range(1, 13):
        for rep in range(4):
            fa = (int(rng.integers(0, 1 << 52)) | (1 << 52) | 1) & ~((rep & 1) << 51)
            fb = (int(rng.integers(0, 1 << 52)) | (1 << 52) | 1) & ~((rep & 1) << 51)
            a, b = ([1], [(fa / 2.0 ** 53, -30)]), ([1], [(fb / 2.0 ** 53, -30 - gap)])
            tag["widths"].append((gap, c.add(f"{53 + gap}-bit sum #{rep}", 1, [a, b, None] if rep < 2 else [b, None, a])))
    # a key whose largest summand lies below 2^-16300: that bin is deferred, and the variant's call; its neighbours are not
    c.add("before the deferred", 2, [([1, 1], big(3)), ([1, 1], big(3, -16290)), None])
    tag["deferred"] = c.add("a deferred key", 2, [([1, 1], [fr(0.9, -20), (0.75, -16301), fr(0.3, -20)]), ([1, 1], [fr(0.9, -20), (0.6, -16350), (0.0, 0)]),
                                                   ([1, 1], [(0.0, 0), (0.5, -16440), fr(0.1, -20)])])
    c.add("behind the deferred", 2, [([1, 1], big(3)), ([1, 1], big(3, -16299)), None])
    tag["deferred_wide"] = c.add("a deferred key, wide", 6, [([1] * 6, big(20) + [(0.75, -16310)]), ([1] * 6, big(20) + [(0.5, -16400)]), None])
    tag["all_deferred"] = c.add("every key deferred", 2, [([1, 1], big(3, -16320)), ([1, 1], big(3, -16390)), None])
    tag["edge_decided"] = c.add("largest summand at 2^-16300", 1, [([1], [(0.5, -16299)]), ([1], [(0.75, -16310)]), ([1], [(0.99, -16400)])])
    # a tiny summand beside a large one: not deferred, the x87's sum; mid + tiny + large is the example of pg_combine.h
    tag["tiny_large"] = c.add("tiny, large", 2, [([1, 1], [(0.75, -16400), (0.6, -16390), (0.51, -16445)]), ([1, 1], [(0.6, -20), (0.7, -300), (0.9, -16000)]), None])
    tag["mid_tiny_large"] = c.add("mid, tiny, large", 1, [([1], [(0.5, -16363)]), ([1], [(0.5 + 2.0 ** -21, -16427)]), ([1], [(0.5, -16299)])])
    # a tie within 1e-10 after combining that no single chain has
    tag["tie"] = c.add("tie after combining", 2, [([1, 1], [fr(0.5, -70), fr(0.1, -70), fr(0.3, -70)]), ([1, 1], [fr(0.3, -70), fr(0.1, -70), fr(0.5 + 4e-11, -70)]),
                                                  None], ids=[0, 5])
    w0, w1 = [fr(0.01, -9)] * 21, [fr(0.01, -9)] * 21
    w0[3], w0[17], w1[3], w1[17] = fr(0.5, -9), fr(0.3, -9), fr(0.3, -9), fr(0.5, -9)
    tag["tie_wide"] = c.add("tie after combining, wide", 6, [([1] * 6, w0), None, ([1] * 6, w1)])
    tag["no_tie"] = c.add("no tie after combining", 2, [([1, 1], [fr(0.5, -70), fr(0.1, -70), fr(0.3, -70)]), ([1, 1], [fr(0.3, -70), fr(0.1, -70), fr(0.5 + 4e-10, -70)]),
                                                        None], ids=[0, 5])
    # allele counts on both sides of the narrow / wide split and beyond the lanes of a wave, alleles absent in some chains
    for A in (1, 2, 5, 6, 12):
        for rep in range(6):
            base, spread = -int(rng.integers(0, 3000)), int(rng.choice([2, 30, 90]))
            ids = np.sort(rng.choice(300, A, replace=False)).tolist()
            c.add(f"A={A} #{rep}", A, [rand_chain(rng, A, base=base, spread=spread) for _ in range(3)], ids=ids)
    tag["A70"] = c.add("A=70", 70, [rand_chain(rng, 70, p_kept=1.0, spread=12) for _ in range(3)], ids=list(range(5, 75)))
    # many more: several blocks, a ragged last wave
    for i in range(520):
        A = int(rng.integers(1, 6)) if rng.random() > 0.04 else int(rng.integers(6, 13))
        base, spread = -int(rng.integers(0, 12000)), (1, 8, 70, 130)[int(rng.integers(0, 4))]
        c.add(f"random #{i}", A, [rand_chain(rng, A, base=base, spread=spread) for _ in range(3)], ids=np.sort(rng.choice(300, A, replace=False)).tolist())
    tag["wide_last"] = c.add("wide last", 6, [rand_chain(rng, 6, p_kept=1.0, zero_frac=0.0) for _ in range(3)])
    V = len(c.names)
    assert V % 64 != 0 and V > 512
    ids = np.array(c.ids, np.uint16)
    arrays = c.arrays()
    got = calls.combine_bins(*arrays)
    want, deferred = combined_yardstick(arrays[0], ids, *arrays[1:])
    return c, tag, ids, arrays, got, want, deferred


def test_every_combined_bin_is_the_long_double_sum_in_the_order_of_the_chains(case):
    c, tag, ids, arrays, got, want, deferred = case
    n_keys, n_deferred = assert_bins(arrays[0], ids, got, want, deferred, "edges")
    assert n_keys > 2000 and n_deferred >= 5


def test_the_reversed_order_gives_the_reversed_sums(case):
    c, tag, ids, arrays, got, want, deferred = case
    rev = c.arrays(order=[2, 1, 0])
    got_r = calls.combine_bins(*rev)
    want_r, deferred_r = combined_yardstick(rev[0], ids, *rev[1:])
    assert_bins(rev[0], ids, got_r, want_r, deferred_r, "reversed")
    differ = (got_r["m"] != got["m"]) | (got_r["e"] != got["e"])
    assert differ.any() and (got_r["flags"] == got["flags"]).all()   # the order changes last bits, never the key sets
    goff = geno_off_of(arrays[0])
    assert differ[int(goff[tag["order_a"]])] and differ[int(goff[tag["order_b"]])]


def test_the_constructions_hit_what_they_aim_at(case):
    """the expected values of the edges that have a closed form, stated, so that a construction that silently misses its edge does not pass"""
    c, tag, ids, arrays, got, want, deferred = case
    goff = geno_off_of(arrays[0])
    val = calls.combined_to_longdouble(got)
    bins = lambda name: slice(int(goff[tag[name]]), int(goff[tag[name] + 1]))
    P, D = calls.PG_COMBINED_PRESENT, calls.PG_COMBINED_DEFERRED
    assert [int(f) for f in got["flags"][bins("union")]] == [P, P, P, P, 0, P]
    assert int(got["flags"][bins("union")][BIN_12_OF_3]) == 0
    assert int((got["flags"][bins("union_wide")] != 0).sum()) == 5
    assert [int(f) for f in got["flags"][bins("zero_held")]] == [P, P, P] and val[bins("zero_held")][1] == 0 and val[bins("zero_held")][2] == 0
    assert not got["flags"][bins("no_chain")].any() and not got["flags"][bins("no_chain_wide")].any()
    assert (got["flags"][bins("one_chain")] == P).all()
    assert val[bins("order_a")][0] == LD(1) and val[bins("order_b")][0] == LD(1) + LD(2.0) ** -63
    for gap, v in tag["widths"]:
        g = int(goff[v])
        parts = [np.ldexp(LD(c.m[s][g]), c.e[s][g]) for s in range(3) if c.kept[s][v]]
        exact = (val[g] - max(parts)) == min(parts)
        assert exact or gap >= 11, (gap, c.names[v])          # up to 64 bits nothing is lost
        assert not exact or gap <= 11, (gap, c.names[v])      # a 65-bit sum is rounded (both last bits are set: no exact sum)
    assert [int(f) for f in got["flags"][bins("deferred")]] == [P, P | D, P]
    assert int(got["flags"][bins("deferred_wide")][20]) == P | D and (got["flags"][bins("deferred_wide")][:20] == P).all()
    assert (got["flags"][bins("all_deferred")] == P | D).all()
    assert int(got["flags"][bins("edge_decided")][0]) == P
    assert (got["flags"][bins("tiny_large")] == P).all()
    assert int(got["flags"][bins("mid_tiny_large")][0]) == P and val[bins("mid_tiny_large")][0] == LD(2.0) ** -16300
    assert tag["wide_first"] == 0 and tag["wide_last"] == len(c.names) - 1


def test_the_calls_from_the_combined_bins_agree_with_the_long_double_host_route(case):
    c, tag, ids, arrays, got, want, deferred = case
    rec = calls.calls_from_combined(arrays[0], ids, got)
    expect = calls_yardstick(want)
    was_deferred = assert_calls(rec, expect, "combined calls")
    assert sorted(was_deferred) == sorted(v for v in range(len(want)) if deferred[v]), [c.names[v] for v in was_deferred]
    assert {tag["deferred"], tag["deferred_wide"], tag["all_deferred"]} <= set(was_deferred)
    fl = lambda name: int(rec[tag[name]]["flags"])
    assert fl("no_chain") == NONE and fl("no_chain_wide") == NONE
    assert fl("tie") == NOT_UNIQUE and fl("tie_wide") == NOT_UNIQUE and fl("no_tie") == OK
    assert (int(rec[tag["no_tie"]]["allele_1"]), int(rec[tag["no_tie"]]["allele_2"])) == (5, 5)
    # ... which no single chain has: each of the two chains alone gives a call
    v = tag["tie"]
    a0, g0 = int(arrays[0][v]), int(geno_off_of(arrays[0])[v])
    for s in (0, 1):
        alone = calls.calls_from_bins(np.array([0, 2], np.uint32), ids[a0:a0 + 2], [1], [1, 1], arrays[3][s][g0:g0 + 3], arrays[4][s][g0:g0 + 3])
        assert int(alone[0]["flags"]) == OK
    A = np.diff(arrays[0].astype(np.int64))
    ok = np.array([w is not None for w in expect])
    assert ok[A <= 5].sum() > 300 and ok[A > 5].sum() > 10 and (~ok).sum() > 10
    assert fl("deferred") == DEFERRED and fl("edge_decided") == OK


@pytest.mark.parametrize("S", [1, 9])
def test_one_chain_and_nine(S):
    rng = np.random.default_rng(7 + S)
    c = Chains(S)
    for A in (1, 2, 5, 6, 12, 70):
        for rep in range(1 if A == 70 else 12):
            base = -int(rng.integers(0, 9000))
            c.add(f"A={A} #{rep}", A, [rand_chain(rng, A, base=base, spread=40) for _ in range(S)], ids=np.sort(rng.choice(300, A, replace=False)).tolist())
    ids = np.array(c.ids, np.uint16)
    arrays = c.arrays()
    got = calls.combine_bins(*arrays)
    want, deferred = combined_yardstick(arrays[0], ids, *arrays[1:])
    n_keys, _ = assert_bins(arrays[0], ids, got, want, deferred, f"S={S}")
    assert n_keys > 500
    rec = calls.calls_from_combined(arrays[0], ids, got)
    assert_calls(rec, calls_yardstick(want), f"S={S} calls")
    if S == 1:   # the bins are the chain's own, the calls those of pg_calls_from_bins byte for byte
        own = np.ldexp(arrays[3][0].astype(LD), arrays[4][0].astype(np.int64))
        present = got["flags"] != 0
        assert (calls.combined_to_longdouble(got)[present] == own[present]).all() and present.sum() == n_keys
        direct = calls.calls_from_bins(arrays[0], ids, arrays[1][0], arrays[2][0], arrays[3][0], arrays[4][0])
        assert rec.tobytes() == direct.tobytes()


def test_argument_checks_and_the_empty_call():
    assert len(calls.combine_bins(np.zeros(1, np.uint32), [[]], [[]], [[]], [[]])) == 0
    assert len(calls.calls_from_combined(np.zeros(1, np.uint32), [], np.zeros(0, calls.COMBINED_DTYPE))) == 0
    with pytest.raises(ValueError):
        calls.combine_bins(np.array([0, 2], np.uint32), [[1]], [[1, 1]], [[0.5]], [[0]])   # three bins belong to two alleles
    with pytest.raises(ValueError):
        calls.combine_bins(np.array([0, 1], np.uint32), [], [], [], [])                     # no chain
