"""GT, GQ and GL per VCF record from combined bins, edge by edge (pangenie_amd/csrc/pg_combine_records.hip through
pg_record_calls_from_combined and pg_record_gl_from_combined): constructed chains are combined with calls.combine_bins, then the
records of a constructed plan are formed from the combined bins — the union of the key sets, a bubble no chain holds, held
values that are all 0, a deferred key among large ones, the order example of pg_combine.h, a tie that exists only on the folded
map, a quality of 10000, a column of one chain only, and bubbles of 6, 65 and 256 alleles whose two chains share one allele.
ONE launch of each kernel pair over all bubbles (more than one block of records, a ragged last wave, a wide bubble first and
last); the yardstick is tests/combined_records_util.records_yardstick over tests/combine_util.combined_yardstick, computed once.
Groups of ONE chain against pg_record_calls_from_bins / pg_record_gl_from_bins byte for byte."""
import numpy as np
import pytest

from pangenie_amd import calls
from tests.calls_util import DEFERRED, NONE, NOT_UNIQUE, OK
from tests.combine_util import combined_yardstick
from tests.combined_records_util import records_of, records_yardstick
from tests.record_calls_util import EMPTY, assert_record_calls
from tests.record_gl_util import assert_record_gl, is_deferred, texts_of_values
from tests.test_combine_edges_gpu import Chains, fr, rand_bins, rand_chain

pytestmark = pytest.mark.gpu


def rand_records(rng, ids, n, undefined=0.1, alleles=None):
    """n records over the bubble's ids: (own by allele ID, defined per record allele); alleles: the records' allele counts"""
    n_ids = max(ids) + 1
    out = []
    for i in range(n):
        nA = int(alleles[i]) if alleles is not None else int(rng.integers(1, min(n_ids, 6) + 1))
        own = rng.integers(0, nA, n_ids)
        own[0] = 0
        out.append((own.tolist(), [True] + [bool(x) for x in (rng.random(nA - 1) >= undefined)]))
    return out


def two_halves(rng, A):
    """two chains of disjoint presence plus the shared allele 0, a third that is not kept"""
    half = (A + 1) // 2
    p0 = [1] + [1 if 1 <= a < half else 0 for a in range(1, A)]
    p1 = [1] + [0 if 1 <= a < half else 1 for a in range(1, A)]
    return [(p0, rand_bins(rng, A, spread=12, zero_frac=0.05)), (p1, rand_bins(rng, A, spread=12, zero_frac=0.05)), None]


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(20261021)
    c = Chains(3)
    tag, records = {}, []

    def add(name, A, chains, recs, ids=None):
        v = c.add(name, A, chains, ids=ids)
        n_ids = max(c.ids[-A:]) + 1
        assert all(len(own) == n_ids for own, _ in recs), name
        records.append(recs)
        tag[name] = v
        return v

    big = lambda n, e=-20: [(0.75, e)] * n
    ident3 = ([0, 1, 2], [True, True, True])
    # wide bubbles of 6, 65 and 256 alleles: rows longer than a wave, the largest staging slot; records of 2 .. 6 alleles, one undefined
    add("wide 6", 6, two_halves(rng, 6), rand_records(rng, list(range(6)), 3, alleles=[2, 4, 6]) + [([0, 1, 2, 0, 1, 2], [True, False, True])])
    # the union of {0, 1} and {0, 2}: (1, 2) is no key; a record that keeps 1 and 2 apart has no likelihood for that pair
    add("union", 3, [([1, 1, 0], rand_bins(rng, 3, zero_frac=0.0)), ([1, 0, 1], rand_bins(rng, 3, zero_frac=0.0)), None],
        [ident3, ([0, 1, 1], [True, True]), ([0, 1, 2], [True, False, True])])
    # no chain holds any key: 0/0, GQ 10000, PG_CALL_EMPTY; GL 0 then -inf
    add("no key", 3, [None, None, ([0, 0, 0], big(6))], [([0, 1, 0], [True, True]), ident3])
    add("no key, wide", 7, [None, None, None], [([0, 1, 0, 1, 0, 1, 0], [True, True])])
    # every held value 0
    add("all zero", 3, [([1, 1, 1], [(0.0, 0)] * 6), ([1, 1, 0], [(0.0, 0)] * 6), None], [([0, 1, 0], [True, True]), ident3])
    add("all zero, wide", 6, [([1] * 6, [(0.0, 0)] * 21), None, ([1] * 6, [(0.0, 0)] * 21)], [([0, 1, 0, 1, 0, 1], [True, True])])
    # one deferred key among large ones: every record and value of that variant, not its neighbours
    add("before the deferred", 2, [([1, 1], big(3)), ([1, 1], big(3, -16290)), None], [([0, 1], [True, True])])
    add("deferred", 3, [([1, 1, 1], big(3) + [(0.75, -16320)] + big(2)), ([1, 1, 1], big(3, -22) + [(0.5, -16400)] + big(2, -25)), None],
        [([0, 1, 0], [True, True]), ident3, ([0, 1, 2], [True, False, True])])
    add("behind the deferred", 2, [([1, 1], big(3)), ([1, 1], big(3, -16299)), None], [([0, 1], [True, True])])
    add("deferred, wide", 6, [([1] * 6, big(20) + [(0.75, -16310)]), ([1] * 6, big(20) + [(0.5, -16400)]), None],
        [([0, 1, 0, 1, 0, 1], [True, True]), ([0, 1, 2, 0, 1, 2], [True, True, False])])
    # the order example of pg_combine.h on key (0,0), (mid + tiny) + large = large, carried through to a record
    add("mid tiny large", 2, [([1, 1], [(0.5, -16363), (0.5, -16297), (0.5, -16298)]), ([1, 1], [(0.5 + 2.0 ** -21, -16427), (0.5, -16289), (0.5, -16296)]),
                              ([1, 1], [(0.5, -16299), (0.5, -16298), (0.5, -16295)])], [([0, 1], [True, True]), ([0, 0], [True])])
    # a tie within 1e-10 that exists only on the folded map: F(0,0) = 1/4 + 3/16 + 1/16 = F(0,1) = 3/8 + 1/8, each chain holds half
    tie = [fr(0.25, -1), fr(0.375, -1), fr(0.1875, -1), (0.0, 0), fr(0.125, -1), fr(0.0625, -1)]
    add("tie on the fold", 3, [([1, 1, 1], tie), None, ([1, 1, 1], tie)], [([0, 1, 0], [True, True]), ident3])
    tie6 = {(0, 0): tie[0], (0, 1): tie[1], (0, 2): tie[2], (1, 2): tie[4], (2, 2): tie[5]}
    add("tie on the fold, wide", 6, [([1] * 6, [tie6.get((a, b), (0.0, 0)) for a in range(6) for b in range(a, 6)]), None,
                                     ([1] * 6, [tie6.get((a, b), (0.0, 0)) for a in range(6) for b in range(a, 6)])],
        [([0, 1, 0, 0, 0, 0], [True, True])])
    # a quality of 10000 from evidence: one key holds everything
    add("certain", 3, [([1, 1, 1], [(0.0, 0)] * 3 + [fr(0.5)] + [(0.0, 0)] * 2), ([1, 1, 0], [(0.0, 0)] * 3 + [fr(0.25)] + [(0.0, 0)] * 2), None],
        [ident3, ([0, 1, 1], [True, True])])
    # a variant that is a kept column in one chain only
    add("one chain's column", 3, [None, ([1, 1, 1], rand_bins(rng, 3, zero_frac=0.0)), None], rand_records(rng, [3, 9, 27], 2), ids=[3, 9, 27])
    add("wide 65", 65, two_halves(rng, 65), rand_records(rng, list(range(65)), 3, alleles=[2, 3, 5]) + [([0] + [1 + a % 3 for a in range(64)], [True, True, False, True])])
    # many more: several blocks of records, both sides of the narrow / wide split
    for i in range(260):
        A = int(rng.integers(1, 6)) if rng.random() > 0.05 else int(rng.integers(6, 13))
        base, spread = -int(rng.integers(0, 12000)), (1, 8, 70, 130)[int(rng.integers(0, 4))]
        ids = [0] + np.sort(rng.choice(np.arange(1, 40), A - 1, replace=False)).tolist()
        add(f"random #{i}", A, [rand_chain(rng, A, base=base, spread=spread) for _ in range(3)], rand_records(rng, ids, int(rng.integers(1, 4))), ids=ids)
    add("wide 256", 256, two_halves(rng, 256), rand_records(rng, list(range(256)), 2, alleles=[2, 6]) + [([0] + [1 + a % 4 for a in range(255)], [True, True, True, False, True])])
    plan = calls.RecordPlan.from_records(records)
    assert plan.n_records > 512 and plan.n_records % 64 != 0
    ids = np.array(c.ids, np.uint16)
    arrays = c.arrays()
    bins = calls.combine_bins(*arrays)
    want, deferred = combined_yardstick(arrays[0], ids, *arrays[1:])
    calls_want, gl_want = records_yardstick(plan, want)
    rec = calls.record_calls_from_combined(arrays[0], ids, bins, plan)
    gl = calls.record_gl_from_combined(arrays[0], ids, bins, plan)
    return dict(c=c, tag=tag, ids=ids, arrays=arrays, plan=plan, bins=bins, deferred=deferred, calls_want=calls_want, gl_want=gl_want, rec=rec, gl=gl)


def test_every_record_says_what_the_long_double_route_says(case):
    plan, rec = case["plan"], case["rec"]
    was_deferred = assert_record_calls(rec, case["calls_want"], "edges")
    expect = records_of(plan, [v for v in range(plan.n_variants) if case["deferred"][v]])
    assert sorted(was_deferred) == expect and len(expect) == 5
    A = np.diff(case["arrays"][0].astype(np.int64))
    per = np.diff(plan.rec_off.astype(np.int64))
    ok = np.array([w is not None for w in case["calls_want"]])
    wide_rec = np.repeat(A > 5, per)
    assert ok[~wide_rec].sum() > 300 and ok[wide_rec].sum() > 20 and (~ok).sum() > 5


def test_every_gl_value_prints_what_the_long_double_route_prints(case):
    plan, gl = case["plan"], case["gl"]
    gl_off = calls.record_gl_offsets(plan)
    was_deferred = assert_record_gl(gl, gl_off, case["gl_want"], "edges")
    expect = [i for r in records_of(plan, [v for v in range(plan.n_variants) if case["deferred"][v]]) for i in range(int(gl_off[r]), int(gl_off[r + 1]))]
    assert was_deferred == expect   # (the window rule defers about 2e-9 of the values: none of these)
    assert len(gl) > 2000


def test_the_constructions_hit_what_they_aim_at(case):
    """the expected fields of the edges that have a closed form, stated, so that a construction that silently misses its edge does not pass"""
    tag, plan, rec, gl = case["tag"], case["plan"], case["rec"], case["gl"]
    gl_off = calls.record_gl_offsets(plan).astype(np.int64)
    r0 = lambda name: int(plan.rec_off[tag[name]])
    fields = lambda r: (int(rec[r]["flags"]), int(rec[r]["allele_1"]), int(rec[r]["allele_2"]), int(rec[r]["gq"]))
    texts = lambda r: list(texts_of_values(gl[gl_off[r]:gl_off[r + 1]]))
    P = calls.PG_COMBINED_PRESENT
    goff = np.concatenate([[0], np.cumsum(np.diff(case["arrays"][0].astype(np.int64)) * (np.diff(case["arrays"][0].astype(np.int64)) + 1) // 2)])
    union = case["bins"][goff[tag["union"]]:goff[tag["union"] + 1]]
    assert [int(f) for f in union["flags"]] == [P, P, P, P, 0, P]
    t = texts(r0("union"))
    assert len(t) == 6 and t[4] == "-inf" and "-inf" not in t[:4] + t[5:]       # 1/2 has no likelihood, every other pair has one
    assert "-inf" not in texts(r0("union") + 1)                                    # 1 and 2 onto one allele: nothing is missing
    for name in ("no key", "no key, wide"):
        assert fields(r0(name)) == (OK | EMPTY, 0, 0, 10000), name
        t = texts(r0(name))
        assert t[0] == "0" and set(t[1:]) == {"-inf"}, name
    for name in ("all zero", "all zero, wide"):
        assert fields(r0(name)) == (NONE, 0xFFFF, 0xFFFF, 0) and set(texts(r0(name))) == {"-inf"}, name
    for name, n in (("deferred", 3), ("deferred, wide", 2)):
        for r in range(r0(name), r0(name) + n):
            assert fields(r)[0] == DEFERRED and is_deferred(gl[gl_off[r]:gl_off[r + 1]]).all(), (name, r)
    for name in ("before the deferred", "behind the deferred"):
        assert fields(r0(name))[0] != DEFERRED and not is_deferred(gl[gl_off[r0(name)]:gl_off[r0(name) + 1]]).any(), name
    mtl = case["bins"][goff[tag["mid tiny large"]]]
    assert int(mtl["flags"]) == P and calls.combined_to_longdouble(np.array([mtl]))[0] == np.longdouble(2.0) ** -16300
    assert fields(r0("mid tiny large"))[0] == OK and fields(r0("mid tiny large") + 1) == (OK, 0, 0, 10000)
    assert fields(r0("tie on the fold"))[0] == NOT_UNIQUE and fields(r0("tie on the fold") + 1)[0] == OK
    assert fields(r0("tie on the fold, wide"))[0] == NOT_UNIQUE
    assert texts(r0("tie on the fold"))[:2] == ["-0.301", "-0.301"]
    assert fields(r0("certain")) == (OK, 1, 1, 10000) and fields(r0("certain") + 1) == (OK, 1, 1, 10000)
    assert texts(r0("certain")) == ["-inf", "-inf", "0", "-inf", "-inf", "-inf"]
    assert fields(r0("one chain's column"))[0] in (OK, NOT_UNIQUE)
    assert tag["wide 6"] == 0 and tag["wide 256"] == plan.n_variants - 1
    for name in ("wide 6", "wide 65", "wide 256"):   # both halves and the shared allele reach the records: calls with evidence
        n = int(plan.rec_off[tag[name] + 1]) - r0(name)
        assert n >= 3 and all(fields(r)[0] in (OK, NOT_UNIQUE) for r in range(r0(name), r0(name) + n)), name
        assert (plan.record(r0(name) + n - 1)[1] == 0xFFFF).any(), name


def test_a_group_of_one_chain_is_that_chain(case):
    """the combined bins of ONE chain through the new kernels against pg_record_calls_from_bins / pg_record_gl_from_bins, byte for byte"""
    c, ids, plan = case["c"], case["ids"], case["plan"]
    for s in (0, 1):
        aoff, kept, pres, lik, lik_exp = c.arrays(order=[s])
        bins = calls.combine_bins(aoff, kept, pres, lik, lik_exp)
        rec = calls.record_calls_from_combined(aoff, ids, bins, plan)
        gl = calls.record_gl_from_combined(aoff, ids, bins, plan)
        direct = calls.record_calls_from_bins(aoff, ids, kept[0], pres[0], lik[0], lik_exp[0], plan)
        direct_gl = calls.record_gl_from_bins(aoff, ids, kept[0], pres[0], lik[0], lik_exp[0], plan)
        # (a chain alone defers a variant by its largest bin, the combined route by any key below the cut: the constructed deferred
        # bubbles aside, the bytes are the same)
        skip = set(records_of(plan, [case["tag"][n] for n in ("deferred", "deferred, wide", "mid tiny large", "before the deferred", "behind the deferred")]))
        keep = np.array([r not in skip for r in range(plan.n_records)])
        assert rec[keep].tobytes() == direct[keep].tobytes(), s
        gl_off = calls.record_gl_offsets(plan).astype(np.int64)
        keep_gl = np.repeat(keep, np.diff(gl_off))
        assert gl[keep_gl].tobytes() == direct_gl[keep_gl].tobytes(), s


def test_argument_checks_and_the_empty_call():
    empty = calls.RecordPlan.from_records([])
    assert len(calls.record_calls_from_combined(np.zeros(1, np.uint32), [], np.zeros(0, calls.COMBINED_DTYPE), empty)) == 0
    assert len(calls.record_gl_from_combined(np.zeros(1, np.uint32), [], np.zeros(0, calls.COMBINED_DTYPE), empty)) == 0
    with pytest.raises(ValueError):
        calls.record_calls_from_combined(np.array([0, 2], np.uint32), [0, 1], np.zeros(2, calls.COMBINED_DTYPE), empty)   # three bins belong to two alleles
