"""Calls per VCF record on the device, edge by edge (k_rcalls / k_rcalls_wide of pangenie_amd/csrc/pg_calls.hip through
pg_record_calls_from_bins): constructed bubbles whose records' calls hang on what the fold onto the record's alleles does —
ties it creates and resolves, sums that exist only after it, the order of the additions onto one key — on undefined alleles,
empty maps, allele ids that are not slots, the narrow / wide split and the deferral cut.  Every construction whose sum is
exactly 1 has quotients that ARE its bins; each is run on both kernels (the wide form: three more alleles, present, all their
bins zero).  ONE launch over all bubbles (more than two blocks of records, a ragged last wave, a wide bubble first and last);
the yardstick is pangenie_amd/genotyping_result.py on the same bins (tests/record_calls_util.py), computed once."""
import numpy as np
import pytest

from pangenie_amd import calls
from tests.calls_util import DEFERRED, NONE, NOT_UNIQUE, OK
from tests.record_calls_util import EMPTY, assert_record_calls, record_yardstick
from tests.test_calls_edges_gpu import Bins, fr, rand_bins

pytestmark = pytest.mark.gpu

U = 2.0 ** -64   # one unit in the last place of a long double in [1/2, 1)


class Bubbles(Bins):
    def __init__(self):
        super().__init__()
        self.records, self.first = [], []

    def add(self, name, bins, records=None, **kw):
        """records: per record (own by allele ID, defined per record allele); None: one record, identity map, all defined"""
        v = super().add(name, bins, **kw)
        A = self.aoff[-1] - self.aoff[-2]
        n_ids = max(self.ids[-A:]) + 1
        if records is None:
            records = [(list(range(n_ids)), [True] * n_ids)]
        for own, defined in records:
            assert len(own) == n_ids, (name, len(own), n_ids)
        self.first.append(sum(len(r) for r in self.records))
        self.records.append(records)
        return v

    def plan(self):
        return calls.RecordPlan.from_records(self.records)


def widen(bins3, own, zero_onto=0):
    """a three-allele construction as a six-allele bubble for k_rcalls_wide: alleles 3 .. 5 are present, their bins zero"""
    at = {}
    k = 0
    for a in range(3):
        for b in range(a, 3):
            at[(a, b)] = bins3[k]
            k += 1
    bins6 = [at.get((a, b), (0.0, 0)) for a in range(6) for b in range(a, 6)]
    return bins6, list(own) + [zero_onto] * 3


def rand_records(rng, ids, n, undefined=0.15):
    n_ids = max(ids) + 1
    out = []
    for _ in range(n):
        nA = int(rng.integers(1, min(n_ids, 6) + 1))
        own = rng.integers(0, nA, n_ids)
        own[0] = 0
        out.append((own.tolist(), [True] + [bool(x) for x in (rng.random(nA - 1) >= undefined)]))
    return out


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(20261019)
    b = Bubbles()
    tag = {}

    def both(name, bins3, own, defined, **kw):
        """the construction on k_rcalls and, widened, on k_rcalls_wide"""
        tag[name] = b.add(name, bins3, [(own, defined)], **kw)
        bins6, own6 = widen(bins3, own)
        if "present" in kw:
            kw = dict(kw, present=list(kw["present"]) + [1, 1, 1])
        tag[name + "_wide"] = b.add(name + " wide", bins6, [(own6, defined)], **kw)

    # a wide bubble first
    ids = list(range(7))
    tag["wide_first"] = b.add("wide first", rand_bins(rng, 7, zero_frac=0.0), rand_records(rng, ids, 2))
    # single records with the identity map: what calls_from_bins says about the bubble
    tag["identity"] = []
    for A in (1, 2, 3, 4, 5, 6, 9):
        for rep in range(5):
            tag["identity"].append(b.add(f"identity A={A} #{rep}", rand_bins(rng, A, base=-int(rng.integers(0, 3000)), spread=int(rng.choice([2, 30, 90])))))
    tag["identity"].append(b.add("identity, not kept", [fr(0.9), fr(0.05), fr(0.05)], kept=0))
    tag["identity"].append(b.add("identity, ids are not slots", rand_bins(rng, 4, zero_frac=0.0), ids=[0, 3, 4, 9], present=[1, 1, 0, 1]))
    # 2, 3 and 4 records over 2 .. 5 alleles; wide bubbles of 6 .. 12 alleles
    for A in (2, 3, 4, 5, 6, 8, 12):
        for n in (2, 3, 4):
            for rep in range(3):
                ids = np.sort(rng.choice(np.arange(1, 40), A - 1, replace=False)).tolist()
                b.add(f"A={A}, {n} records #{rep}", rand_bins(rng, A, base=-int(rng.integers(0, 9000)), spread=int(rng.choice([2, 8, 70, 200]))),
                      rand_records(rng, [0] + ids, n), ids=[0] + ids, present=[int(x) for x in (rng.random(A) < 0.85)])
    # more alleles than lanes, three records, one with more keys than lanes
    ids70 = list(range(5, 75))
    n70 = 75
    r70 = []
    for nA in (3, 7, 40):
        own = rng.integers(0, nA, n70)
        own[0] = 0
        r70.append((own.tolist(), [True] + [bool(x) for x in (rng.random(nA - 1) >= 0.2)]))
    tag["A70"] = b.add("A=70, three records", rand_bins(rng, 70, spread=12), r70, ids=ids70, present=[int(x) for x in (rng.random(70) < 0.8)])
    # empty maps: 0/0, GQ 10000, PG_CALL_EMPTY
    tie_maker = [fr(0.25), fr(0.375), fr(0.1875), (0.0, 0), fr(0.125), fr(0.0625)]
    both("not_kept", tie_maker, [0, 1, 0], [True, True], kept=0)
    both("no_present", tie_maker, [0, 1, 1], [True, False], present=[0, 0, 0])
    tag["no_present_wide"] = b.add("no present allele, wide", rand_bins(rng, 6), [([0, 1, 1, 0, 1, 0], [True, False])], present=[0] * 6)
    both("all_zero", [(0.0, 0)] * 6, [0, 1, 0], [True, True])
    # the fold creates a tie: F(0,0) = 1/4 + 3/16 + 1/16 = F(0,1) = 3/8 + 1/8, no two bins of the bubble within 1/16
    both("tie_created", tie_maker, [0, 1, 0], [True, True])
    # ... resolves one: the bubble's (1,1) and (1,2) are equal maxima, both are 1/1 of the record
    both("tie_resolved", [fr(0.25), (0.0, 0), (0.0, 0), fr(0.375), fr(0.375), (0.0, 0)], [0, 1, 1], [True, True])
    # the likeliest folded genotype 0/1 holds the undefined allele 1: 2/2 with 1/4 of the defined 1/2 is GT 1/1, GQ 3
    both("undefined_best", [fr(0.125), fr(0.5), fr(0.125), (0.0, 0), (0.0, 0), fr(0.25)], [0, 1, 2], [True, False, True])
    both("defined_all_zero", [(0.0, 0), fr(0.5), (0.0, 0), fr(0.5), (0.0, 0), (0.0, 0)], [0, 1, 2], [True, False, True])
    # best = 1 - m 2^-64 only as the sum of two bins: (1 - 2^-53) + (2048 - m) 2^-64; the third key m 2^-64 makes the sum 1
    for m in range(5):
        both(f"top{m}", [fr(1.0 - 2.0 ** -53), fr((2048.0 - m) * U), (0.0, 0), (0.0, 0), (0.0, 0), fr(m * U) if m else (0.0, 0)], [0, 0, 1], [True, True])
    # three quotients onto one key: (q1 + q2) + q3 = 1 - 2u (a tie to even, then a sticky quarter unit) but (q2 + q3) + q1 = 1 - u
    q1, q2, q3 = fr(1.0 - 2.0 ** -53), fr(2046.5 * U), fr(0.25 * U)
    both("order_123", [q1, q2, (0.0, 0), q3, (0.0, 0), fr(2 * U)], [0, 0, 1], [True, True])
    both("order_231", [q2, q3, (0.0, 0), q1, (0.0, 0), fr(2 * U)], [0, 0, 1], [True, True])
    # a runner-up at best - 1e-10 (1 -+ 2^-20) after the fold: best = 2 x 0.25 (1 + t), runner-up 0.5 (1 - t)
    for name, sign in (("tie_inside", -1.0), ("tie_outside", 1.0)):
        t = 1e-10 * (1.0 + sign * 2.0 ** -20)
        both(name, [fr(0.25 * (1.0 + t), -700), (0.0, 0), fr(0.25 * (1.0 + t), -700), fr(0.5 * (1.0 - t), -700), (0.0, 0), (0.0, 0)], [0, 1, 0], [True, True])
    # allele ids that are not slots, an absent allele in the middle, an undefined record allele: 1/1 with 1/4 of 1/2
    nine = (0.9, 3)
    tag["ids_not_slots"] = b.add("ids are not slots", [fr(0.125), nine, fr(0.125), (0.0, 0), nine, nine, nine, fr(0.25), fr(0.5), (0.0, 0)],
                                 [([0, 9, 1, 9, 9, 1, 9, 2], [True, True, False] + [True] * 7)], ids=[0, 2, 5, 7], present=[1, 0, 1, 1])
    # both sides of 2^-16300: every record of the bubble below it is deferred
    rec3 = [([0, 1, 0], [True, True]), ([0, 1, 1], [True, False]), ([0, 1, 2], [True, True, True])]
    tag["deferred"] = b.add("largest bin below 2^-16300", [(0.5, -16310), (0.75, -16300), (0.5, -16400), (0.5, -16330), (0.5, -16305), (0.5, -16302)], rec3)
    tag["deferred_wide"] = b.add("largest bin below 2^-16300, wide", [(0.5, -16320)] * 20 + [(0.99, -16300)], rand_records(rng, list(range(6)), 2))
    tag["decided_edge"] = b.add("largest bin at 2^-16300", [(0.5, -16310), (0.5, -16299), (0.5, -16400), (0.5, -16330), (0.5, -16305), (0.5, -16302)], rec3)
    tag["decided_edge_wide"] = b.add("largest bin just above 2^-16300, wide", [(0.5, -16320)] * 20 + [(0.51, -16299)], rand_records(rng, list(range(6)), 2))
    # many more, so that the launch has several blocks of records
    for i in range(230):
        A = int(rng.integers(1, 6)) if rng.random() > 0.06 else int(rng.integers(6, 13))
        ids = [0] + np.sort(rng.choice(np.arange(1, 200), A - 1, replace=False)).tolist()
        style = int(rng.integers(0, 4))
        b.add(f"random #{i}", rand_bins(rng, A, base=-int(rng.integers(0, 12000)), spread=(1, 8, 70, 200)[style]),
              rand_records(rng, ids, int(rng.integers(1, 4))), kept=int(rng.random() < 0.95), present=[int(x) for x in (rng.random(A) < 0.85)], ids=ids)
    # a wide bubble last
    tag["wide_last"] = b.add("wide last", rand_bins(rng, 6, zero_frac=0.0), rand_records(rng, list(range(6)), 3))
    arrays, plan = b.arrays(), b.plan()
    assert plan.n_records % 64 != 0 and plan.n_records > 512
    got = calls.record_calls_from_bins(*arrays, plan)
    want = record_yardstick(*arrays, plan)
    bubble_calls = calls.calls_from_bins(*arrays)
    return b, tag, arrays, plan, got, want, bubble_calls


def records_of(b, v):
    return range(b.first[v], b.first[v] + len(b.records[v]))


def test_every_record_agrees_with_the_long_double_host_route(case):
    b, tag, arrays, plan, got, want, _ = case
    deferred = assert_record_calls(got, want, "edges")
    # deferred where constructed, every record of the bubble, and nowhere else
    assert deferred == [r for name in ("deferred", "deferred_wide") for r in records_of(b, tag[name])], deferred
    # the comparison is not empty-handed: calls, no-calls, both kernels, records with undefined alleles
    A = np.diff(arrays[0].astype(np.int64))
    wide = np.repeat(A > 5, np.diff(plan.rec_off.astype(np.int64)))
    ok = np.array([w is not None for w in want])
    assert ok[~wide].sum() > 300 and ok[wide].sum() > 40 and (~ok).sum() > 20
    undefined = np.array([(plan.record(r)[1] == 0xFFFF).any() for r in range(plan.n_records)])
    assert (ok & undefined).sum() > 40
    gq = np.array([w[2] if w else -1 for w in want])
    assert (gq == 10000).any() and ((gq > 100) & (gq <= 192)).any() and ((gq >= 0) & (gq < 10)).any()


def test_a_single_record_with_the_identity_map_is_the_bubbles_call(case):
    b, tag, arrays, plan, got, want, bubble_calls = case
    for v in tag["identity"]:
        (r,) = records_of(b, v)
        rec, bub = got[r], bubble_calls[v]
        if int(rec["flags"]) & EMPTY:   # the VCF prints 0/0 for a bubble without likelihoods; the bubble's own call is "none"
            assert int(bub["flags"]) == NONE and (int(rec["allele_1"]), int(rec["allele_2"]), int(rec["gq"]), int(rec["flags"])) == (0, 0, 10000, OK | EMPTY)
        else:
            assert rec == bub, (b.names[v], rec, bub)
    assert sum(int(got[records_of(b, v)[0]]["flags"]) == OK for v in tag["identity"]) > 20


def test_the_constructions_hit_what_they_aim_at(case):
    """the expected values of the edges that have a closed form, stated — so that a construction that silently misses its edge
    (and a yardstick and a kernel that agree on something easier) does not pass"""
    b, tag, arrays, plan, got, want, bubble_calls = case

    def rec(name, i=0):
        r = got[b.first[tag[name]] + i]
        return (int(r["allele_1"]), int(r["allele_2"]), int(r["gq"]), int(r["flags"]))

    expect = [10000] + [int(-10 * np.log10(np.longdouble(m) * np.longdouble(2.0) ** -64)) for m in range(1, 5)]
    assert expect == [10000, 192, 189, 187, 186]
    for s in ("", "_wide"):
        assert rec("not_kept" + s) == (0, 0, 10000, OK | EMPTY) and rec("no_present" + s) == (0, 0, 10000, OK | EMPTY)
        assert rec("all_zero" + s)[3] == NONE
        # the bubble itself has a unique likeliest genotype; its record does not — and the other way round
        assert int(bubble_calls[tag["tie_created" + s]]["flags"]) == OK and rec("tie_created" + s)[3] == NOT_UNIQUE
        assert int(bubble_calls[tag["tie_resolved" + s]]["flags"]) == NOT_UNIQUE and rec("tie_resolved" + s) == (1, 1, 6, OK)
        assert rec("undefined_best" + s) == (1, 1, 3, OK)
        assert rec("defined_all_zero" + s)[3] == NONE
        for m in range(5):
            assert rec(f"top{m}{s}") == (0, 0, expect[m], OK), (m, s, rec(f"top{m}{s}"))
            assert want[b.first[tag[f"top{m}{s}"]]][:3] == (0, 0, expect[m])
        assert rec("order_123" + s) == (0, 0, 189, OK) and rec("order_231" + s) == (0, 0, 192, OK)
        assert want[b.first[tag["tie_inside" + s]]] is None and rec("tie_inside" + s)[3] == NOT_UNIQUE
        assert want[b.first[tag["tie_outside" + s]]] is not None and rec("tie_outside" + s) == (0, 0, 3, OK)
        assert all(rec("deferred" + s, i)[3] == DEFERRED for i in range(len(b.records[tag["deferred" + s]])))
        assert all(rec("decided_edge" + s, i)[3] != DEFERRED for i in range(len(b.records[tag["decided_edge" + s]])))
    assert rec("ids_not_slots") == (1, 1, 3, OK)
    assert tag["wide_first"] == 0 and tag["wide_last"] == len(b.names) - 1
    assert all(int(got[r]["flags"]) & 0xFF in (OK, NOT_UNIQUE) for v in (0, len(b.names) - 1) for r in records_of(b, v))
    assert len(b.records[tag["A70"]]) == 3 and all(rec("A70", i)[3] & 0xFF in (OK, NOT_UNIQUE, NONE) for i in range(3))


def test_argument_checks_and_the_empty_call():
    empty = calls.RecordPlan([0], [0], [], [], [0], [])
    assert len(calls.record_calls_from_bins(np.zeros(1, np.uint32), [], [], [], [], [], empty)) == 0
    with pytest.raises(ValueError):
        calls.record_calls_from_bins(np.array([0, 2], np.uint32), [0, 1], [1], [1, 1], [0.5], [0], empty)   # three bins belong to two alleles
