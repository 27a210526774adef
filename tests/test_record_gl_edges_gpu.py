"""The GL column per VCF record on the device, edge by edge (k_rgl / k_rgl_wide of pangenie_amd/csrc/pg_calls.hip through
pg_record_gl_from_bins): constructed bubbles whose records' values hang on what the fold onto the record's alleles does —
absent keys, zero bins, sums next to 1 and above it, undefined alleles, empty maps, allele ids that are not slots, the narrow /
wide split and the deferral cut.  Each construction is run on both kernels (the wide form of tests/test_record_calls_edges_gpu.py:
three more alleles, present, all their bins zero).  ONE launch over all bubbles (more than two blocks of records, a ragged last
wave, a wide bubble first and last); the yardstick is pangenie_amd/genotyping_result.py on the same bins with exact long double
formatting (tests/record_gl_util.py), computed once."""
import numpy as np
import pytest

from pangenie_amd import calls
from tests.record_gl_util import assert_record_gl, is_deferred, record_gl_yardstick, text_of_log, texts_of_values
from tests.test_calls_edges_gpu import fr, rand_bins
from tests.test_record_calls_edges_gpu import Bubbles, rand_records, widen

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -64   # one unit in the last place of a long double in [1/2, 1)
# five quotients whose rounded sum onto one key is 1 + 2^-63 (found by tests/cpp/test_gl_arith.cpp's search)
ABOVE_ONE = [(float.fromhex("0x1.25b31ae2e211ep-1"), -1), (float.fromhex("0x1.340170994a66fp-1"), -4), (float.fromhex("0x1.d5d2292d154f2p-1"), 0),
             (float.fromhex("0x1.b89769fe0cfd3p-1"), 0), (float.fromhex("0x1.f297f7368e762p-1"), -5), (0.0, 0)]


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(20261022)
    b = Bubbles()
    tag = {}

    def both(name, bins3, own, defined, **kw):
        """the construction on k_rgl and, widened, on k_rgl_wide"""
        tag[name] = b.add(name, bins3, [(own, defined)], **kw)
        bins6, own6 = widen(bins3, own)
        if "present" in kw:
            kw = dict(kw, present=list(kw["present"]) + [1, 1, 1])
        tag[name + "_wide"] = b.add(name + " wide", bins6, [(own6, defined)], **kw)

    # a wide bubble first
    tag["wide_first"] = b.add("wide first", rand_bins(rng, 7, zero_frac=0.0), rand_records(rng, list(range(7)), 2))
    # identity records: the bubble's own normalised likelihoods
    tag["identity"] = []
    for A in (1, 2, 3, 4, 5, 6, 9):
        for rep in range(4):
            tag["identity"].append(b.add(f"identity A={A} #{rep}", rand_bins(rng, A, base=-int(rng.integers(0, 3000)), spread=int(rng.choice([2, 30, 90])))))
    # 2, 3 and 4 records over 2 .. 5 alleles; wide bubbles of 6 .. 12 alleles
    for A in (2, 3, 4, 5, 6, 8, 12):
        for n in (2, 3, 4):
            for rep in range(2):
                ids = np.sort(rng.choice(np.arange(1, 40), A - 1, replace=False)).tolist()
                b.add(f"A={A}, {n} records #{rep}", rand_bins(rng, A, base=-int(rng.integers(0, 9000)), spread=int(rng.choice([2, 8, 70, 200]))),
                      rand_records(rng, [0] + ids, n), ids=[0] + ids, present=[int(x) for x in (rng.random(A) < 0.85)])
    # more alleles than lanes, three records, one with more keys than lanes
    r70 = []
    for nA in (3, 7, 40):
        own = rng.integers(0, nA, 75)
        own[0] = 0
        r70.append((own.tolist(), [True] + [bool(x) for x in (rng.random(nA - 1) >= 0.2)]))
    tag["A70"] = b.add("A=70, three records", rand_bins(rng, 70, spread=12), r70, ids=list(range(5, 75)), present=[int(x) for x in (rng.random(70) < 0.8)])
    six = [fr(0.25), fr(0.375), fr(0.1875), (0.0, 0), fr(0.125), fr(0.0625)]
    # a single key: "0", the rest "-inf"
    both("single_key", [fr(0.7, -300)] + [fr(0.5)] * 5, [0, 1, 2], [True, True, True], present=[1, 0, 0])
    # an absent key (nothing folds onto 2/2 or 0/2) and a zero bin among the keys
    both("absent_key", six, [0, 1, 1], [True, True, True])
    # empty maps: F[(0,0)] = 1
    both("not_kept", six, [0, 1, 0], [True, True], kept=0)
    both("no_present", six, [0, 1, 2], [True, False, True], present=[0, 0, 0])
    tag["no_present_wide"] = b.add("no present allele, wide", rand_bins(rng, 6), [([0, 1, 2, 0, 1, 0], [True, False, True])], present=[0] * 6)
    both("all_zero", [(0.0, 0)] * 6, [0, 1, 0], [True, True])
    # logarithms of every magnitude up to the cut: exp10 1, 2 and 3
    both("deep", [fr(0.5), (0.5, -400), (0.5, -4000), (0.5, -16000), (0.0, 0), (0.0, 0)], [0, 1, 2], [True, True, True])
    # the best value 1 - m 2^-64 only as the sum of two bins
    for m in range(1, 5):
        both(f"top{m}", [fr(1.0 - 2.0 ** -53), fr((2048.0 - m) * U), (0.0, 0), (0.0, 0), (0.0, 0), fr(m * U)], [0, 0, 1], [True, True])
    # a fold whose rounded sum is 1 + 2^-63: a positive logarithm
    both("above_one", ABOVE_ONE, [0, 0, 0], [True])
    # undefined alleles: the defined keys all zero; the likeliest genotype over the undefined allele
    both("defined_all_zero", [(0.0, 0), fr(0.5), (0.0, 0), fr(0.5), (0.0, 0), (0.0, 0)], [0, 1, 2], [True, False, True])
    both("undefined_best", [fr(0.125), fr(0.5), fr(0.125), (0.0, 0), (0.0, 0), fr(0.25)], [0, 1, 2], [True, False, True])
    # allele ids that are not slots, an absent allele in the middle, an undefined record allele
    nine = (0.9, 3)
    tag["ids_not_slots"] = b.add("ids are not slots", [fr(0.125), nine, fr(0.125), (0.0, 0), nine, nine, nine, fr(0.25), fr(0.5), (0.0, 0)],
                                 [([0, 9, 1, 9, 9, 1, 9, 2], [True, True, False] + [True] * 7)], ids=[0, 2, 5, 7], present=[1, 0, 1, 1])
    # both sides of 2^-16300: every value of the bubble below it is deferred; so is a folded value below it
    rec3 = [([0, 1, 0], [True, True]), ([0, 1, 1], [True, False]), ([0, 1, 2], [True, True, True])]
    tag["deferred"] = b.add("largest bin below 2^-16300", [(0.5, -16310), (0.75, -16300), (0.5, -16400), (0.5, -16330), (0.5, -16305), (0.5, -16302)], rec3)
    tag["deferred_wide"] = b.add("largest bin below 2^-16300, wide", [(0.5, -16320)] * 20 + [(0.99, -16300)], rand_records(rng, list(range(6)), 2))
    tag["decided_edge"] = b.add("largest bin at 2^-16300", [(0.5, -16299)] * 6, rec3)
    tag["decided_edge_wide"] = b.add("largest bin just above 2^-16300, wide", [(0.5, -16299)] * 21, rand_records(rng, list(range(6)), 2))
    both("tiny_fold", [fr(0.5), (0.5, -16350), (0.0, 0), (0.0, 0), (0.0, 0), (0.0, 0)], [0, 1, 2], [True, True, True])
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
    gl_off = calls.record_gl_offsets(plan).astype(np.int64)
    got = calls.record_gl_from_bins(*arrays, plan)
    want = record_gl_yardstick(*arrays, plan)
    return b, tag, arrays, plan, gl_off, got, want


def records_of(b, v):
    return range(b.first[v], b.first[v] + len(b.records[v]))


def test_every_value_agrees_with_the_long_double_host_route(case):
    b, tag, arrays, plan, gl_off, got, want = case
    deferred = assert_record_gl(got, gl_off, want, "edges")
    # deferred where constructed — every value of a bubble below the cut, the one folded value below it — and nowhere else
    expect = [i for name in ("deferred", "deferred_wide") for r in records_of(b, tag[name]) for i in range(gl_off[r], gl_off[r + 1])]
    expect += [int(gl_off[b.first[tag[name]]]) + 1 for name in ("tiny_fold", "tiny_fold_wide")]
    assert deferred == sorted(expect), (deferred, expect)
    # the comparison is not empty-handed: finite values and -inf on both kernels, records with undefined alleles
    A = np.diff(arrays[0].astype(np.int64))
    wide = np.repeat(np.repeat(A > 5, np.diff(plan.rec_off.astype(np.int64))), np.diff(gl_off))
    finite = got["mant"] != 0
    assert finite[~wide].sum() > 1000 and finite[wide].sum() > 300 and (~finite & ~is_deferred(got))[wide].sum() > 50
    undefined = np.array([(plan.record(r)[1] == 0xFFFF).any() for r in range(plan.n_records)])
    assert finite[np.repeat(undefined, np.diff(gl_off))].sum() > 100
    assert set(np.unique(got["exp10"][finite]).tolist()) >= {-1, 0, 1, 2, 3}


def test_an_identity_record_holds_the_bubbles_normalised_likelihoods(case):
    b, tag, arrays, plan, gl_off, got, want = case
    aoff, _, kept, pres, lik, lik_exp = arrays
    n = 0
    for v in tag["identity"]:
        (r,) = records_of(b, v)
        A = int(aoff[v + 1] - aoff[v])
        assert gl_off[r + 1] - gl_off[r] == A * (A + 1) // 2
        g0 = int(sum(int(a) * (int(a) + 1) // 2 for a in np.diff(aoff[:v + 1].astype(np.int64))))
        x = np.ldexp(lik[g0:g0 + A * (A + 1) // 2].astype(LD), lik_exp[g0:g0 + A * (A + 1) // 2].astype(np.int64))
        s = LD(0)
        for t in x:
            s += t
        texts = texts_of_values(got[gl_off[r]:gl_off[r + 1]])
        k = 0
        for a in range(A):
            for c in range(a, A):
                with np.errstate(divide="ignore"):   # (every bin zero: nothing is normalised)
                    assert texts[c * (c + 1) // 2 + a] == text_of_log(np.log10(x[k] / s if s > 0 else x[k])), (b.names[v], a, c)
                k += 1
                n += 1
    assert n > 200


def test_the_constructions_hit_what_they_aim_at(case):
    """the expected texts of the edges that have a closed form, stated — so that a construction that silently misses its edge
    (and a yardstick and a kernel that agree on something easier) does not pass"""
    b, tag, arrays, plan, gl_off, got, want = case

    def texts(name, i=0):
        r = b.first[tag[name]] + i
        return texts_of_values(got[gl_off[r]:gl_off[r + 1]]).tolist()

    top = [text_of_log(np.log10(LD(1) - LD(m) * LD(2) ** -64)) for m in range(1, 5)]
    assert top[0] == "-2.354e-20" and len(set(top)) == 4
    for s in ("", "_wide"):
        assert texts("single_key" + s) == ["0"] + ["-inf"] * 5
        # F(0,0) = 1/4, F(0,1) = 3/8 + 3/16, F(1,1) = 0 + 1/8 + 1/16; nothing onto allele 2
        assert texts("absent_key" + s) == ["-0.6021", "-0.2499", "-0.727", "-inf", "-inf", "-inf"]
        assert texts("not_kept" + s) == ["0", "-inf", "-inf"] and texts("no_present" + s) == ["0", "-inf", "-inf"]
        assert texts("all_zero" + s) == ["-inf"] * 3
        for m in range(1, 5):
            assert texts(f"top{m}{s}") == [top[m - 1], "-inf", text_of_log(np.log10(LD(m) * LD(2) ** -64))], (m, s)
        assert texts("above_one" + s) == ["4.709e-20"] and want[b.first[tag["above_one" + s]]] == ["4.709e-20"]
        assert texts("defined_all_zero" + s) == ["-inf"] * 3
        # 0/0 1/8 and 2/2 1/4 of the defined 1/2 (0/2 1/8): log10 of 1/4, 1/4, 1/2
        assert texts("undefined_best" + s) == ["-0.6021", "-0.6021", "-0.301"]
        assert texts("deep" + s) == ["0", "-120.4", "-4816", "-1204", "-inf", "-inf"]
        assert texts("tiny_fold" + s) == ["0", None, "-inf", "-inf", "-inf", "-inf"]
        assert all(t is None for i in range(len(b.records[tag["deferred" + s]])) for t in texts("deferred" + s, i))
        assert all(t is not None for i in range(len(b.records[tag["decided_edge" + s]])) for t in texts("decided_edge" + s, i))
    assert texts("ids_not_slots") == ["-0.6021", "-0.6021", "-0.301"] + ["-inf"] * 42
    assert tag["wide_first"] == 0 and tag["wide_last"] == len(b.names) - 1
    assert len(b.records[tag["A70"]]) == 3 and sum(len(texts("A70", i)) for i in range(3)) > 400


def test_argument_checks_and_the_empty_call():
    empty = calls.RecordPlan([0], [0], [], [], [0], [])
    assert len(calls.record_gl_from_bins(np.zeros(1, np.uint32), [], [], [], [], [], empty)) == 0
    with pytest.raises(ValueError):
        calls.record_gl_from_bins(np.array([0, 2], np.uint32), [0, 1], [1], [1, 1], [0.5], [0], empty)   # three bins belong to two alleles
