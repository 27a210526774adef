"""The reference's own known answers of GenotypingResult (tests/golden/genotyping_result_known_answers.json: the 16 cases of its
tests/GenotypingResultTest.cpp, as data) on the two things that must both say what they say:

  - pangenie_amd/genotyping_result.py, the np.longdouble yardstick of every test of the device's calls, records, GL values and
    combined bins (CPU part: every step of every case, likelihoods at the reference's own 1e-7, GT / GQ / sizes / booleans exactly,
    the throw of get_genotype_quality on unnormalised input, get_all_likelihoods' order and its error outside nr_alleles);
  - the device's unit entry points (GPU part), fed with the cases' add_to_likelihood sums as (mantissa, exponent) pairs of np.frexp:
    calls.calls_from_bins (likeliest genotype, the tie and the empty result, GQ 2 / 3 / 10000), calls.record_calls_from_bins and
    calls.record_gl_from_bins (get_specific_likelihoods with allele 1 undefined, get_all_likelihoods' order, normalize),
    calls.combine_bins and calls.calls_from_combined (combine, combine_empty1..3).  One launch per entry point: the cases are the
    variants of one contig.  What the device is given and what it is held to come from the JSON alone, not from the yardstick.

Host only, on the yardstick alone: coverage_kmers, contains_no_likelihoods, divide_likelihoods_by (no device entry point computes
them; the JSON marks them "host_only"), and the GQ 0 of the triallelic case — the quality of genotype 0/1, which is NOT the
likeliest there: every device entry point forms the quality of the likeliest genotype only (its GQ 3 is checked on the device).
combine's r3 lacks the keys 1/1 and 0/2 although alleles 0, 1 and 2 all occur in it: allele_present is per allele, so the device's
chain carries them as keys of value 0 — the sums are the same, the union's key set holds 0/2 in addition."""
import json
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd.genotyping_result import GenotypingResult

LD = np.longdouble
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "genotyping_result_known_answers.json").read_text())
CASES = {c["name"]: c for c in GOLDEN["cases"]}
TOL = GOLDEN["tolerance"]
HOST_ONLY = ["divide_likelihoods_by", "coverage_kmers", "contains_no_likelihoods"]


def test_the_file_holds_the_sixteen_cases():
    assert len(GOLDEN["cases"]) == 16 and len(CASES) == 16 and TOL == 1e-7
    assert sorted(c["name"] for c in GOLDEN["cases"] if c.get("host_only")) == sorted(HOST_ONLY)
    assert all(c["ref"].startswith("tests/GenotypingResultTest.cpp:") and c["steps"] for c in GOLDEN["cases"])


# ---- CPU: the yardstick ---------------------------------------------------------------------------------------------------------
def close(got, want):
    return abs(LD(got) - LD(want)) < TOL   # tests/utils.cpp:9-11


@pytest.mark.parametrize("name", list(CASES))
def test_yardstick_gives_the_references_answers(name):
    objs, checked = {}, 0
    for i, s in enumerate(CASES[name]["steps"]):
        r = objs.setdefault(s["on"], GenotypingResult())
        op, what = s["op"], (name, i, s)
        if op == "add_to_likelihood":
            r.add_to_likelihood(*s["genotype"], s["value"])
        elif op == "get_genotype_likelihood":
            assert close(r.get_genotype_likelihood(*s["genotype"]), s["expect"]), what
        elif op == "add_first_haplotype_allele":
            r.haplotype_1 = s["allele"]
        elif op == "add_second_haplotype_allele":
            r.haplotype_2 = s["allele"]
        elif op == "get_haplotype":
            assert [r.haplotype_1, r.haplotype_2] == s["expect"], what
        elif op == "get_likeliest_genotype":
            assert list(r.get_likeliest_genotype()) == s["expect"], what
        elif op == "divide_likelihoods_by":
            r.divide_likelihoods_by(s["value"])
        elif op == "get_all_likelihoods":
            got = r.get_all_likelihoods(s["nr_alleles"])
            assert len(got) == len(s["expect"]) and all(close(g, w) for g, w in zip(got, s["expect"])), (what, got)
        elif op == "get_specific_likelihoods":
            got = r.get_specific_likelihoods(s["defined_alleles"]).get_all_likelihoods(s["nr_alleles"])
            assert len(got) == len(s["expect"]) and all(close(g, w) for g, w in zip(got, s["expect"])), (what, got)
        elif op == "get_genotype_quality":
            if s["expect"] == "throws":
                with pytest.raises(RuntimeError):
                    r.get_genotype_quality(*s["genotype"])
            else:
                got = r.get_genotype_quality(*s["genotype"])
                assert isinstance(got, int) and got == s["expect"], (what, got)
        elif op == "combine":
            r.combine(objs.setdefault(s["other"], GenotypingResult()))
        elif op == "normalize":
            r.normalize()
        elif op == "set_coverage":
            r.local_coverage = s["value"]
        elif op == "coverage":
            assert r.coverage() == s["expect"], what
        elif op == "set_unique_kmers":
            r.unique_kmers = s["value"]
        elif op == "nr_unique_kmers":
            assert r.nr_unique_kmers() == s["expect"], what
        elif op == "contains_no_likelihoods":
            assert r.contains_no_likelihoods() is s["expect"], what
        else:
            raise AssertionError(("unknown op", what))
        checked += "expect" in s
    assert checked > 0


def test_get_all_likelihoods_refuses_a_genotype_outside_nr_alleles():
    """src/genotypingresult.cpp:48-67: the triallelic case asked for two alleles throws; the biallelic one asked for three gives six
    values in the VCF's order with zeros for the keys it does not hold"""
    tri, bi = GenotypingResult(), GenotypingResult()
    for s in CASES["get_all_likelihoods (triallelic)"]["steps"]:
        if s["op"] == "add_to_likelihood":
            tri.add_to_likelihood(*s["genotype"], s["value"])
    for s in CASES["get_all_likelihoods (biallelic)"]["steps"]:
        if s["op"] == "add_to_likelihood":
            bi.add_to_likelihood(*s["genotype"], s["value"])
    with pytest.raises(RuntimeError):
        tri.get_all_likelihoods(2)
    with pytest.raises(RuntimeError):
        bi.get_all_likelihoods(1)
    got = bi.get_all_likelihoods(3)
    assert len(got) == 6 and [float(x) for x in got] == [0.1, 0.7, 0.2, 0.0, 0.0, 0.0]


# ---- GPU: the unit entry points ---------------------------------------------------------------------------------------------------
def adds(case, on):
    """{(a, b): fp64 sum} of the add_to_likelihood calls of a case on one object, a <= b"""
    out = {}
    for s in CASES[case]["steps"]:
        if s["op"] == "add_to_likelihood" and s["on"] == on:
            g = tuple(sorted(s["genotype"]))
            out[g] = out.get(g, 0.0) + float(s["value"])
    return out


def expects(case, op, on=None):
    return [s for s in CASES[case]["steps"] if s["op"] == op and "expect" in s and (on is None or s["on"] == on)]


def bin_of(A, a, b):
    return a * A - a * (a - 1) // 2 + (b - a)


def contig(variants):
    """variants: (A, {(a, b): value} or None for a variant that is not kept) -> allele_off, allele_id, kept, allele_present, lik, lik_exp;
    an allele is present iff some key names it"""
    aoff, aid, kept, pres, lik = [0], [], [], [], []
    for A, keys in variants:
        aoff.append(aoff[-1] + A)
        aid += list(range(A))
        kept.append(0 if keys is None else 1)
        named = {a for g in (keys or {}) for a in g}
        pres += [1 if a in named else 0 for a in range(A)]
        row = [0.0] * (A * (A + 1) // 2)
        for (a, b), x in (keys or {}).items():
            row[bin_of(A, a, b)] = x
        lik += row
    m, e = np.frexp(np.asarray(lik, np.float64))
    return (np.asarray(aoff, np.uint32), np.asarray(aid, np.uint16), np.asarray(kept, np.uint8), np.asarray(pres, np.uint8), m, e.astype(np.int32))


def call_from_numbers(values):
    """(index of the largest, GQ) of likelihoods that need not be normalised, from the JSON's numbers in long double"""
    x = np.asarray(values, LD)
    x = x / x.sum()
    best = int(np.argmax(x))
    wrong = LD(1) - x[best]
    return best, (int(-10 * np.log10(wrong)) if wrong > 0 else 10000)


@pytest.mark.gpu
def test_device_calls_give_the_references_answers():
    from pangenie_amd import calls
    from tests.calls_util import DEFERRED, NONE, NOT_UNIQUE, OK, yardstick
    tri = CASES["get_all_likelihoods (triallelic)"]
    variants = [(2, adds("get_genotype_likelihood", "r")), (2, adds("get_likeliest_genotype", "r")), (2, adds("get_likeliest_genotype", "r2")), (2, None),
                (3, adds(tri["name"], "r")), (2, adds("get_genotype_quality unnormalized", "r")), (2, adds("get_genotype_quality", "r"))]
    assert adds("get_likeliest_genotype", "r3") == {} and adds("get_genotype_quality", "r") == {(1, 1): 1.0}
    arrays = contig(variants)
    got = calls.calls_from_bins(*arrays)
    host = yardstick(*arrays)

    def answer(v):
        """the device's, or — for a variant it leaves to the host — the host rule's on the same bins"""
        rec = got[v]
        if int(rec["flags"]) == DEFERRED:
            return ("host",) + (host[v] or ("./.",))
        return ("device", int(rec["flags"]), int(rec["allele_1"]), int(rec["allele_2"]), int(rec["gq"]))

    def likeliest(case, on):
        return expects(case, "get_likeliest_genotype", on)[0]["expect"]
    print([answer(v) for v in range(len(variants))])
    assert answer(0)[-3:-1] == tuple(likeliest("get_genotype_likelihood", "r")) == (1, 1) and answer(0)[0] == "device"
    assert answer(1)[-3:-1] == tuple(likeliest("get_likeliest_genotype", "r")) == (0, 1)
    assert likeliest("get_likeliest_genotype", "r2") == [-1, -1] and answer(2) in (("device", NOT_UNIQUE, 0xFFFF, 0xFFFF, 0), ("host", "./."))
    assert likeliest("get_likeliest_genotype", "r3") == [-1, -1] and answer(3) == ("device", NONE, 0xFFFF, 0xFFFF, 0)
    # the triallelic case: 1/2 is the largest of the JSON's six values, and its quality is the JSON's 3
    six = expects(tri["name"], "get_all_likelihoods")[0]["expect"]
    gq = {tuple(s["genotype"]): s["expect"] for s in expects(tri["name"], "get_genotype_quality")}
    assert int(np.argmax(six)) == 2 * 3 // 2 + 1 and gq == {(1, 2): 3, (0, 1): 0}
    assert answer(4)[-3:] == (1, 2, 3)
    unn = expects("get_genotype_quality unnormalized", "get_genotype_quality")
    assert [s["expect"] for s in unn] == ["throws", 2] and answer(5)[-3:] == (1, 1, 2)   # (the device normalises what it is given)
    assert expects("get_genotype_quality", "get_genotype_quality")[0]["expect"] == 10000 and answer(6)[-3:] == (1, 1, 10000)
    assert all(answer(v)[1] == OK for v in (0, 1, 4, 5, 6) if answer(v)[0] == "device")


@pytest.mark.gpu
def test_device_records_give_the_references_specific_likelihoods_and_order():
    from pangenie_amd import calls
    from tests.calls_util import NOT_UNIQUE, OK
    from tests.record_gl_util import text_of_log, texts_of_values
    spec = expects("get_specific_likelihoods", "get_specific_likelihoods")[0]
    spec2 = expects("get_specific_likelihoods2", "get_specific_likelihoods")[0]
    assert spec["defined_alleles"] == [0, 2] and spec2["defined_alleles"] == [0, 1]
    norm = {tuple(sorted(s["genotype"])): s["expect"] for s in expects("normalize", "get_genotype_likelihood")}
    tri = "get_all_likelihoods (triallelic)"
    # (A, bins, defined record alleles, the JSON's likelihoods in the VCF's order)
    rows = [(3, adds("get_specific_likelihoods", "r"), [True, False, True], spec["expect"]),   # the undefined allele is allele 1
            (2, adds("get_specific_likelihoods2", "r"), [True, True], spec2["expect"]),
            (2, adds("get_all_likelihoods (biallelic)", "r"), [True, True], expects("get_all_likelihoods (biallelic)", "get_all_likelihoods")[0]["expect"]),
            (3, adds(tri, "r"), [True, True, True], expects(tri, "get_all_likelihoods")[0]["expect"]),
            (2, adds("normalize", "g"), [True, True], [norm[(0, 0)], norm[(0, 1)], norm[(1, 1)]])]
    arrays = contig([(A, keys) for A, keys, _, _ in rows])
    plan = calls.RecordPlan.from_records([[(list(range(A)), defined)] for A, _, defined, _ in rows])
    gl_off = calls.record_gl_offsets(plan).astype(np.int64)
    assert np.diff(gl_off).tolist() == [len(want) for *_, want in rows]
    gl = calls.record_gl_from_bins(*arrays, plan)
    rec = calls.record_calls_from_bins(*arrays, plan)
    texts = texts_of_values(gl)
    for r, (A, _, defined, want) in enumerate(rows):
        with np.errstate(divide="ignore"):
            want_text = [text_of_log(x) for x in np.log10(np.asarray(want, LD))]   # log10 of the JSON's numbers at four digits
        assert list(texts[gl_off[r]:gl_off[r + 1]]) == want_text, (r, list(texts[gl_off[r]:gl_off[r + 1]]), want_text)
        n = sum(defined)
        pairs = [(a, b) for b in range(n) for a in range(b + 1)]   # the VCF's order over the defined alleles
        top = sorted(want)[-2:]
        if top[1] - top[0] < 1e-10:
            assert int(rec["flags"][r]) == NOT_UNIQUE, (r, rec[r])   # normalize: 0/0 and 1/1 at 0.4 each
        else:
            best, gq = call_from_numbers(want)
            assert (int(rec["flags"][r]), int(rec["allele_1"][r]), int(rec["allele_2"][r]), int(rec["gq"][r])) == (OK, *pairs[best], gq), (r, rec[r], pairs[best], gq)
    assert int(rec["flags"][4]) == NOT_UNIQUE and (int(rec["allele_1"][0]), int(rec["allele_2"][0])) == (0, 1)


@pytest.mark.gpu
def test_device_combine_gives_the_references_sums():
    from pangenie_amd import calls
    from tests.calls_util import NONE, OK
    r1, r2, r3 = adds("combine", "r1"), adds("combine", "r2"), adds("combine", "r3")
    e1, e2 = adds("combine_empty1", "r2"), adds("combine_empty2", "r1")
    assert adds("combine_empty1", "r1") == adds("combine_empty2", "r2") == adds("combine_empty3", "r1") == adds("combine_empty3", "r2") == {}
    # one triallelic layout, three chains; None: the chain holds no key at that variant (it is not a kept column there)
    chains = [[r1, r1, None, e2, None], [r2, r2, e1, None, None], [None, r3, None, None, None]]
    arrays = [contig([(3, keys) for keys in ch]) for ch in chains]
    aoff, aid = arrays[0][0], arrays[0][1]
    bins = calls.combine_bins(aoff, [a[2] for a in arrays], [a[3] for a in arrays], [a[4] for a in arrays], [a[5] for a in arrays])
    val = calls.combined_to_longdouble(bins)
    steps = CASES["combine"]["steps"]
    second = max(i for i, s in enumerate(steps) if s["op"] == "combine")
    want = [{tuple(sorted(s["genotype"])): s["expect"] for s in steps[:second] if s["op"] == "get_genotype_likelihood"},
            {tuple(sorted(s["genotype"])): s["expect"] for s in steps[second:] if s["op"] == "get_genotype_likelihood"}]
    want += [{tuple(sorted(s["genotype"])): s["expect"] for s in expects(c, "get_genotype_likelihood")} for c in ("combine_empty1", "combine_empty2", "combine_empty3")]
    assert [len(w) for w in want] == [3, 5, 3, 3, 3]
    for v, w in enumerate(want):
        for a in range(3):
            for b in range(a, 3):
                k = 6 * v + bin_of(3, a, b)
                fl = int(bins["flags"][k])
                assert not fl & calls.PG_COMBINED_DEFERRED, (v, a, b)
                assert abs(val[k] - LD(w.get((a, b), 0.0))) < TOL, (v, a, b, val[k], w)
                if w.get((a, b), 0.0) > 0:
                    assert fl & calls.PG_COMBINED_PRESENT, (v, a, b)
                if v == 4 or (v != 1 and 2 in (a, b)):
                    assert fl == 0 and val[k] == 0, (v, a, b, bins[k])   # no chain holds allele 2 there: no such key
    rec = calls.calls_from_combined(aoff, aid, bins)
    pairs = [(a, b) for a in range(3) for b in range(a, 3)]
    for v, w in enumerate(want[:4]):
        best, gq = call_from_numbers([w.get(p, 0.0) for p in pairs])
        assert int(rec["flags"][v]) == OK and (int(rec["allele_1"][v]), int(rec["allele_2"][v])) == pairs[best] == (1, 1), (v, rec[v])
        if v < 2:   # (combine_empty1 / 2: 1 - 0.9 lies on GQ 10's edge, where the JSON's decimal numbers decide nothing ...)
            assert int(rec["gq"][v]) == gq, (v, rec[v], gq)
    assert [int(rec[f][4]) for f in ("flags", "allele_1", "allele_2", "gq")] == [NONE, 0xFFFF, 0xFFFF, 0]
    # (... so there, and everywhere else once more, the yardstick the CPU part pins: combine in the chains' order on the same fp64 sums)
    from tests.combine_util import calls_yardstick
    host = []
    for v in range(5):
        res = GenotypingResult()
        for ch in chains:
            other = GenotypingResult()
            for g, x in (ch[v] or {}).items():
                other.add_to_likelihood(*g, x)
            res.combine(other)
        host.append(res)
    for v, w in enumerate(calls_yardstick(host)):
        got = None if int(rec["flags"][v]) != OK else (int(rec["allele_1"][v]), int(rec["allele_2"][v]), int(rec["gq"][v]))
        assert got == w, (v, rec[v], w)
