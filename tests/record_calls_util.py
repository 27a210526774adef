"""Shared by the tests of the device's calls per VCF record (tests/test_record_calls_edges_gpu.py, tests/test_record_calls_gpu.py):
the yardstick — pangenie_amd/genotyping_result.py on the SAME bins, in np.longdouble: normalize, the fold onto the record's
alleles (fold_onto_record, Variant::separate_variants restated), get_specific_likelihoods over the defined alleles,
get_likeliest_genotype, 1 - best through log10 — and the comparison of records against it.  Nothing of pangenie_amd/calls.py
or of the kernels is used to form the expected values."""
from types import SimpleNamespace

import numpy as np

from pangenie_amd.genotyping_result import record_call, results_from_flat
from tests.calls_util import DEFERRED, NONE, NOT_UNIQUE, OK, geno_off_of

LD = np.longdouble
EMPTY = 0x100


def record_yardstick(allele_off, allele_id, kept, allele_present, lik, lik_exp, plan):
    """per record (allele_1, allele_2, gq, empty) or None for ./. ; `empty`: the bubble's map has no key at all"""
    V = len(allele_off) - 1
    batch = SimpleNamespace(n_variants=V, allele_off=np.asarray(allele_off), allele_id=np.asarray(allele_id), geno_off=geno_off_of(allele_off))
    lik_ld = np.ldexp(np.asarray(lik, np.float64).astype(LD), np.asarray(lik_exp).astype(np.int64))
    zeros = np.zeros(V, np.uint16)
    out = []
    for v, res in enumerate(results_from_flat(batch, lik_ld, kept, allele_present, zeros, zeros)):
        res.normalize()
        for r in range(int(plan.rec_off[v]), int(plan.rec_off[v + 1])):
            own, vcf = plan.record(r)
            g, gq = record_call(res, own, vcf)
            out.append(None if g is None else (int(g[0]), int(g[1]), int(gq), res.contains_no_likelihoods()))
    assert len(out) == plan.n_records
    return out


def assert_record_calls(records, want, what=""):
    """every record that is not flagged deferred says what the yardstick says: GT, GQ, call or no call, empty or not; answers
    the deferred records"""
    assert len(records) == len(want), what
    deferred = []
    for r, (rec, w) in enumerate(zip(records, want)):
        fl = int(rec["flags"])
        if fl == DEFERRED:
            deferred.append(r)
            continue
        if w is None:
            assert fl in (NONE, NOT_UNIQUE), (what, r, rec, w)
            assert int(rec["allele_1"]) == 0xFFFF and int(rec["allele_2"]) == 0xFFFF and int(rec["gq"]) == 0, (what, r, rec)
        else:
            assert fl == (OK | EMPTY if w[3] else OK) and (int(rec["allele_1"]), int(rec["allele_2"]), int(rec["gq"])) == w[:3], (what, r, rec, w)
    return deferred


def random_plan(rng, batch, max_records=3, undefined=0.1):
    """a random record plan over a batch's bubbles: 1 .. max_records records each, every bubble allele id mapped onto one of
    the record's 1 .. 6 alleles (id 0 onto 0), a share `undefined` of the non-reference record alleles without a sequence"""
    from pangenie_amd.calls import RecordPlan
    bubbles = []
    aoff, aid = np.asarray(batch.allele_off).astype(np.int64), np.asarray(batch.allele_id)
    for v in range(len(aoff) - 1):
        n_ids = int(aid[aoff[v]:aoff[v + 1]].max()) + 1
        records = []
        for _ in range(int(rng.integers(1, max_records + 1))):
            nA = int(rng.integers(1, min(n_ids, 6) + 1))
            own = rng.integers(0, nA, n_ids)
            own[0] = 0
            defined = [True] + [bool(x) for x in (rng.random(nA - 1) >= undefined)]
            records.append((own.tolist(), defined))
        bubbles.append(records)
    return RecordPlan.from_records(bubbles)
