"""Shared by the tests of the device's genotype calls (tests/test_calls_gpu.py, tests/test_calls_edges_gpu.py): the
yardstick — pangenie_amd/genotyping_result.py on the SAME bins, in np.longdouble — and the comparison of a chain's records
against it.  Nothing of pangenie_amd/calls.py or of the kernels is used to form the expected values."""
from types import SimpleNamespace

import numpy as np

from pangenie_amd.genotyping_result import results_from_flat

LD = np.longdouble
OK, NONE, NOT_UNIQUE, DEFERRED = 0, 1, 2, 3


def geno_off_of(allele_off):
    A = np.diff(np.asarray(allele_off, np.uint64))
    out = np.zeros(len(allele_off), np.uint64)
    np.cumsum(A * (A + 1) // 2, out=out[1:])
    return out


def yardstick(allele_off, allele_id, kept, allele_present, lik, lik_exp):
    """per variant (allele_1, allele_2, gq) or None for ./. : results_from_flat -> normalize -> get_likeliest_genotype ->
    get_genotype_quality, the host's long double route"""
    V = len(allele_off) - 1
    batch = SimpleNamespace(n_variants=V, allele_off=np.asarray(allele_off), allele_id=np.asarray(allele_id), geno_off=geno_off_of(allele_off))
    lik_ld = np.ldexp(np.asarray(lik, np.float64).astype(LD), np.asarray(lik_exp).astype(np.int64))
    zeros = np.zeros(V, np.uint16)
    out = []
    for r in results_from_flat(batch, lik_ld, kept, allele_present, zeros, zeros):
        r.normalize()
        g = r.get_likeliest_genotype()
        out.append(None if g[0] < 0 else (int(g[0]), int(g[1]), int(r.get_genotype_quality(g[0], g[1]))))
    return out


def assert_calls(records, want, what=""):
    """every record that is not flagged deferred says what the yardstick says: GT, GQ, call or no call; answers the deferred variants"""
    assert len(records) == len(want), what
    deferred = []
    for v, (rec, w) in enumerate(zip(records, want)):
        fl = int(rec["flags"])
        if fl == DEFERRED:
            deferred.append(v)
            continue
        if w is None:
            assert fl in (NONE, NOT_UNIQUE), (what, v, rec, w)
            assert int(rec["allele_1"]) == 0xFFFF and int(rec["allele_2"]) == 0xFFFF and int(rec["gq"]) == 0, (what, v, rec)
        else:
            assert fl == OK and (int(rec["allele_1"]), int(rec["allele_2"]), int(rec["gq"])) == w, (what, v, rec, w)
    return deferred


def yardstick_of_result(batch, res):
    """the yardstick on a fetched ContigResult (the job's own bins)"""
    return yardstick(batch.allele_off, batch.allele_id, res.kept, res.allele_present, res.lik, res.lik_exp)
