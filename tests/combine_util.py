"""Shared by the tests of the path-subset flow (tests/test_combine_edges_gpu.py, tests/test_combine_gpu.py): the yardstick —
pangenie_amd/genotyping_result.py, GenotypingResult.combine over the chains of a group in the order given, in np.longdouble —
and the comparison of a group's combined bins against it.  Nothing of pangenie_amd/calls.py or of the kernels forms the
expected values (calls.combined_to_longdouble only reads the bins that are compared)."""
from types import SimpleNamespace

import numpy as np

from pangenie_amd import calls
from pangenie_amd.genotyping_result import GenotypingResult, results_from_flat
from tests.calls_util import geno_off_of

LD = np.longdouble
CUT = LD(2.0) ** -16300


def combined_yardstick(aoff, ids, kept, pres, lik, lik_exp):
    """per variant the combined GenotypingResult (keys over the allele ids) and the set of deferred keys: GenotypingResult.combine
    over the chains in the order given; a key is deferred iff its largest nonzero summand is below 2^-16300"""
    V = len(aoff) - 1
    batch = SimpleNamespace(n_variants=V, allele_off=np.asarray(aoff), allele_id=np.asarray(ids), geno_off=geno_off_of(aoff))
    zeros = np.zeros(V, np.uint16)
    out = [GenotypingResult() for _ in range(V)]
    largest = [dict() for _ in range(V)]
    for s in range(len(kept)):
        lik_ld = np.ldexp(np.asarray(lik[s], np.float64).astype(LD), np.asarray(lik_exp[s]).astype(np.int64))
        for v, r in enumerate(results_from_flat(batch, lik_ld, kept[s], pres[s], zeros, zeros)):
            out[v].combine(r)
            for g, l in r.genotype_to_likelihood.items():
                largest[v][g] = max(largest[v].get(g, LD(0)), l)
    deferred = [{g for g, l in d.items() if 0 < l < CUT} for d in largest]
    return out, deferred


def assert_bins(aoff, ids, got, want, deferred, what):
    """key sets exactly, DEFERRED exactly where the rule says, every other value ldexp(LD(m), e) == the long double sum"""
    goff = geno_off_of(aoff)
    val = calls.combined_to_longdouble(got)
    n_keys = n_deferred = 0
    for v in range(len(aoff) - 1):
        a0, A = int(aoff[v]), int(aoff[v + 1] - aoff[v])
        bin_ = int(goff[v])
        for a in range(A):
            for b in range(a, A):
                key = (int(ids[a0 + a]), int(ids[a0 + b]))
                fl = int(got["flags"][bin_])
                assert (fl & calls.PG_COMBINED_PRESENT != 0) == (key in want[v].genotype_to_likelihood), (what, v, key, fl)
                if key in want[v].genotype_to_likelihood:
                    n_keys += 1
                    assert (fl & calls.PG_COMBINED_DEFERRED != 0) == (key in deferred[v]), (what, v, key, fl)
                    if key in deferred[v]:
                        n_deferred += 1
                        assert int(got["m"][bin_]) == 0 and int(got["e"][bin_]) == 0, (what, v, key)
                    else:
                        assert val[bin_] == want[v].genotype_to_likelihood[key], (what, v, key, got[bin_], want[v].genotype_to_likelihood[key])
                        assert int(got["m"][bin_]) >> 63 == 1 or (int(got["m"][bin_]) == 0 and int(got["e"][bin_]) == 0), (what, v, key, got[bin_])
                else:
                    assert fl == 0 and int(got["m"][bin_]) == 0 and int(got["e"][bin_]) == 0, (what, v, key, got[bin_])
                bin_ += 1
    return n_keys, n_deferred


def calls_yardstick(want):
    out = []
    for r in want:
        c = GenotypingResult()
        c.genotype_to_likelihood = dict(r.genotype_to_likelihood)
        c.normalize()
        g = c.get_likeliest_genotype()
        out.append(None if g[0] < 0 else (int(g[0]), int(g[1]), int(c.get_genotype_quality(g[0], g[1]))))
    return out
