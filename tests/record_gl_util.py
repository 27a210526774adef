"""Shared by the tests of the device's GL column per VCF record (tests/test_record_gl_edges_gpu.py, tests/test_record_gl_gpu.py,
tests/test_gl_values_gpu.py): the yardstick — pangenie_amd/genotyping_result.py on the SAME bins in np.longdouble: normalize,
fold_onto_record, get_specific_likelihoods over the defined alleles, get_all_likelihoods — and the text the reference prints of
each value, `setprecision(4) << log10(long double)`, formed from the long double itself (numpy's exact decimal expansion, not
a detour through a double).  Nothing of pangenie_amd/calls.py or of the kernels is used to form the expected texts."""
from types import SimpleNamespace

import numpy as np

from pangenie_amd import calls
from pangenie_amd.genotyping_result import fold_onto_record, results_from_flat
from tests.calls_util import geno_off_of

LD = np.longdouble


def text_of_log(v) -> str:
    """"%.4Lg" of a long double: four significant digits, correctly rounded from the exact binary value"""
    v = LD(v)
    if np.isinf(v):
        return "-inf" if v < 0 else "inf"
    if v == 0:
        return "0"
    sci = np.format_float_scientific(v, precision=3, unique=False, trim="k")   # d.ddde-XX, exact
    return "%.4g" % float(sci)   # four digits survive a double; %g strips the zeros and chooses the notation


def texts_of_likelihoods(x) -> list:
    with np.errstate(divide="ignore"):
        return [text_of_log(v) for v in np.log10(np.asarray(x, LD))]


def record_gl_yardstick(allele_off, allele_id, kept, allele_present, lik, lik_exp, plan):
    """per record the texts of its GL values, in the VCF's order"""
    V = len(allele_off) - 1
    batch = SimpleNamespace(n_variants=V, allele_off=np.asarray(allele_off), allele_id=np.asarray(allele_id), geno_off=geno_off_of(allele_off))
    lik_ld = np.ldexp(np.asarray(lik, np.float64).astype(LD), np.asarray(lik_exp).astype(np.int64))
    zeros = np.zeros(V, np.uint16)
    out = []
    for v, res in enumerate(results_from_flat(batch, lik_ld, kept, allele_present, zeros, zeros)):
        res.normalize()
        for r in range(int(plan.rec_off[v]), int(plan.rec_off[v + 1])):
            own, vcf = plan.record(r)
            f = fold_onto_record(res, own)
            if f.contains_no_likelihoods():
                f.add_to_likelihood(0, 0, 1.0)
            defined = [a for a, x in enumerate(vcf) if int(x) != 0xFFFF]
            gl = f.get_specific_likelihoods(defined) if len(defined) < len(vcf) else f
            out.append(texts_of_likelihoods(gl.get_all_likelihoods(len(defined))))
    assert len(out) == plan.n_records
    return out


def texts_of_values(values) -> np.ndarray:
    """pg_gl_text of every value (None where deferred), one library call per distinct value"""
    values = np.ascontiguousarray(values, calls.GL_DTYPE)
    words = values.view(np.uint32)
    uniq, inv = np.unique(words, return_inverse=True)
    table = np.array([calls.gl_text(u.reshape(1).view(calls.GL_DTYPE)[0]) for u in uniq], dtype=object)
    return table[inv] if len(values) else np.zeros(0, object)


def is_deferred(values) -> np.ndarray:
    return (values["mant"] == 0) & (values["exp10"] == calls.PG_GL_DEFERRED)


def assert_record_gl(values, gl_off, want, what=""):
    """every value that is not deferred prints what the yardstick prints; answers the indices of the deferred values"""
    gl_off = np.asarray(gl_off).astype(np.int64)
    assert len(gl_off) == len(want) + 1 and int(gl_off[-1]) == len(values), (what, len(values), int(gl_off[-1]))
    flat = [t for rec in want for t in rec]
    assert [len(rec) for rec in want] == np.diff(gl_off).tolist(), what
    got = texts_of_values(values)
    deferred = np.flatnonzero(is_deferred(values))
    bad = [i for i in range(len(flat)) if got[i] is not None and got[i] != flat[i]]
    assert not bad, (what, [(i, int(np.searchsorted(gl_off, i, "right")) - 1, got[i], flat[i]) for i in bad[:10]])
    assert all(got[i] is not None for i in range(len(flat)) if i not in set(deferred.tolist())), what
    return deferred.tolist()
