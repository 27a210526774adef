"""k_viterbi<1|2|4> and k_vit_backtrack (pangenie_amd/csrc/pg_viterbi.hip) on the constructed cases of
tests/viterbi_cases.py — exact zeros, every staging guard, the edges of the 64-column backtrace, wide columns at the
staged-block boundaries, exact ties, the phantom-lane patterns on either side of each width — which
tests/test_viterbi_cases.py proves to reach those conditions.  The bar is that of tests/test_viterbi_gpu.py: kept columns
and haplotype alleles identical to the long double oracle's."""
import numpy as np
import pytest

from oracle import pyoracle as orc  # checker only
from pangenie_amd import hmm
from pangenie_amd.panel import synthetic_panel
from tests import viterbi_cases as vc
from tests.fixtures_util import fill_table

pytestmark = pytest.mark.gpu

CASES = vc.all_cases()
BY_NAME = {c.name: c for c in CASES}


def device_table(spec):
    t = hmm.ProbabilityTable(default=True) if spec["default"] else hmm.ProbabilityTable(*spec["args"])
    return fill_table(t, spec, orc.copynumber_regularized)


def check(res, ref, what, meta=False):
    assert res.n_columns == ref.n_columns, what
    assert np.array_equal(res.kept, ref.kept), what
    bad = np.flatnonzero((res.haplotype_1 != ref.hap1) | (res.haplotype_2 != ref.hap2))
    assert bad.size == 0, (what, bad[:10], res.haplotype_1[bad[:10]], ref.hap1[bad[:10]], res.haplotype_2[bad[:10]], ref.hap2[bad[:10]])
    if meta:  # (sic: by column index, reference src/hmm.cpp:164-165)
        assert np.array_equal(res.n_kmers, ref.n_kmers) and np.array_equal(res.coverage, ref.coverage), what


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_viterbi_case(case):
    """(the twins_below_fp64 cases are the ones that found the contracted double-double products: with `p + e` and
    `s - p` of dd_mul fused into FMAs the device exchanged the two haplotype alleles at 11 of 59 columns with 16 paths, at
    4 of 60 with 32 and at 15 of 60 with 64, where the exact-rational restatement and the emulation of the specified
    double-double arithmetic of tests/test_viterbi_precision.py both give the oracle's haplotypes)"""
    t = device_table(case.table)
    for regime in case.regimes:
        recomb, eff_n, uniform = regime
        ref = vc.oracle_result(case.name, regime)
        for geno in (False, True) if case.genotyping else (False,):
            res = hmm.genotype_contig(case.batch, t, hmm.make_params(recomb, uniform, eff_n, run_genotyping=geno, run_phasing=True))
            check(res, ref, (case.name, vc.REGIME_NAME[regime], geno), meta=not geno)


def no_columns():
    b = synthetic_panel(40, 6, 20, seed=77)
    b.path_allele[:] = 0  # every path carries the reference allele: no column is kept
    return b


JOBS = {  # chains of one job: the launch mask (hp_bits) and each kernel's early return on chains of another width
    "width16_only": ["a_H7_C33", "a_H16_C65", "b_H6_ends_and_mid", "d_H12_wide", "a_H16_C1"],
    "width32_only": ["a_H20_C33", "a_H32_C65", "b_H30_ends_and_mid", "d_H24_wide", "a_H32_C1"],
    "width64_only": ["a_H40_C33", "a_H64_C65", "b_H64_ends_and_mid", "d_H48_wide", "a_H64_C1"],
    "width16_and_64": ["a_H16_C64", "a_H64_C97", "b_H6_run65_last", "b_H64_run64_last", "d_H64_wide", "a_H7_C2"],
    "C0_C1_C33": [None, "a_H7_C1", "a_H20_C33", None, "a_H64_C1", "a_H64_C33", "a_H20_C1", "a_H16_C33"],
}


@pytest.mark.parametrize("name", list(JOBS), ids=list(JOBS))
def test_viterbi_job(name):
    """one resident job, run twice; phasing only, so the by-column-index meta data are checked too"""
    recomb, eff_n, uniform = vc.PRODUCTION
    cases = [BY_NAME[n] if n else None for n in JOBS[name]]
    assert all(c is None or (c.table is vc.PANEL_TABLE and vc.PRODUCTION in c.regimes) for c in cases)
    batches = [c.batch if c else no_columns() for c in cases]
    widths = {vc.kernel_k(b.n_paths) for b in batches}
    assert widths == {"width16_only": {1}, "width32_only": {2}, "width64_only": {4}, "width16_and_64": {1, 4}, "C0_C1_C33": {1, 2, 4}}[name]
    o = vc.oracle_table(vc.PANEL_TABLE)
    prm = orc.make_params(recomb, uniform, eff_n, run_genotyping=False, run_phasing=True)
    refs = [vc.oracle_result(c.name, vc.PRODUCTION) if c else orc.viterbi_contig(b, o, prm, form=0) for c, b in zip(cases, batches)]
    if name == "C0_C1_C33":
        assert sorted({r.n_columns for r in refs}) == [0, 1, 33]
    job = hmm.Job(batches, device_table(vc.PANEL_TABLE), hmm.make_params(recomb, uniform, eff_n, run_genotyping=False, run_phasing=True))
    try:
        for run in range(2):
            job.run()
            for i, ref in enumerate(refs):
                check(job.fetch(i), ref, (name, run, i), meta=True)
    finally:
        job.close()
