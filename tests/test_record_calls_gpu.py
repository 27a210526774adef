"""Calls per VCF record through a job (pg_job_record_plan / pg_job_record_calls / pg_job_fetch_record_calls[_all], k_rcalls and
k_rcalls_wide of pangenie_amd/csrc/pg_calls.hip): every record of every chain against pangenie_amd/genotyping_result.py in
np.longdouble — normalize, the fold onto the record's alleles, get_specific_likelihoods, likeliest genotype, quality
(tests/record_calls_util.py) — on the job's OWN fetched bins, under random plans of 1-3 records per bubble with a tenth of the
record alleles undefined.  No record is left out and none may be deferred (the panels' likelihoods are nowhere near 2^-16300).
One plan per INDEX contig, uploaded once and shared by the samples of a cohort; a chain without a plan is left out; a replaced
plan takes effect; pg_job_calls' records and the bins are what they were; the refusals."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.calls_util import OK, yardstick_of_result
from tests.record_calls_util import assert_record_calls, random_plan, record_yardstick

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)


def check_records(job, plans, what):
    """plans: {index contig: RecordPlan}, already uploaded.  Every chain with a plan: records == yardstick on the fetched bins,
    none deferred, fetch_record_calls_all == fetch_record_calls, a second pg_job_record_calls gives the same records; the bins
    and pg_job_calls' records are what they were before.  Answers the number of records with a call."""
    before, bubble_calls = job.fetch_all(), job.calls()
    recs = job.record_calls()
    again = job.record_calls()
    after, bubble_calls_after = job.fetch_all(), job.calls()
    n_ok, nc = 0, len(job.index)
    for c, (b, r0, r1) in enumerate(zip(job.batches, before, after)):
        assert np.array_equal(r0.lik, r1.lik) and np.array_equal(r0.lik_exp, r1.lik_exp) and np.array_equal(r0.kept, r1.kept)
        assert np.array_equal(bubble_calls[c], bubble_calls_after[c])
        plan = plans.get(c % nc)
        d, n = C.c_void_p(), C.c_uint64()
        assert job._lib.pg_job_device_record_calls(job.h, c, C.byref(d), C.byref(n)) == 0
        if plan is None:   # left out, not an error
            assert len(recs[c]) == 0 and n.value == 0
            continue
        assert recs[c].dtype == calls.CALL_DTYPE and len(recs[c]) == plan.n_records == n.value
        assert np.array_equal(recs[c], again[c]) and np.array_equal(recs[c], calls.fetch_record_calls(job, c))
        want = record_yardstick(b.allele_off, b.allele_id, r0.kept, r0.allele_present, r0.lik, r0.lik_exp, plan)
        assert assert_record_calls(recs[c], want, (what, c)) == []
        n_ok += int((recs[c]["flags"] == OK).sum())
    assert job.record_calls_ms() > 0.0 or n_ok == 0
    return n_ok


def test_64_chains_at_16_paths_with_multiallelic_and_wide_objects_fused(monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "fused")
    monkeypatch.setenv("PG_KERNELS", "small")   # (keeps the wide columns of a job of few 16-path chains fused, as in tests/test_calls_gpu.py)
    index = [synthetic_panel(300, 16, 20, seed=7500, multiallelic_frac=0.3, wide_frac=0.05, wide_at=(0, 150, 299))]
    A = np.diff(index[0].allele_off.astype(np.int64))
    assert (A > 5).sum() >= 3 and ((A > 2) & (A <= 5)).sum() > 30   # both kernels have work
    samples = [tuple([x] for x in synthetic_sample_counts(index[0], seed=7510 + s)) for s in range(64)]
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.n_chains == 64 and job.sweep_mode()[0] == "fused", job.plan()
    job.run()
    plan = random_plan(np.random.default_rng(7501), index[0])
    assert int(np.diff(plan.rec_off.astype(np.int64)).max()) == 3 and (plan.vcf_index == 0xFFFF).sum() > 20
    job.record_plan(0, plan)
    assert check_records(job, {0: plan}, "fused") > 64 * 300
    job.close()


def test_two_chains_at_64_paths_chunked_one_plan_then_two_then_one_replaced(monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    batches = [synthetic_panel(300, 64, 20, seed=7600 + i, multiallelic_frac=0.2) for i in range(2)]
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.sweep_mode()[0] == "chunked", job.plan()
    job.run()
    rng = np.random.default_rng(7601)
    plans = {1: random_plan(rng, batches[1])}
    job.record_plan(1, plans[1])
    assert check_records(job, plans, "chunked, chain 0 without a plan") > 200
    plans[0] = random_plan(rng, batches[0])
    job.record_plan(0, plans[0])
    assert check_records(job, plans, "chunked") > 400
    old = job.record_calls()[1].copy()
    plans[1] = random_plan(rng, batches[1])   # a second plan for the same contig replaces the first
    job.record_plan(1, plans[1])
    assert check_records(job, plans, "chunked, plan replaced") > 400
    new = job.record_calls()[1]
    assert len(new) != len(old) or not np.array_equal(new, old)
    # a plan for another index contig's shape is refused and changes nothing
    with pytest.raises(hmm.PanGenieError) as e:
        job.record_plan(0, random_plan(rng, batches[0].slice(0, 100)))
    assert e.value.code == -1
    assert np.array_equal(job.record_calls()[1], new)
    job.close()


def test_cohort_of_two_samples_over_three_contigs_one_of_them_empty():
    full = [synthetic_panel(270, 16, 20, seed=7700, multiallelic_frac=0.3, wide_frac=0.03, wide_at=(269,)),
            synthetic_panel(120, 16, 20, seed=7701, multiallelic_frac=0.3)]
    index = [full[0], full[0].slice(0, 0), full[1]]
    assert index[1].n_variants == 0
    samples = []
    for s in range(2):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=7710 + 10 * s + c) if ix.n_variants else (np.zeros(0, np.uint16), np.zeros(0, np.uint16))
                          for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.n_chains == 6
    job.run()
    rng = np.random.default_rng(7702)
    plans = {0: random_plan(rng, index[0]), 1: calls.RecordPlan.from_records([]), 2: random_plan(rng, index[2])}
    for c, p in plans.items():   # once per index contig: both samples' chains share it
        job.record_plan(c, p)
    assert check_records(job, plans, "cohort") > 2 * 390
    recs = job.record_calls()
    assert len(recs[1]) == 0 and len(recs[4]) == 0
    assert len(recs[0]) == len(recs[3]) and not np.array_equal(recs[0], recs[3])   # two samples, one plan, two sets of records
    # a new batch of samples invalidates the run: the record calls are refused until the next one
    job.upload_begin(samples[::-1])
    job.upload_end()
    with pytest.raises(hmm.PanGenieError) as e:
        job.record_calls()
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_calls(job, 0)
    assert e.value.code == -1
    job.run()
    swapped = job.record_calls()
    assert np.array_equal(swapped[0], recs[3]) and np.array_equal(swapped[3], recs[0]) and np.array_equal(swapped[2], recs[5])
    job.close()


def test_refusals():
    b = synthetic_panel(40, 16, 20, seed=7800)
    t = hmm.ProbabilityTable(*ARGS)
    plan = random_plan(np.random.default_rng(7801), b)
    job = hmm.Job([b], t, hmm.make_params(1.26, False, 1e-5))
    job.record_plan(0, plan)   # the plan hangs on the index alone: before the run
    with pytest.raises(hmm.PanGenieError) as e:   # before pg_job_run
        job.record_calls()
    assert e.value.code == -1
    job.run()
    with pytest.raises(hmm.PanGenieError) as e:   # records are fetched only after pg_job_record_calls
        calls.fetch_record_calls(job, 0)
    assert e.value.code == -1
    assert len(job.record_calls(0)) == plan.n_records
    with pytest.raises(hmm.PanGenieError) as e:   # no such index contig
        job.record_plan(1, plan)
    assert e.value.code == -1
    # an allele id of the index outside a record's map: found when the records are formed, on the host
    short = calls.RecordPlan.from_records([[([0], [True])] for _ in range(40)])
    job.record_plan(0, short)
    with pytest.raises(hmm.PanGenieError) as e:
        job.record_calls()
    assert e.value.code == -1
    job.record_plan(0, plan)
    assert len(job.record_calls(0)) == plan.n_records
    job.close()
    job = hmm.Job([b], t, hmm.make_params(1.26, False, 1e-5, run_genotyping=False, run_phasing=True))
    job.run()
    with pytest.raises(hmm.PanGenieError) as e:   # a job without run_genotyping has no bins
        job.record_calls()
    assert e.value.code == -1
    job.close()


def test_where_the_records_differ_from_the_calls():
    """The record calls' side of tests/test_calls_gpu.py's test_what_only_the_calls_do: a chain with nothing to fetch needs no `out`,
    the device pointers are refused from a new plan until the records are formed again (the calls' are not), a later pg_job_run
    leaves the formed records fetchable, and pg_record_calls_from_bins checks its plan before V = 0 answers PG_OK."""
    b = synthetic_panel(10, 16, 20, seed=7850)
    rng = np.random.default_rng(7851)
    job = hmm.Job([b, b.slice(0, 0)], hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    lib, err = job._lib, C.create_string_buffer(512)
    plan = random_plan(rng, b)
    job.record_plan(0, plan)
    job.run()
    job.calls()
    recs = job.record_calls()
    d, n = C.c_void_p(), C.c_uint64()
    assert lib.pg_job_device_record_calls(job.h, 0, C.byref(d), C.byref(n)) == 0 and n.value == plan.n_records
    assert lib.pg_job_fetch_record_calls(job.h, 1, None, err, 512) == 0   # nothing to fetch: no `out` needed
    assert lib.pg_job_fetch_record_calls(job.h, 0, None, err, 512) == -1 and err.value == b"bad argument"
    job.run()   # the same inputs again: the records formed before are still there
    assert np.array_equal(calls.fetch_record_calls(job, 0), recs[0])
    job.record_plan(0, random_plan(rng, b))
    assert lib.pg_job_device_record_calls(job.h, 0, C.byref(d), C.byref(n)) == -1
    assert lib.pg_job_device_calls(job.h, 0, C.byref(d), C.byref(n)) == 0 and n.value == 10   # (the calls hang on no plan)
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_calls(job, 0)
    assert e.value.code == -1
    job.record_calls()
    assert lib.pg_job_device_record_calls(job.h, 0, C.byref(d), C.byref(n)) == 0
    job.close()
    assert lib.pg_record_calls_from_bins(0, 0, None, None, None, None, None, None, None, None) == -1   # the null plan, V = 0 or not
