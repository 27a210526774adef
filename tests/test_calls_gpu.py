"""Genotype calls on the device through a job (pg_job_calls / pg_job_fetch_calls[_all], pangenie_amd/csrc/pg_calls.hip): the
8-byte records of every chain against pangenie_amd/genotyping_result.py — results_from_flat -> normalize ->
get_likeliest_genotype -> get_genotype_quality in np.longdouble, the reference's src/genotypingresult.cpp:118-210 — on the
job's OWN fetched bins.  No variant is left out of the comparison and none may be deferred: the panels' likelihoods are
nowhere near 2^-16300 (smallest bin exponent of these panels: -247; the test prints it per chain).  The refusals, a second
pg_job_calls, and the bins before and after it.  (All-zero, tied and deferred variants through a job:
tests/test_regime_consumers_gpu.py.)"""
import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.calls_util import OK, assert_calls, yardstick_of_result

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)


def check_job(job, what):
    """every chain: calls == yardstick on the fetched bins, no deferred variant, fetch_calls_all == fetch_calls, a second
    pg_job_calls gives the same records, and the bins are what they were before the calls were formed"""
    before = job.fetch_all()
    recs = job.calls()
    again = job.calls()
    after = job.fetch_all()
    n_ok = 0
    for c, (b, r0, r1) in enumerate(zip(job.batches, before, after)):
        assert np.array_equal(r0.lik, r1.lik) and np.array_equal(r0.lik_exp, r1.lik_exp) and np.array_equal(r0.kept, r1.kept)
        assert recs[c].dtype == calls.CALL_DTYPE and len(recs[c]) == b.n_variants
        assert np.array_equal(recs[c], again[c]) and np.array_equal(recs[c], calls.fetch_calls(job, c))
        if r0.lik_exp.size and (r0.lik != 0).any():
            print(what, "chain", c, "smallest bin exponent", int(r0.lik_exp[r0.lik != 0].min()))
        deferred = assert_calls(recs[c], yardstick_of_result(b, r0), (what, c))
        assert deferred == []
        n_ok += int((recs[c]["flags"] == OK).sum())
    assert job.calls_ms() > 0.0 or all(b.n_variants == 0 for b in job.batches)
    return n_ok


@pytest.mark.parametrize("mode", ["fused", "chunked"])
def test_three_chains_at_16_paths_with_multiallelic_and_wide_objects(mode, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", mode)
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    monkeypatch.setenv("PG_KERNELS", "small")   # (by default only jobs with hundreds of 16-path chains take k_sweep_small16x, which keeps wide columns fused)
    batches = [synthetic_panel(300, 16, 20, seed=7100 + i, multiallelic_frac=0.3, wide_frac=0.05, wide_at=(0, 150, 299)) for i in range(3)]
    A = np.concatenate([np.diff(b.allele_off.astype(np.int64)) for b in batches])
    assert (A > 5).sum() >= 9 and ((A > 2) & (A <= 5)).sum() > 100   # both kernels have work
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.sweep_mode()[0] == mode, job.plan()
    job.run()
    assert check_job(job, mode) > 600
    job.close()


def test_one_chain_at_64_paths():
    b = synthetic_panel(200, 64, 20, seed=7200, multiallelic_frac=0.2)
    job = hmm.Job([b], hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    job.run()
    assert check_job(job, "h64") > 120
    job.close()


def test_cohort_of_two_samples_over_two_contigs_one_of_them_empty():
    full = synthetic_panel(270, 16, 20, seed=7300, multiallelic_frac=0.3, wide_frac=0.03, wide_at=(269,))
    index = [full, full.slice(0, 0)]
    assert index[1].n_variants == 0
    samples = []
    for s in range(2):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=7310 + 10 * s + c) if ix.n_variants else (np.zeros(0, np.uint16), np.zeros(0, np.uint16))
                          for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.n_chains == 4
    job.run()
    assert check_job(job, "cohort") > 300
    recs = job.calls()
    assert len(recs[1]) == 0 and len(recs[3]) == 0
    assert not np.array_equal(recs[0], recs[2])   # two samples, two sets of calls
    # a new batch of samples invalidates the run: the calls are refused until the next one
    job.upload_begin(samples[::-1])
    job.upload_end()
    with pytest.raises(hmm.PanGenieError) as e:
        job.calls()
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_calls(job, 0)
    assert e.value.code == -1
    job.run()
    swapped = job.calls()
    assert np.array_equal(swapped[0], recs[2]) and np.array_equal(swapped[2], recs[0])
    job.close()


def test_refusals():
    b = synthetic_panel(40, 16, 20, seed=7400)
    t = hmm.ProbabilityTable(*ARGS)
    job = hmm.Job([b], t, hmm.make_params(1.26, False, 1e-5))
    with pytest.raises(hmm.PanGenieError) as e:   # before pg_job_run
        job.calls()
    assert e.value.code == -1
    job.run()
    with pytest.raises(hmm.PanGenieError) as e:   # records are fetched only after pg_job_calls
        calls.fetch_calls(job, 0)
    assert e.value.code == -1
    assert len(job.calls(0)) == 40
    job.close()
    job = hmm.Job([b], t, hmm.make_params(1.26, False, 1e-5, run_genotyping=False, run_phasing=True))
    job.run()
    with pytest.raises(hmm.PanGenieError) as e:   # a job without run_genotyping has no bins
        job.calls()
    assert e.value.code == -1
    job.close()


def test_what_only_the_calls_do():
    """Where pg_job_calls and its fetches differ from the record families (tests/test_record_calls_gpu.py and
    tests/test_record_gl_gpu.py: test_where_the_records_differ_from_the_calls): a null `out` is refused even for a chain without variants, the device pointers are handed out as soon as the buffer
    exists, a later pg_job_run leaves the formed calls fetchable, and pg_calls_from_bins answers V = 0 before it looks at a pointer."""
    import ctypes as C
    b = synthetic_panel(10, 16, 20, seed=7450)
    job = hmm.Job([b, b.slice(0, 0)], hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    lib, err = job._lib, C.create_string_buffer(512)
    job.run()
    d, n = C.c_void_p(), C.c_uint64()
    assert lib.pg_job_device_calls(job.h, 0, C.byref(d), C.byref(n)) == -1   # no buffer yet
    recs = job.calls()
    assert lib.pg_job_device_calls(job.h, 0, C.byref(d), C.byref(n)) == 0 and n.value == 10 and d.value
    assert lib.pg_job_device_calls(job.h, 1, C.byref(d), C.byref(n)) == 0 and n.value == 0
    assert lib.pg_job_fetch_calls(job.h, 1, None, err, 512) == -1 and err.value == b"bad argument"   # nothing to fetch, `out` asked for all the same
    assert len(calls.fetch_calls(job, 1)) == 0
    job.run()   # the same inputs again: the records formed before are still there, and still the same after forming them anew
    assert np.array_equal(calls.fetch_calls(job, 0), recs[0])
    assert np.array_equal(job.calls()[0], recs[0])
    job.close()
    assert lib.pg_calls_from_bins(0, 0, None, None, None, None, None, None, None) == 0
