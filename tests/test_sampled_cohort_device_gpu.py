"""Sampled cohorts with the samples' arrays already on the device (include/pangenie_sampler.h: pg_sampler_cohort_new_device,
pg_sampler_counts_*): every output must be, bit for bit, what pg_sampler_cohort_new gives for host copies of
the same arrays — whether the arrays are torch tensors, a SamplerCounts filled by copies, or a SamplerCounts a count plan
filled from reads.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from pangenie_amd import _lib, hmm, kmers
from pangenie_amd import sampler as smp
from tests.test_counts_gpu import genome, plan_over, reads_of, windows
from tests.test_sampled_cohort_gpu import PANEL_FIELDS, PARAMS, TABLE, draw_samples, fixture_panel, panel

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("lik", "lik_exp", "kept", "n_kmers", "coverage")


def outputs(made):
    """runs the job of a sample_cohort[_device] call and takes everything the contract names to the host"""
    job, sampled, best = made
    job.run()
    out = {"results": job.fetch_all(), "panels": list(job.batches), "sampled": sampled, "best": best, "n_chains": job.n_chains}
    job.close()
    return out


def assert_same_outputs(got, want, phasing, what):
    assert got["n_chains"] == want["n_chains"], what
    for s, (rows_g, rows_w) in enumerate(zip(got["sampled"], want["sampled"])):
        for c, (g, w) in enumerate(zip(rows_g, rows_w)):
            assert np.array_equal(g, w), (what, "sampled paths", s, c)
            assert got["best"][s][c].tolist() == want["best"][s][c].tolist(), (what, "best scores", s, c)
    for chain, (g, w) in enumerate(zip(got["panels"], want["panels"])):
        assert g.n_paths == w.n_paths and g.n_variants == w.n_variants, (what, chain)
        for f in PANEL_FIELDS:
            assert np.array_equal(getattr(g, f), getattr(w, f)), (what, "panel", chain, f)
    for chain, (g, w) in enumerate(zip(got["results"], want["results"])):
        assert g.n_columns == w.n_columns, (what, chain)
        for f in RESULT_FIELDS:
            assert np.array_equal(getattr(g, f), getattr(w, f)), (what, chain, f)
        if phasing:
            assert np.array_equal(g.haplotype_1, w.haplotype_1) and np.array_equal(g.haplotype_2, w.haplotype_2), (what, chain)


def as_device(samples):
    """host arrays -> the form CountPlan.fill_device returns: int16 tensors on the device holding the uint16 bits"""
    return [([torch.from_numpy(a.view(np.int16).copy()).to("cuda") for a in kcs], [torch.from_numpy(a.view(np.int16).copy()).to("cuda") for a in covs])
            for kcs, covs in samples]


@pytest.fixture(scope="module")
def cohort():
    index = [fixture_panel(), panel(150, 64, 11, 2, 4), panel(60, 40, 13, a_lo=6, a_hi=12), panel(10, 30, 14).slice(0, 0)]
    return index, draw_samples(index, 3, 31)


@pytest.mark.parametrize("kernel,phasing", [("fast", False), ("general", False), ("fast", True)])
def test_device_arrays_equal_host_arrays(cohort, kernel, phasing, monkeypatch):
    index, samples = cohort
    if kernel == "general":
        monkeypatch.setenv("PG_SAMPLER_KERNEL", "general")
    t = hmm.ProbabilityTable(*TABLE)
    p = hmm.make_params(*PARAMS, run_phasing=True) if phasing else hmm.make_params(*PARAMS)
    want = outputs(smp.sample_cohort(index, samples, 15, t, p, add_reference=True))
    assert (smp.last_ms()[1] == 0) == (kernel == "general")
    host_h2d = smp.last_h2d_bytes()
    assert host_h2d[1] == 3 * sum(2 * int(b.kmer_off[-1]) for b in index)
    # precondition: the samples are told apart — at least two of the three picked different paths
    picks = [np.concatenate([want["sampled"][s][c].ravel() for c in range(len(index))]).tobytes() for s in range(3)]
    assert len(set(picks)) >= 2
    tensors = as_device(samples)
    got = outputs(smp.sample_cohort_device(index, tensors, 15, t, p, add_reference=True))
    assert smp.last_h2d_bytes() == (host_h2d[0], 0)
    assert (smp.last_ms()[1] == 0) == (kernel == "general")
    assert_same_outputs(got, want, phasing, "tensors")
    with smp.SamplerCounts(index, 3) as counts:
        for s, (kcs, covs) in enumerate(tensors):
            counts.copy_from(s, kcs, covs)
        for s, (kcs, covs) in enumerate(samples):   # (the arrays read back are the ones that went in: a row per sample, no overlap)
            back_k, back_c = counts.as_tensors(s)
            for c in range(len(index)):
                assert np.array_equal(back_k[c].numpy().view(np.uint16), kcs[c]) and np.array_equal(back_c[c].numpy().view(np.uint16), covs[c]), (s, c)
        ks, cs = counts.pointers(2)
        assert all(ks) and all(cs) and all(a % 256 == 0 for a in ks + cs)   # the empty contig too: a valid zero-length slice
        got = outputs(smp.sample_cohort_device(index, counts, 15, t, p, add_reference=True))
        assert smp.last_h2d_bytes() == (host_h2d[0], 0)
        assert_same_outputs(got, want, phasing, "SamplerCounts")
        # read in place and left alone
        back_k, _ = counts.as_tensors(1)
        assert np.array_equal(back_k[1].numpy().view(np.uint16), samples[1][0][1])


def test_from_reads_the_plan_fills_what_the_sampler_reads():
    """counter -> plan.fill_device(out = a SamplerCounts row) -> sample_cohort_device against plan.fill -> sample_cohort"""
    k, S = 21, 3
    rng = np.random.default_rng(64)
    g = genome(rng, 5000)
    pool = np.unique(kmers.canonical_codes(windows(g, k), k))
    index = [panel(150, 64, 41), panel(90, 215, 42, 2, 3), panel(40, 30, 43), panel(10, 30, 14).slice(0, 0)]
    contigs = plan_over(rng, index, pool)
    t = hmm.ProbabilityTable(*TABLE)
    p = hmm.make_params(*PARAMS)
    with kmers.KmerCounter(k) as counter:
        counter.add_codes(pool)
        with kmers.CountPlan(counter, contigs) as plan:
            for round_ in range(2):   # the second round: another SamplerCounts, other reads and coverages
                coverages = [28 + 3 * s + round_ for s in range(S)]
                filled = []
                with smp.SamplerCounts(index, S) as counts:
                    for s in range(S):
                        counter.reset_counts()
                        counter.count(reads_of(rng, g[1000 * s:1000 * s + 3000], 1500))
                        filled.append(plan.fill(coverages[s]))
                        plan.fill_device(coverages[s], out=counts.rows(s))
                    for s, (kcs, covs) in enumerate(filled):
                        # precondition: counts on both sides of the sampler's "present" threshold of 3
                        every = np.concatenate(kcs)
                        assert (every >= 3).any() and (every < 3).any(), (round_, s)
                        back_k, back_c = counts.as_tensors(s)
                        for c in range(len(index)):
                            assert np.array_equal(back_k[c].numpy().view(np.uint16), kcs[c]), (round_, s, c)
                            assert np.array_equal(back_c[c].numpy().view(np.uint16), covs[c]), (round_, s, c)
                    assert not np.array_equal(filled[0][0][0], filled[1][0][0])
                    got = outputs(smp.sample_cohort_device(index, counts, 6, t, p, add_reference=True))
                    assert smp.last_h2d_bytes()[1] == 0
                want = outputs(smp.sample_cohort(index, filled, 6, t, p, add_reference=True))
                assert_same_outputs(got, want, False, f"round {round_}")
                for s in range(S):   # the coverage the job answers with is the plan's
                    for c, b in enumerate(index):
                        r = got["results"][s * len(index) + c]
                        if r.n_columns:
                            assert np.array_equal(r.coverage, filled[s][1][c]), (round_, s, c)


def test_refusals_are_decided_on_the_host(cohort):
    index, samples = cohort
    t = hmm.ProbabilityTable(*TABLE)
    p = hmm.make_params(*PARAMS)
    tensors = as_device(samples)
    lib = smp._hip()
    arr = (_lib.PgContigBatch * len(index))(*[b.as_c() for b in index])
    ld = C.c_longdouble(25000.0)
    err = C.create_string_buffer(1024)

    def raw(d_samples, size=4):
        cs, keep = smp.marshal_device_samples(index, d_samples)
        h = C.c_void_p()
        rc = lib.pg_sampler_cohort_new_device(0, len(index), arr, len(cs), cs, size, 1, 1.26, ld, 10, t.h, C.byref(p), None, None, C.byref(h), err, 1024)
        del keep
        return rc, h

    # a host array where a device array is expected: refused by name, nothing launched, no job
    bad = [(list(k), list(c)) for k, c in tensors]
    bad[1][0][2] = samples[1][0][2]
    rc, h = raw(bad)
    assert rc == _lib.PG_ERR_INVALID and h.value is None
    assert all(w in err.value for w in (b"pg_sampler_cohort_new_device", b"sample 1", b"contig 2", b"kmer_count")), err.value
    bad = [(list(k), list(c)) for k, c in tensors]
    bad[2][1][0] = samples[2][1][0]
    rc, h = raw(bad)
    assert rc == _lib.PG_ERR_INVALID and h.value is None
    assert all(w in err.value for w in (b"sample 2", b"contig 0", b"coverage")), err.value
    with pytest.raises(hmm.PanGenieError) as e:
        smp.sample_cohort_device(index, bad, 4, t, p)
    assert e.value.code == _lib.PG_ERR_INVALID and "coverage" in str(e.value)
    # ... and a correct call right after them works
    rc, h = raw(tensors)
    assert rc == _lib.PG_OK and h.value
    hmm.Job.from_handle(h.value, t, p).close()
    # a sample outside the handle
    with smp.SamplerCounts(index, 2) as counts:
        counts.rows(1)
        with pytest.raises(hmm.PanGenieError) as e:
            counts.rows(2)
        assert e.value.code == _lib.PG_ERR_INVALID and "sample 2 of 2" in str(e.value)
    # as many passes as paths: the host variant's error, text and code
    small, small_host, small_dev = [index[2]], [([k[2]], [c[2]]) for k, c in samples], [([k[2]], [c[2]]) for k, c in tensors]
    for size in (40, 41):
        with pytest.raises(hmm.PanGenieError) as host:
            smp.sample_cohort(small, small_host, size, t, p)
        with pytest.raises(hmm.PanGenieError) as dev:
            smp.sample_cohort_device(small, small_dev, size, t, p)
        assert dev.value.code == host.value.code == _lib.PG_ERR_INVALID and str(dev.value) == str(host.value)
    # lengths are checked before the C ABI is reached
    with pytest.raises(ValueError):
        smp.sample_cohort_device(small, [([small_dev[0][0][0][:-1]], small_dev[0][1])], 3, t, p)
