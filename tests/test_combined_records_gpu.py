"""GT, GQ and GL per VCF record of combined groups through a job (pg_job_combined_record_calls / pg_job_combined_record_gl,
pangenie_amd/csrc/pg_combine_records.hip): the panel of tests/test_combine_gpu.py — two contigs of 300 variants over 12 paths,
three subsets of 4 paths, ONE job of six chains in two groups — with a random record plan per contig (up to 3 records a bubble,
a tenth of the record alleles undefined) on the index contig of each group's FIRST chain only.  Records and GL values against
the long double route over the job's own fetched bins (tests/combined_records_util.py), bit for bit against the unit entry
points fed with job.combined(), the fetch forms, a second formation, what the new calls leave untouched, reversed groups,
groups of ONE chain against that chain's own record_calls() / record_gl() byte for byte, a group without a plan, the refusals.
Chunked sweeps on the panel with its objects of 6 .. 12 alleles, fused sweeps once on the panel without them."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import calls, hmm
from tests.combine_util import combined_yardstick
from tests.combined_records_util import make_panel, one_entry_short, panel_plans, plan_coverage, records_yardstick
from tests.record_calls_util import assert_record_calls
from tests.record_gl_util import assert_record_gl

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
GROUPS = [[0, 1, 2], [3, 4, 5]]


@pytest.fixture(scope="module")
def panel():
    return make_panel(True)


@pytest.fixture(scope="module")
def narrow_panel():
    return make_panel(False)


def new_job(panel):
    batches = [b for sub in panel for b in sub]
    return hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5)), batches


def refused(fn, code=-1):
    with pytest.raises(hmm.PanGenieError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def check_groups(job, groups, plans, what):
    """plans[g]: the plan on group g's first chain's index contig.  Forms both columns and compares them with the yardstick over
    the job's own fetched bins and with the unit entry points; answers (records, values, deferred values)."""
    results = job.fetch_all()
    bins = job.combined()
    recs, gls = job.combined_record_calls(), job.combined_record_gl()
    assert job.combined_record_calls_ms() > 0.0 and job.combined_record_gl_ms() > 0.0
    n_deferred = 0
    for g, grp in enumerate(groups):
        b, plan = job.batches[grp[0]], plans[g]
        want, deferred = combined_yardstick(b.allele_off, b.allele_id, [results[c].kept for c in grp], [results[c].allele_present for c in grp],
                                            [results[c].lik for c in grp], [results[c].lik_exp for c in grp])
        assert not any(deferred)   # (the panels' likelihoods are nowhere near 2^-16300)
        calls_want, gl_want = records_yardstick(plan, want)
        gl_off = calls.record_gl_offsets(plan)
        assert recs[g].dtype == calls.CALL_DTYPE and gls[g].dtype == calls.GL_DTYPE
        assert assert_record_calls(recs[g], calls_want, (what, g)) == []   # no record may be PG_CALL_DEFERRED
        n_deferred += len(assert_record_gl(gls[g], gl_off, gl_want, (what, g)))
        # the unit entry points over the job's combined bins: the same kernels, the same bytes
        assert calls.record_calls_from_combined(b.allele_off, b.allele_id, bins[g], plan).tobytes() == recs[g].tobytes(), (what, g)
        assert calls.record_gl_from_combined(b.allele_off, b.allele_id, bins[g], plan).tobytes() == gls[g].tobytes(), (what, g)
        # the _all fetches are the per-group fetches
        assert job.combined_record_calls(g).tobytes() == recs[g].tobytes() and job.combined_record_gl(g).tobytes() == gls[g].tobytes()
    print(what, "records", sum(len(r) for r in recs), "GL values", sum(len(x) for x in gls), "deferred GL values", n_deferred)
    # the window rule defers about 2e-9 of the values: none is expected, an unlucky digit or two do not fail the run
    assert n_deferred <= 2
    return recs, gls, n_deferred


def test_the_panel_covers_what_the_records_are_about(panel, narrow_panel):
    """on the CPU, from the plans and the batches"""
    n, multi, undef, wide = plan_coverage(panel, panel_plans(panel))
    assert n > 600 and multi > 100 and undef > 20 and wide > 5
    n, multi, undef, wide = plan_coverage(narrow_panel, panel_plans(narrow_panel))
    assert n > 600 and multi > 100 and undef > 20 and wide == 0


def test_fused_sweeps_once_on_the_narrow_panel(narrow_panel, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "fused")
    plans = panel_plans(narrow_panel)
    job, _ = new_job(narrow_panel)
    assert job.sweep_mode()[0] == "fused", job.plan()
    job.run()
    job.combine_plan(GROUPS)
    for g, grp in enumerate(GROUPS):
        job.record_plan(grp[0], plans[g])
    job.combine()
    check_groups(job, GROUPS, plans, "fused")
    job.close()


def test_six_chains_in_two_groups_against_the_host_route(panel, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    plans = panel_plans(panel)
    job, batches = new_job(panel)
    assert job.sweep_mode()[0] == "chunked", job.plan()
    lib, d, n = job._lib, C.c_void_p(), C.c_uint64()
    job.run()
    job.record_plan(0, plans[0])
    assert "pg_job_combine_plan" in refused(job.combined_record_calls)     # without a combine plan
    refused(job.combined_record_gl)
    job.combine_plan(GROUPS)
    assert "pg_job_combine " in refused(job.combined_record_calls) + " "   # before combine()
    refused(job.combined_record_gl)
    job.combine()
    assert lib.pg_job_device_combined_record_calls(job.h, 0, C.byref(d), C.byref(n)) == -1   # nothing formed yet
    # a group whose first chain has no plan is left out, the other is formed
    recs, gls = job.combined_record_calls(), job.combined_record_gl()
    assert len(recs[0]) == plans[0].n_records and len(recs[1]) == 0 and len(gls[1]) == 0 and len(gls[0]) == int(calls.record_gl_offsets(plans[0])[-1])
    assert lib.pg_job_device_combined_record_calls(job.h, 1, C.byref(d), C.byref(n)) == 0 and n.value == 0
    assert lib.pg_job_device_combined_record_gl(job.h, 0, C.byref(d), C.byref(n)) == 0 and n.value == len(gls[0]) and d.value
    err = C.create_string_buffer(256)
    assert lib.pg_job_fetch_combined_record_calls(job.h, 1, None, err, 256) == 0      # no records: no buffer needed
    assert lib.pg_job_fetch_combined_record_calls(job.h, 2, None, err, 256) == -1     # no such group
    only_first = recs[0].tobytes(), gls[0].tobytes()
    # a plan on the second group's first chain: both are formed; a new plan invalidates what was formed
    job.record_plan(3, plans[1])
    assert lib.pg_job_device_combined_record_calls(job.h, 0, C.byref(d), C.byref(n)) == -1
    before = job.fetch_all()
    bins_before, calls_before, ccalls_before = job.combined(), job.calls(), job.combined_calls()
    rcalls_before, rgl_before = job.record_calls(), job.record_gl()
    recs, gls, _ = check_groups(job, GROUPS, plans, "chunked")
    assert (recs[0].tobytes(), gls[0].tobytes()) == only_first
    assert sum(len(r) for r in recs) > 600
    # a second formation gives the same bytes
    again, again_gl = job.combined_record_calls(), job.combined_record_gl()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(recs, again)) and all(x.tobytes() == y.tobytes() for x, y in zip(gls, again_gl))
    # what the new calls leave alone: the bins, the combined bins, the calls, the record calls and GLs of the chains, the combined calls
    for r0, r1 in zip(before, job.fetch_all()):
        assert np.array_equal(r0.lik, r1.lik) and np.array_equal(r0.lik_exp, r1.lik_exp) and np.array_equal(r0.kept, r1.kept)
        assert np.array_equal(r0.allele_present, r1.allele_present)
    assert all(np.array_equal(x, y) for x, y in zip(bins_before, job.combined()))
    assert all(np.array_equal(x, y) for x, y in zip(calls_before, job.calls()))
    assert all(np.array_equal(x, y) for x, y in zip(ccalls_before, job.combined_calls()))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(rcalls_before, job.record_calls()))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(rgl_before, job.record_gl()))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(recs, job.combined_record_calls()))
    # groups of ONE chain: that chain's own record calls and GLs, byte for byte — the new kernels pinned on the existing ones
    job.combine_plan([[0], [3]])
    job.combine()
    one, one_gl = job.combined_record_calls(), job.combined_record_gl()
    assert one[0].tobytes() == rcalls_before[0].tobytes() and one[1].tobytes() == rcalls_before[3].tobytes()
    assert one_gl[0].tobytes() == rgl_before[0].tobytes() and one_gl[1].tobytes() == rgl_before[3].tobytes()
    assert len(one[0]) == plans[0].n_records and len(one[1]) == plans[1].n_records
    # no plan on any group: chains 1 and 4 come first
    job.combine_plan([[1, 0, 2], [4, 3, 5]])
    job.combine()
    assert "record plan" in refused(job.combined_record_calls)
    refused(job.combined_record_gl)
    # the reversed groups give the reversed yardstick (the plans go onto what is now the first chain)
    rev = [g[::-1] for g in GROUPS]
    job.record_plan(2, plans[0])
    job.record_plan(5, plans[1])
    job.combine_plan(rev)
    job.combine()
    recs_r, gls_r, _ = check_groups(job, rev, plans, "reversed")   # (the order moves last bits of the sums: four digits and a GQ seldom show it)
    # a new run without a new combine: refused, as the combined calls are; a new combine invalidates what was formed
    job.run()
    refused(job.combined_record_calls)
    refused(job.combined_record_gl)
    assert lib.pg_job_device_combined_record_gl(job.h, 0, C.byref(d), C.byref(n)) == -1
    job.combine()
    assert lib.pg_job_fetch_combined_record_calls(job.h, 0, recs_r[0].copy().ctypes.data, err, 256) == -1   # formed from the combine before
    assert job.combined_record_calls(0).tobytes() == recs_r[0].tobytes()
    # a plan whose map is one entry short for a bubble's highest id: the device's id check names group and variant
    short, v = one_entry_short(plans[1], batches[3])
    job.record_plan(5, short)
    msg = refused(job.combined_record_calls)
    assert "group 1" in msg and f"variant {v}" in msg, msg
    msg = refused(job.combined_record_gl)
    assert "group 1" in msg and f"variant {v}" in msg, msg
    job.record_plan(5, plans[1])
    assert job.combined_record_gl(1).tobytes() == gls_r[1].tobytes()
    job.close()
