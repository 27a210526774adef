"""Records of sampled cohorts: pg_job_record_plan_strided, the id check on the device (k_rplan_ids) and the
packed fetches, on jobs of sampler.sample_cohort — 3 samples over an index of 3 contigs with 0, 1 and 240 bubbles and 24
panel paths (a third of the bubbles multiallelic with up to 12 alleles, some alleles undefined), sampled to 7 + 1 and to
15 + 1 paths; both jobs keep bubbles of more than five alleles, so the wide kernels run.  Every record call and every GL value
of every chain against pangenie_amd/genotyping_result.py in np.longdouble (tests/record_calls_util.py,
tests/record_gl_util.py) on the chain's OWN fetched bins and OWN fetched reduced panel, under random plans of 1-3 records per
bubble with a tenth of the record alleles undefined, one plan per contig; none may be deferred.  The same bytes with the plan
attached chain by chain; the packed arrays sliced by record_first() equal the per-chain fetches; the refusals, each followed
by a valid call that gives the same again; the shared plan replaced as a whole and for one member."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd import sampler as smp
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.calls_util import OK
from tests.record_calls_util import assert_record_calls, random_plan, record_yardstick
from tests.record_gl_util import assert_record_gl, record_gl_yardstick

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
SEED, NS, NC = 8100, 3, 3


def make_index():
    big = synthetic_panel(240, 24, 20, seed=SEED, multiallelic_frac=0.3, max_alleles=12, undefined_frac=0.05, local_alts=11)
    one = synthetic_panel(1, 24, 20, seed=SEED + 50, multiallelic_frac=1.0, max_alleles=12, local_alts=11)
    A = np.diff(big.allele_off.astype(np.int64))
    assert 0.25 < (A > 2).mean() < 0.4 and A.max() == 12 and (big.allele_flags & 1).sum() >= 5
    return [big.slice(0, 0), one, big]


def make_samples(index):
    none = np.zeros(0, np.uint16)
    out = []
    for s in range(NS):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=SEED + 10 * (c - 1) + s) if ix.n_variants else (none, none) for c, ix in enumerate(index)])
        out.append((list(kcs), list(covs)))
    return out


def make_plans(index, seed):
    rng = np.random.default_rng(seed)
    return [calls.RecordPlan.from_records([]), random_plan(rng, index[1]), random_plan(rng, index[2])]


def bubbles_of(plan):
    """the plan back as RecordPlan.from_records takes it"""
    out = []
    for v in range(plan.n_variants):
        recs = []
        for r in range(int(plan.rec_off[v]), int(plan.rec_off[v + 1])):
            own, vcf = plan.record(r)
            recs.append(([int(x) for x in own], [int(x) != 0xFFFF for x in vcf]))
        out.append(recs)
    return out


class Cohort:
    """a sampled cohort job that has run, its bins (they stay what they are: the job is not run again), and the yardstick's
    answers per (chain, plan), formed once"""

    def __init__(self, size):
        self.index = make_index()
        self.job, _, _ = smp.sample_cohort(self.index, make_samples(self.index), size, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5),
                                           add_reference=True, want_paths=False)
        assert self.job.n_chains == NS * NC and all(b.n_paths == size + 1 for b in self.job.batches if b.n_variants)
        self.job.run()
        self.bins = self.job.fetch_all()
        self.want = {}

    def model(self, chain, plan):
        key = (chain, id(plan))
        if key not in self.want:
            b, r = self.job.batches[chain], self.bins[chain]
            args = (b.allele_off, b.allele_id, r.kept, r.allele_present, r.lik, r.lik_exp, plan)
            self.want[key] = (plan, record_yardstick(*args), record_gl_yardstick(*args))   # (the plan is kept: its id stays its own)
        return self.want[key][1:]

    def strided(self, plans):
        for c, p in enumerate(plans):
            self.job.record_plan_strided(c, NC, p)

    def check_against_the_model(self, plan_of_chain, what):
        """(a): every record call and every GL value of every chain is the model's on that chain's own bins and panel; none
        deferred.  Answers the bytes per chain."""
        rec, gls = self.job.record_calls(), self.job.record_gl()
        called = sum(int((r["flags"] == OK).sum()) for r in rec)   # (calls from evidence: neither `.` nor the 0/0 of an empty bubble)
        finite = sum(int((x["mant"] != 0).sum()) for x in gls)
        print(f"{what}: {sum(len(r) for r in rec)} records, {called} called from likelihoods, {finite} finite GL values")
        assert called > NS * 160 and finite > called, (what, called, finite)
        for g in range(NS * NC):
            plan = plan_of_chain[g]
            want_calls, want_gl = self.model(g, plan)
            assert len(rec[g]) == plan.n_records
            assert assert_record_calls(rec[g], want_calls, (what, g)) == []
            assert assert_record_gl(gls[g], calls.record_gl_offsets(plan), want_gl, (what, g)) == []
        return [r.tobytes() for r in rec], [x.tobytes() for x in gls]


@pytest.fixture(scope="module", params=[7, 15])
def cohort(request):
    c = Cohort(request.param)
    yield c
    c.job.close()


def test_strided_plans_give_the_models_records_the_per_chain_bytes_and_the_packed_arrays(cohort):
    job = cohort.job
    # the reduced panels hold what this test is about: bubbles of more than five alleles (k_rcalls_wide / k_rgl_wide), and
    # allele ids that are not 0 .. A - 1 (the id-keyed lookup)
    wide = other_ids = 0
    for b in job.batches:
        off = b.allele_off.astype(np.int64)
        wide += int((np.diff(off) > 5).sum())
        other_ids += sum(b.allele_id[off[v]:off[v + 1]].tolist() != list(range(off[v + 1] - off[v])) for v in range(b.n_variants))
    assert wide >= 3 and other_ids >= 1, (wide, other_ids)
    plans = make_plans(cohort.index, SEED + 1)
    assert int(np.diff(plans[2].rec_off.astype(np.int64)).max()) == 3 and (plans[2].vcf_index == 0xFFFF).sum() > 20
    cohort.strided(plans)
    by_chain = [plans[g % NC] for g in range(NS * NC)]
    rec_bytes, gl_bytes = cohort.check_against_the_model(by_chain, "strided")   # (a)
    assert job.record_calls_ms() > 0.0 and job.record_gl_ms() > 0.0
    # (c) the packed arrays, sliced by record_first(), are the per-chain fetches
    calls_first, gl_first = job.record_first()
    packed, first = job.record_calls_packed()
    packed_gl, first_gl = job.record_gl_packed()
    assert np.array_equal(first, calls_first) and np.array_equal(first_gl, gl_first)
    assert packed.dtype == calls.CALL_DTYPE and packed_gl.dtype == calls.GL_DTYPE
    assert len(packed) == int(calls_first[-1]) == NS * (plans[1].n_records + plans[2].n_records) and len(packed_gl) == int(gl_first[-1])
    for g in range(NS * NC):
        assert packed[int(calls_first[g]):int(calls_first[g + 1])].tobytes() == rec_bytes[g] == calls.fetch_record_calls(job, g).tobytes(), g
        assert packed_gl[int(gl_first[g]):int(gl_first[g + 1])].tobytes() == gl_bytes[g] == calls.fetch_record_gl(job, g).tobytes(), g
    assert rec_bytes[2] != rec_bytes[5] and gl_bytes[2] != gl_bytes[8]   # three samples, one plan, three sets of records
    # a length that is not the buffer's is refused
    err = C.create_string_buffer(256)
    assert job._lib.pg_job_fetch_record_calls_packed(job.h, packed.ctypes.data, len(packed) + 1, err, 256) == -1
    assert job._lib.pg_job_fetch_record_gl_packed(job.h, packed_gl.ctypes.data, len(packed_gl) - 1, err, 256) == -1
    # (b) the plan attached chain by chain through pg_job_record_plan: the same bytes
    for g in range(NS * NC):
        job.record_plan(g, plans[g % NC])
    assert [r.tobytes() for r in job.record_calls()] == rec_bytes
    assert [x.tobytes() for x in job.record_gl()] == gl_bytes


def test_refusals_attach_nothing_and_the_shared_plan_is_replaced_as_a_whole_and_for_one_member():
    cohort = Cohort(7)
    job = cohort.job
    plans = make_plans(cohort.index, SEED + 2)
    by_chain = [plans[g % NC] for g in range(NS * NC)]

    def refused(*args):
        with pytest.raises(hmm.PanGenieError) as e:
            job.record_plan_strided(*args)
        assert e.value.code == -1, e.value
        return str(e.value)

    # the calls that attach nothing: a job of 9 index contigs is no multiple of 2, contig >= n_contigs, n_contigs == 0, and a plan
    # that fits the first member of its stride only (index contigs 0, 1, 2, ... hold 0, 1, 240, ... bubbles)
    refused(0, 2, plans[0])
    refused(3, 3, plans[2])
    refused(0, 0, plans[0])
    assert "variants" in refused(0, 1, plans[0])
    assert "variants" in refused(1, 3, plans[2])
    assert all(len(r) == 0 for r in job.record_calls()) and all(len(x) == 0 for x in job.record_gl())   # a chain without a plan is left out
    cohort.strided(plans)
    rec_bytes, gl_bytes = cohort.check_against_the_model(by_chain, "after the refusals")
    refused(0, 2, plans[0])   # ... and a refused call leaves the plans that are attached alone
    assert [r.tobytes() for r in job.record_calls()] == rec_bytes

    # a shared plan whose maps are one entry too short for an id that occurs in sample 1 only, at two bubbles: the lowest
    # (chain, variant) is named
    top = [[int(b.allele_id[b.allele_off[v]:b.allele_off[v + 1]].max()) for v in range(240)] for b in (job.batches[s * NC + 2] for s in range(NS))]
    only_1 = [v for v in range(240) if top[1][v] > top[0][v] and top[1][v] > top[2][v]]
    assert len(only_1) >= 2, only_1
    bubbles = bubbles_of(plans[2])
    for v in only_1[:2]:
        bubbles[v] = [(own[:top[1][v]], defined) for own, defined in bubbles[v]]
    short = calls.RecordPlan.from_records(bubbles)
    job.record_plan_strided(2, NC, short)   # (the plan itself is in order: the ids are checked when the records are formed)
    for form in (job.record_calls, job.record_gl):
        with pytest.raises(hmm.PanGenieError) as e:
            form()
        assert e.value.code == -1
        text = str(e.value)
        assert "chain 5" in text and "variant %d:" % only_1[0] in text and "allele id %d " % top[1][only_1[0]] in text and "(%d entries)" % top[1][only_1[0]] in text, text
    with pytest.raises(hmm.PanGenieError):   # ... and the records of the plans before are gone with it
        job.record_calls_packed()
    job.record_plan_strided(2, NC, plans[2])
    assert cohort.check_against_the_model(by_chain, "after the short plan") == (rec_bytes, gl_bytes)

    # the shared plan replaced by another strided call: all its members follow
    second = random_plan(np.random.default_rng(SEED + 3), cohort.index[2])
    job.record_plan_strided(2, NC, second)
    by_chain = [second if g % NC == 2 else plans[g % NC] for g in range(NS * NC)]
    rec_2, gl_2 = cohort.check_against_the_model(by_chain, "shared plan replaced")
    assert all(rec_2[g] != rec_bytes[g] or gl_2[g] != gl_bytes[g] for g in (2, 5, 8)) and all(rec_2[g] == rec_bytes[g] for g in (1, 4, 7))
    # one member replaced by pg_job_record_plan: the other members keep the shared plan and their bytes
    by_chain[5] = plans[2]
    job.record_plan(5, plans[2])
    rec_3, gl_3 = cohort.check_against_the_model(by_chain, "one member replaced")
    assert rec_3[5] == rec_bytes[5] and gl_3[5] == gl_bytes[5]
    assert all(rec_3[g] == rec_2[g] and gl_3[g] == gl_2[g] for g in range(NS * NC) if g != 5)
    # the last references to the shared plan go one by one; the job goes on
    job.record_plan(2, plans[2])
    job.record_plan(8, plans[2])
    assert [r.tobytes() for r in job.record_calls()] == rec_bytes and [x.tobytes() for x in job.record_gl()] == gl_bytes
    job.close()
