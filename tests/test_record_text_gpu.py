"""The record text through a job (pg_job_record_text and its fetches; k_rtext_* of pangenie_amd/csrc/pg_record_text.hip): the
bytes of the GT:GQ:GL:KC column of every record of every chain against the text put together in Python
(tests/record_text_util.py) from the job's OWN record calls, record GLs and pg_job_fetch's coverage / n_kmers — byte for byte,
with ignore_imputed off and on.  A cohort of 2 samples x 2 contigs x 300 bubbles, a fifth of them multiallelic, a twentieth
without k-mers (so `.:.:` occurs under ignore_imputed), random plans of 1-3 records a bubble with a tenth of the record alleles
undefined.  The only records left out are those of fewer than three values — predicted from the plan — since the seeds give no
deferred call and no deferred value, which is asserted.  Then: a chain without a kept column (KC 0, UK 0), a contig without a
plan, the packed fetch, the device pointers, what makes the text stale, and the refusals.  (Deferred calls and values inside a
job's packed text: tests/test_regime_consumers_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.record_calls_util import random_plan
from tests.record_gl_util import is_deferred
from tests.record_text_util import DEFERRED, OK, assert_text, expected_text

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
SEED = 9300


def fields_of(job, c, plan):
    """what the text of chain c is made from, fetched from the job: calls, GL offsets and values, KC and UK per record"""
    rec, gl = calls.fetch_record_calls(job, c), calls.fetch_record_gl(job, c)
    res = job.fetch(c)
    rec_var = np.repeat(np.arange(plan.n_variants), np.diff(plan.rec_off.astype(np.int64)))
    return rec, calls.record_gl_offsets(plan), gl, res.coverage[rec_var], res.n_kmers[rec_var]


def check_chain(job, c, plan, ignore_imputed, got):
    """got = (off, bytes) of chain c; answers (records of the host's, records printed as .:.:)"""
    rec, gl_off, gl, kc, uk = fields_of(job, c, plan)
    assert not is_deferred(gl).any() and not ((rec["flags"] & 0xFF) == DEFERRED).any()
    no_call = (uk == 0).astype(np.uint8) if ignore_imputed else None
    want_off, want_text, hosts = expected_text(rec, gl_off, gl, kc, no_call)
    assert np.array_equal(hosts, np.diff(gl_off.astype(np.int64)) < 3)   # predicted from the plan alone
    assert_text(got[0], got[1], want_off, want_text, ("chain", c, ignore_imputed))
    return int(hosts.sum()), want_text.count(b".:.:")


@pytest.fixture(scope="module")
def cohort():
    index = [synthetic_panel(300, 16, 20, seed=SEED + i, multiallelic_frac=0.2, zero_kmer_frac=0.05) for i in range(2)]
    samples = []
    for s in range(2):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=SEED + 10 + 2 * s + c) for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.n_chains == 4
    job.run()
    rng = np.random.default_rng(SEED + 1)
    plans = [random_plan(rng, ix) for ix in index]
    for c, p in enumerate(plans):
        job.record_plan(c, p)
    yield job, index, plans
    job.close()


@pytest.mark.parametrize("ignore_imputed", [False, True])
def test_the_text_is_the_fields_text(cohort, ignore_imputed):
    job, index, plans = cohort
    texts = job.record_text(ignore_imputed=ignore_imputed)   # (forms the record calls and the record GLs itself)
    assert len(texts) == 4 and job.record_text_ms() > 0.0
    hosts = dots = 0
    for c in range(4):
        h, d = check_chain(job, c, plans[c % 2], ignore_imputed, texts[c])
        hosts, dots = hosts + h, dots + d
    assert hosts > 0   # random_plan makes records of a single allele: one value
    # bubbles without k-mers carry calls: they print as .:.: only under ignore_imputed
    uk0_called = 0
    for c in range(4):
        rec, _, _, _, uk = fields_of(job, c, plans[c % 2])
        uk0_called += int((((rec["flags"] & 0xFF) == OK) & (uk == 0)).sum())
    assert uk0_called > 0
    other = sum(t.count(b".:.:") for _, t in job.record_text(ignore_imputed=not ignore_imputed))
    assert (dots > other) if ignore_imputed else (dots < other)
    # the packed fetch: the chains' texts end to end, absolute offsets, text_first from the lengths
    job.record_text(ignore_imputed=ignore_imputed)
    off, text, first = job.record_text_packed(ignore_imputed)
    assert text == b"".join(t for _, t in texts)
    assert first.tolist() == np.concatenate([[0], np.cumsum([len(t) for _, t in texts])]).tolist()
    assert off.tolist() == np.concatenate([o[:-1].astype(np.int64) + int(first[c]) for c, (o, _) in enumerate(texts)] + [[int(first[-1])]]).tolist()
    assert len(text) <= calls.record_text_bound(len(off) - 1, sum(int(calls.record_gl_offsets(p)[-1]) for p in plans) * 2)
    # the device pointers and the lengths the fetches ask for
    lib, err = job._lib, C.create_string_buffer(256)
    for c in range(4):
        d_off, d_text, n_rec, n_bytes = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        assert lib.pg_job_device_record_text(job.h, c, C.byref(d_off), C.byref(d_text), C.byref(n_rec), C.byref(n_bytes)) == 0
        assert n_rec.value == plans[c % 2].n_records and n_bytes.value == len(texts[c][1]) and d_off.value and d_text.value
    buf = np.zeros(len(text) + 8, np.uint8)
    assert lib.pg_job_fetch_record_text_packed(job.h, None, buf.ctypes.data, len(text) + 1, err, 256) == -1
    assert lib.pg_job_fetch_record_text(job.h, 1, None, buf.ctypes.data, len(texts[1][1]) - 1, err, 256) == -1
    assert lib.pg_job_fetch_record_text(job.h, 1, None, buf.ctypes.data, len(texts[1][1]), err, 256) == 0   # (off may be NULL)
    assert buf[:len(texts[1][1])].tobytes() == texts[1][1]
    assert lib.pg_job_fetch_record_text(job.h, 4, None, buf.ctypes.data, 0, err, 256) == -1


def test_stale_after_a_run_and_after_a_new_plan_then_equal_again(cohort):
    job, index, plans = cohort
    before = job.record_text()
    job.run()   # the same inputs again: the text of the run before is stale all the same
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_text(job, 0)
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_text_packed(job)
    assert e.value.code == -1
    d = C.c_void_p()
    assert job._lib.pg_job_device_record_text(job.h, 0, C.byref(d), None, None, None) == -1
    after = job.record_text()
    assert [t for _, t in after] == [t for _, t in before] and all(np.array_equal(a[0], b[0]) for a, b in zip(after, before))
    new = random_plan(np.random.default_rng(SEED + 2), index[1])
    job.record_plan(1, new)
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_text(job, 0)
    assert e.value.code == -1
    texts = job.record_text()
    for c in range(4):
        check_chain(job, c, new if c % 2 else plans[0], False, texts[c])
    assert texts[0][1] == before[0][1] and texts[1][1] != before[1][1]
    job.record_plan(1, plans[1])   # (as the other tests of the module expect it)
    again = job.record_text()
    assert [t for _, t in again] == [t for _, t in before]


def test_a_chain_without_a_kept_column_and_a_contig_without_a_plan():
    flat = synthetic_panel(60, 16, 20, seed=SEED + 20, multiallelic_frac=0.2)
    flat.path_allele[:] = 0   # every selected path carries the reference allele: no column is kept
    batches = [flat, synthetic_panel(300, 16, 20, seed=SEED + 21, multiallelic_frac=0.2), synthetic_panel(80, 16, 20, seed=SEED + 22)]
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    job.run()
    assert job.fetch(0).n_columns == 0 and job.fetch(1).n_columns > 0
    rng = np.random.default_rng(SEED + 23)
    plans = [random_plan(rng, batches[0]), random_plan(rng, batches[1])]
    job.record_plan(0, plans[0])
    job.record_plan(1, plans[1])   # (contig 2 has none)
    for ignore in (False, True):
        texts = job.record_text(ignore_imputed=ignore)
        assert len(texts[2][1]) == 0 and texts[2][0].tolist() == [0]   # left out, not an error
        for c in (0, 1):
            check_chain(job, c, plans[c], ignore, texts[c])
        # KC 0 everywhere on the chain without a column although its coverage array holds the sample's; UK 0 too: all .:.: when imputed calls are ignored
        off, text = texts[0]
        recs = [text[int(off[r]):int(off[r + 1])] for r in range(plans[0].n_records) if off[r + 1] > off[r]]
        assert recs and all(t.endswith(b":0") for t in recs) and batches[0].coverage.min() > 0
        assert all(t.startswith(b".:.:") for t in recs) if ignore else any(t.startswith(b"0/0:10000:") for t in recs)
    off, text, first = job.record_text_packed()
    assert first[2] == first[3] == len(text) and len(off) == plans[0].n_records + plans[1].n_records + 1
    job.close()


def test_refusals():
    b = synthetic_panel(40, 16, 20, seed=SEED + 30)
    t = hmm.ProbabilityTable(*ARGS)
    plan = random_plan(np.random.default_rng(SEED + 31), b)
    job = hmm.Job.cohort([b], [tuple([x] for x in synthetic_sample_counts(b, seed=SEED + 32))], t, hmm.make_params(1.26, False, 1e-5))
    job.record_plan(0, plan)
    with pytest.raises(hmm.PanGenieError) as e:   # before pg_job_run
        job.record_text()
    assert e.value.code == -1
    job.run()
    job.record_calls()
    job.record_gl()
    with pytest.raises(hmm.PanGenieError) as e:   # the two families do not stand in for the text
        calls.fetch_record_text(job, 0)
    assert e.value.code == -1
    first = job.record_text(0)
    check_chain(job, 0, plan, False, first)
    # a new batch of samples (here: the same again) invalidates the run
    job.upload_begin()
    job.upload_end()
    with pytest.raises(hmm.PanGenieError) as e:
        job.record_text()
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_text(job, 0)
    assert e.value.code == -1
    job.run()
    assert job.record_text(0)[1] == first[1]
    # an allele id of the index outside a record's map
    job.record_plan(0, calls.RecordPlan.from_records([[([0], [True])] for _ in range(40)]))
    with pytest.raises(hmm.PanGenieError) as e:
        job.record_text()
    assert e.value.code == -1
    job.record_plan(0, plan)
    assert job.record_text(0)[1] == first[1]
    job.close()
    job = hmm.Job([b], t, hmm.make_params(1.26, False, 1e-5, run_genotyping=False, run_phasing=True))
    job.run()
    with pytest.raises(hmm.PanGenieError) as e:   # a job without run_genotyping has no bins
        job.record_text()
    assert e.value.code == -1
    job.close()
