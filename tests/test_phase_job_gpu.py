"""The phasing column through a job (pg_job_record_phase, pg_job_phased_text, pg_job_phased_lines and their fetches; k_rphase and
k_ptext_* of pangenie_amd/csrc/pg_phase_text.hip, the joiner of pg_record_lines.hip) against the Python mirror of the rule
(tests/phase_util.py) over pg_job_fetch's OWN haplotypes, kept flags, n_kmers and coverage: a phasing-only chain of 60 variants
at 16 paths and one at 30, the same chain with run_genotyping too in both sweep modes, a chain with variants but no column (UK =
KC = 0), ignore_imputed off and on; a cohort of 3 samples x 2 contigs whose phased lines are the plain join of its own phased
text behind random prefixes, with the bound reached exactly, the packed fetch and the device pointers; every refusal and what
makes phase, text and lines stale."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.phase_util import UNDEFINED, as_pairs, job_mirror
from tests.record_calls_util import random_plan

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
SEED = 9900
S, NC = 3, 2


def params(genotyping, phasing=True):
    return hmm.make_params(1.26, False, 1e-5, run_genotyping=genotyping, run_phasing=phasing)


def check_chain(job, c, plan, run_genotyping, ignore_imputed, phase, text):
    """phase / text = what the job answered for chain c; answers the mirror's (phase, bytes)"""
    want_phase, want_off, want_text = job_mirror(job, c, plan, run_genotyping, ignore_imputed)
    assert as_pairs(phase).tolist() == want_phase.tolist(), ("phase of chain", c)
    assert text[0].astype(np.int64).tolist() == want_off.tolist() and text[1] == want_text, ("text of chain", c, ignore_imputed)
    return want_phase, want_text


def panel(V, H, seed):
    # a third of the bubbles multiallelic, a tenth without k-mers (./. under ignore_imputed); every thirteenth bubble has the
    # reference allele on every path and so no column: the column count stays below the bubble count
    b = synthetic_panel(V, H, 20, seed=seed, multiallelic_frac=0.3, zero_kmer_frac=0.1)
    b.path_allele.reshape(V, H)[5::13] = 0
    return b


@pytest.mark.parametrize("H", [16, 30])
@pytest.mark.parametrize("ignore_imputed", [False, True])
def test_a_phasing_only_chain(H, ignore_imputed):
    b = panel(60, H, SEED + H)
    plan = random_plan(np.random.default_rng(SEED + 1), b, undefined=0.3)
    job = hmm.Job([b], hmm.ProbabilityTable(*ARGS), params(False))
    job.run()
    job.record_plan(0, plan)
    phase = job.record_phase(0)
    text = job.phased_text(0, ignore_imputed=ignore_imputed)
    assert job.record_phase_ms() > 0.0 and job.phased_text_ms() > 0.0
    want_phase, want_text = check_chain(job, 0, plan, False, ignore_imputed, phase, text)
    res = job.fetch(0)
    assert 0 < res.n_columns < 60 and (res.haplotype_1 > 0).any()
    # no likelihoods anywhere: a record with undefined alleles prints 0 or . and nothing else
    some = np.array([(plan.record(r)[1] == UNDEFINED).any() for r in range(plan.n_records)])
    assert some.any() and np.isin(want_phase[some], [0, UNDEFINED]).all() and (want_phase[~some] > 0).any()
    # UK and KC are set at the COLUMN index: the bubbles behind the column count print KC 0 (and ./. when imputed calls are ignored)
    rec_var = np.repeat(np.arange(60), np.diff(plan.rec_off.astype(np.int64)))
    tail = [text[1][int(text[0][r]):int(text[0][r + 1])] for r in np.nonzero(rec_var >= res.n_columns)[0]]
    assert tail and all(t.endswith(b":0") for t in tail) and b.coverage.min() > 0
    assert all(t.startswith(b"./.") for t in tail) == ignore_imputed
    job.close()


@pytest.mark.parametrize("mode", ["chunked", "fused"])
def test_the_same_chain_with_genotyping_too(mode, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", mode)
    b = panel(60, 16, SEED + 16)
    plan = random_plan(np.random.default_rng(SEED + 1), b, undefined=0.3)
    job = hmm.Job([b], hmm.ProbabilityTable(*ARGS), params(True))
    job.run()
    job.record_plan(0, plan)
    for ignore in (False, True):
        text = job.phased_text(0, ignore_imputed=ignore)   # (forms the record phase itself)
        want_phase, _ = check_chain(job, 0, plan, True, ignore, calls.fetch_record_phase(job, 0), text)
    # kept bubbles hold likelihoods: there a defined haplotype of a record with undefined alleles keeps its number
    res = job.fetch(0)
    rec_var = np.repeat(np.arange(60), np.diff(plan.rec_off.astype(np.int64)))
    some = np.array([(plan.record(r)[1] == UNDEFINED).any() for r in range(plan.n_records)])
    assert ((want_phase[some & (res.kept[rec_var] != 0)] > 0) & (want_phase[some & (res.kept[rec_var] != 0)] != UNDEFINED)).any()
    # every bubble reports its own KC and UK: the coverage of the last one too
    assert text[1].endswith(b":%d" % int(res.coverage[-1])) and res.coverage[-1] > 0 and res.n_columns < 60
    # the record text of the same job is its own family: both stand side by side
    assert len(job.record_text(0)[1]) > 0 and calls.fetch_phased_text(job, 0)[1] == text[1]
    job.close()


def test_a_chain_with_variants_but_no_column_and_a_contig_without_a_plan():
    flat = panel(60, 16, SEED + 20)
    flat.path_allele[:] = 0   # every selected path carries the reference allele: no column is kept
    batches = [flat, panel(60, 16, SEED + 21), panel(40, 16, SEED + 22)]
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), params(False))
    job.run()
    assert job.fetch(0).n_columns == 0 and job.fetch(1).n_columns > 0
    rng = np.random.default_rng(SEED + 23)
    plans = [random_plan(rng, batches[0]), random_plan(rng, batches[1])]
    job.record_plan(0, plans[0])
    job.record_plan(1, plans[1])   # (contig 2 has none)
    for ignore in (False, True):
        texts = job.phased_text(ignore_imputed=ignore)
        phases = calls.fetch_record_phase_all(job)
        assert len(texts[2][1]) == 0 and texts[2][0].tolist() == [0] and len(phases[2]) == 0   # left out, not an error
        for c in (0, 1):
            check_chain(job, c, plans[c], False, ignore, phases[c], texts[c])
        off, text = texts[0]
        recs = [text[int(off[r]):int(off[r + 1])] for r in range(plans[0].n_records)]
        assert all(t == (b"./.:0" if ignore else t) and t.endswith(b":0") for t in recs) and batches[0].coverage.min() > 0
    off, text, rf, tf = job.phased_text_packed()
    assert tf[2] == tf[3] == len(text) and rf.tolist() == [0, plans[0].n_records, plans[0].n_records + plans[1].n_records, plans[0].n_records + plans[1].n_records]
    assert len(off) == int(rf[-1]) + 1 and int(off[-1]) == len(text)
    job.close()


# ---- a cohort: text, lines, packed fetches, device pointers, staleness ---------------------------------------------------
def random_prefix(rng, R):
    lens = rng.integers(0, 80, R)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return off, rng.integers(0, 256, int(off[-1]), dtype=np.uint8)


def cut(p, r):
    off, data = p
    data = data.tobytes() if isinstance(data, np.ndarray) else data
    return data[int(off[r]):int(off[r + 1])]


def joined(prefix, texts):
    """(off, bytes) of one index contig: the rule of the lines, as plain concatenation"""
    lines = [cut(prefix, r) + b"".join(b"\t" + cut(t, r) for t in texts) + b"\n" for r in range(len(prefix[0]) - 1)]
    return np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.uint64), b"".join(lines)


@pytest.fixture(scope="module")
def cohort():
    index = [panel(120, 16, SEED + 30 + i) for i in range(NC)]
    samples = []
    for s in range(S):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=SEED + 40 + NC * s + c) for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*ARGS), params(False))
    assert job.n_chains == S * NC
    job.run()
    rng = np.random.default_rng(SEED + 31)
    plans = [random_plan(rng, ix, undefined=0.3) for ix in index]
    prefixes = [random_prefix(rng, p.n_records) for p in plans]
    for c, p in enumerate(plans):
        job.record_plan(c, p)
        job.phased_line_prefix(c, *prefixes[c])
    yield job, index, plans, prefixes
    job.close()


@pytest.mark.parametrize("ignore_imputed", [False, True])
def test_a_cohorts_text_and_its_lines(cohort, ignore_imputed):
    job, index, plans, prefixes = cohort
    texts = job.phased_text(ignore_imputed=ignore_imputed)
    phases = calls.fetch_record_phase_all(job)
    assert len(texts) == S * NC
    for c in range(S * NC):
        check_chain(job, c, plans[c % NC], False, ignore_imputed, phases[c], texts[c])
    assert (b"./." in b"".join(t for _, t in texts)) == ignore_imputed
    assert texts[0][1] != texts[NC][1]   # (the samples differ: coverage, haplotypes)
    # the packed text: the chains' texts end to end, absolute offsets
    off, text, rf, tf = job.phased_text_packed(ignore_imputed)
    assert text == b"".join(t for _, t in texts)
    assert tf.tolist() == np.concatenate([[0], np.cumsum([len(t) for _, t in texts])]).tolist()
    assert rf.tolist() == np.concatenate([[0], np.cumsum([plans[c % NC].n_records for c in range(S * NC)])]).tolist()
    assert off.tolist() == np.concatenate([o[:-1].astype(np.int64) + int(tf[c]) for c, (o, _) in enumerate(texts)] + [[int(tf[-1])]]).tolist()
    assert len(text) <= calls.phase_text_bound(len(off) - 1)
    lib, err = job._lib, C.create_string_buffer(256)
    for c in range(S * NC):
        d_off, d_text, n_rec, n_bytes, d_ph, n_ph = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        assert lib.pg_job_device_phased_text(job.h, c, C.byref(d_off), C.byref(d_text), C.byref(n_rec), C.byref(n_bytes)) == 0
        assert n_rec.value == plans[c % NC].n_records and n_bytes.value == len(texts[c][1]) and d_off.value and d_text.value
        assert lib.pg_job_device_record_phase(job.h, c, C.byref(d_ph), C.byref(n_ph)) == 0 and n_ph.value == plans[c % NC].n_records and d_ph.value
    assert lib.pg_job_device_phased_text(job.h, S * NC, None, None, None, None) == -1 and lib.pg_job_device_record_phase(job.h, S * NC, None, None) == -1
    buf = np.zeros(len(text) + 8, np.uint8)
    assert lib.pg_job_fetch_phased_text_packed(job.h, None, buf.ctypes.data, len(text) + 1, err, 256) == -1
    assert lib.pg_job_fetch_phased_text(job.h, 1, None, buf.ctypes.data, len(texts[1][1]), err, 256) == 0   # (off may be NULL)
    assert buf[:len(texts[1][1])].tobytes() == texts[1][1]
    # the lines: the plain join of the job's own text behind the prefixes, sample s in column s
    want = [joined(prefixes[k], [texts[s * NC + k] for s in range(S)]) for k in range(NC)]
    got = job.phased_lines()
    assert len(got) == NC and job.phased_lines_ms() > 0.0
    for k in range(NC):
        assert got[k][0].tolist() == want[k][0].tolist() and got[k][1] == want[k][1], k
    one = job.phased_lines(1)
    assert one[1] == want[1][1] and one[0].tolist() == want[1][0].tolist()
    loff, lines, line_first, byte_first = job.phased_lines_packed()
    assert lines == b"".join(w[1] for w in want)
    assert line_first.tolist() == [0, plans[0].n_records, plans[0].n_records + plans[1].n_records]
    assert byte_first.tolist() == [0, len(want[0][1]), len(want[0][1]) + len(want[1][1])]
    assert loff.tolist() == np.concatenate([want[0][0][:-1].astype(np.int64), want[1][0].astype(np.int64) + len(want[0][1])]).tolist()
    # no line is the host's: the bound is reached exactly
    bound = sum(calls.record_lines_bound(plans[k].n_records, S, int(prefixes[k][0][-1]), sum(len(texts[s * NC + k][1]) for s in range(S))) for k in range(NC))
    assert len(lines) == bound
    n = C.c_uint64(0)
    assert lib.pg_job_phased_lines_first(job.h, C.byref(n), None, None, err, 256) == 0 and n.value == NC
    d0 = None
    for k in range(NC):
        d_off, d_text, n_l, n_b = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        assert lib.pg_job_device_phased_lines(job.h, k, C.byref(d_off), C.byref(d_text), C.byref(n_l), C.byref(n_b)) == 0
        assert n_l.value == plans[k].n_records and n_b.value == len(want[k][1]) and d_off.value and d_text.value
        d0 = d_text.value if k == 0 else d0
        assert d_text.value - d0 == int(byte_first[k])
    assert lib.pg_job_device_phased_lines(job.h, NC, None, None, None, None) == -1
    assert lib.pg_job_fetch_phased_lines_packed(job.h, None, buf.ctypes.data, len(lines) + 1, err, 256) == -1
    assert lib.pg_job_fetch_phased_lines(job.h, NC, None, buf.ctypes.data, 0, err, 256) == -1
    # the prefixes of the record lines are another family: this job has none of those, and no record text to join
    with pytest.raises(hmm.PanGenieError) as e:
        job.record_lines()
    assert e.value.code == -1


def refused(call, *args):
    with pytest.raises(hmm.PanGenieError) as e:
        call(*args)
    assert e.value.code == -1


def test_stale_after_a_run_a_new_plan_and_a_new_prefix(cohort):
    job, index, plans, prefixes = cohort
    before_text = job.phased_text()
    before_lines = job.phased_lines()
    job.run()   # the same inputs again: what was formed from the run before is stale all the same
    for fetch in (calls.fetch_record_phase, calls.fetch_phased_text, calls.fetch_phased_lines):
        refused(fetch, job, 0)
    refused(calls.fetch_phased_text_packed, job)
    refused(calls.fetch_phased_lines_packed, job)
    refused(calls.form_phased_lines, job)   # (it does not form the text itself)
    d = C.c_void_p()
    assert job._lib.pg_job_device_phased_text(job.h, 0, C.byref(d), None, None, None) == -1
    assert job._lib.pg_job_device_phased_lines(job.h, 0, C.byref(d), None, None, None) == -1
    assert job._lib.pg_job_device_record_phase(job.h, 0, C.byref(d), None) == -1
    after = job.phased_text()
    assert [t for _, t in after] == [t for _, t in before_text]
    assert [l for _, l in job.phased_lines()] == [l for _, l in before_lines]
    # forming the text again makes the lines stale although the bytes are the same
    job.phased_text()
    refused(calls.fetch_phased_lines, job, 0)
    assert [l for _, l in job.phased_lines()] == [l for _, l in before_lines]
    # a new prefix: the lines alone
    new_prefix = random_prefix(np.random.default_rng(SEED + 50), plans[1].n_records)
    job.phased_line_prefix(1, *new_prefix)
    refused(calls.fetch_phased_lines, job, 0)
    assert calls.fetch_phased_text(job, 1)[1] == before_text[1][1]
    lines = job.phased_lines()
    assert lines[0][1] == before_lines[0][1] and lines[1][1] == joined(new_prefix, [after[s * NC + 1] for s in range(S)])[1]
    # a new plan: phase, text and lines, and the contig's prefix is dropped
    new = random_plan(np.random.default_rng(SEED + 51), index[1], undefined=0.3)
    job.record_plan(1, new)
    for fetch in (calls.fetch_record_phase, calls.fetch_phased_text, calls.fetch_phased_lines):
        refused(fetch, job, 0)
    texts = job.phased_text()
    for c in range(S * NC):
        check_chain(job, c, new if c % NC else plans[0], False, False, calls.fetch_record_phase(job, c), texts[c])
    assert texts[0][1] == before_text[0][1] and texts[1][1] != before_text[1][1]
    lines = job.phased_lines()
    assert lines[0][1] == before_lines[0][1] and len(lines[1][1]) == 0   # (contig 1 has no prefix any more: left out)
    job.record_plan(1, plans[1])   # (as the other tests of the module expect it)
    job.phased_line_prefix(1, *prefixes[1])
    assert [t for _, t in job.phased_text()] == [t for _, t in before_text]
    assert [l for _, l in job.phased_lines()] == [l for _, l in before_lines]


def test_stale_after_a_new_index():
    b = panel(60, 16, SEED + 70)
    plan = random_plan(np.random.default_rng(SEED + 71), b, undefined=0.3)
    prefix = random_prefix(np.random.default_rng(SEED + 72), plan.n_records)
    job = hmm.Job([b], hmm.ProbabilityTable(*ARGS), params(False))
    job.run()
    job.record_plan(0, plan)
    job.phased_line_prefix(0, *prefix)
    text = job.phased_text(0)
    lines = job.phased_lines(0)
    assert lines[1] == joined(prefix, [text])[1]
    job.upload()   # a plain job sends every array again, the index too: new allele ids as far as the job knows
    job.run()
    for fetch in (calls.fetch_record_phase, calls.fetch_phased_text, calls.fetch_phased_lines):   # stale although the run is new
        refused(fetch, job, 0)
    refused(calls.form_phased_lines, job)
    check_chain(job, 0, plan, False, False, job.record_phase(0), job.phased_text(0))   # (the ids are checked again, the plan stands)
    assert calls.fetch_phased_text(job, 0)[1] == text[1]
    assert len(job.phased_lines(0)[1]) == 0   # the index's prefix was dropped with it: the contig is left out ...
    job.phased_line_prefix(0, *prefix)
    assert job.phased_lines(0)[1] == lines[1]   # ... until its fixed columns are sent again
    job.close()


def test_refusals():
    b = panel(40, 16, SEED + 60)
    t = hmm.ProbabilityTable(*ARGS)
    plan = random_plan(np.random.default_rng(SEED + 61), b)
    job = hmm.Job.cohort([b], [tuple([x] for x in synthetic_sample_counts(b, seed=SEED + 62))], t, params(False))
    job.record_plan(0, plan)
    for form in (job.record_phase, job.phased_text, job.phased_lines):   # before pg_job_run
        refused(form)
    job.run()
    job.record_phase()
    refused(calls.fetch_phased_text, job, 0)   # the phase does not stand in for the text
    refused(job.phased_lines)                  # ... nor is there a text to join
    first = job.phased_text(0)
    check_chain(job, 0, plan, False, False, calls.fetch_record_phase(job, 0), first)
    prefix = random_prefix(np.random.default_rng(SEED + 63), plan.n_records)
    lib, err = job._lib, C.create_string_buffer(256)
    assert lib.pg_job_phased_line_prefix(job.h, 1, prefix[0].ctypes.data, prefix[1].ctypes.data, err, 256) == -1   # no such index contig
    assert lib.pg_job_phased_line_prefix(job.h, 0, None, prefix[1].ctypes.data, err, 256) == -1
    bad = prefix[0].copy()
    bad[0] = 1
    assert lib.pg_job_phased_line_prefix(job.h, 0, bad.ctypes.data, prefix[1].ctypes.data, err, 256) == -1
    job.phased_line_prefix(0, *prefix)
    lines = job.phased_lines(0)
    assert lines[1] == joined(prefix, [first])[1]
    # a new batch of samples (here: the same again) invalidates the run
    job.upload_begin()
    job.upload_end()
    for form in (job.record_phase, job.phased_text, job.phased_lines):
        refused(form)
    for fetch in (calls.fetch_record_phase, calls.fetch_phased_text, calls.fetch_phased_lines):
        refused(fetch, job, 0)
    job.run()
    assert job.phased_text(0)[1] == first[1] and job.phased_lines(0)[1] == lines[1]
    # an allele id of the index outside a record's map: the id check runs before the first formation under the new plan
    job.record_plan(0, calls.RecordPlan.from_records([[([0], [True])] for _ in range(40)]))
    refused(job.record_phase)
    refused(job.phased_text)
    job.record_plan(0, plan)
    assert job.phased_text(0)[1] == first[1]
    job.close()
    # a job without run_phasing has no haplotypes
    job = hmm.Job([b], t, params(True, phasing=False))
    job.run()
    job.record_plan(0, plan)
    for form in (job.record_phase, job.phased_text, job.phased_lines):
        refused(form)
    assert len(job.record_text(0)[1]) > 0   # (its record text is there as ever)
    job.close()
    # ... and a phasing-only job still has no bins for the record text
    job = hmm.Job([b], t, params(False))
    job.run()
    job.record_plan(0, plan)
    refused(job.record_text)
    assert len(job.phased_text(0)[1]) > 0
    job.close()
