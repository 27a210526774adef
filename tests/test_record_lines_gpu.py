"""The record lines through a job (pg_job_line_prefix, pg_job_record_lines and the fetches; k_rlines_* of
pangenie_amd/csrc/pg_record_lines.hip): a cohort of 3 samples x 2 contigs x 300 bubbles at 16 paths, a fifth of the bubbles
multiallelic, a twentieth without k-mers, random plans, and RANDOM BYTES per record as prefixes.  Every line is compared byte
for byte with the join, in Python, of the prefix and the job's OWN record_text of the contig's three chains — ignore_imputed
off and on.  The lines left to the host are exactly the records whose plan gives fewer than three values; at least a third of
all lines carry text.  Then the packed fetch and _first, the device pointers, a job of three single chains of which one has no
prefix and one no plan, what makes the lines stale, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.record_calls_util import random_plan

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
SEED = 9500
S, NC = 3, 2


def random_prefix(rng, R):
    lens = rng.integers(0, 80, R)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return off, rng.integers(0, 256, int(off[-1]), dtype=np.uint8)


def cut(p, r):
    off, data = p
    data = data.tobytes() if isinstance(data, np.ndarray) else data
    return data[int(off[r]):int(off[r + 1])]


def joined(prefix, texts):
    """(off, bytes, lines of the host's) of one index contig: the rule, as plain concatenation"""
    R = len(prefix[0]) - 1
    lines = []
    for r in range(R):
        ts = [cut(t, r) for t in texts]
        lines.append(b"" if any(len(t) == 0 for t in ts) else cut(prefix, r) + b"".join(b"\t" + t for t in ts) + b"\n")
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.uint64)
    return off, b"".join(lines), np.array([len(l) == 0 for l in lines])


@pytest.fixture(scope="module")
def cohort():
    index = [synthetic_panel(300, 16, 20, seed=SEED + i, multiallelic_frac=0.2, zero_kmer_frac=0.05) for i in range(NC)]
    samples = []
    for s in range(S):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=SEED + 10 + NC * s + c) for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.n_chains == S * NC
    job.run()
    rng = np.random.default_rng(SEED + 1)
    plans = [random_plan(rng, ix) for ix in index]
    prefixes = [random_prefix(rng, p.n_records) for p in plans]
    for c, p in enumerate(plans):
        job.record_plan(c, p)
        job.line_prefix(c, *prefixes[c])
    yield job, index, plans, prefixes
    job.close()


def want_of(job, prefixes, ignore_imputed):
    """forms the text and answers the expected (off, bytes, hosts) per index contig from the job's own texts"""
    texts = job.record_text(ignore_imputed=ignore_imputed)
    return [joined(prefixes[k], [texts[s * NC + k] for s in range(S)]) for k in range(NC)], texts


@pytest.mark.parametrize("ignore_imputed", [False, True])
def test_the_lines_are_the_join_of_the_jobs_own_text(cohort, ignore_imputed):
    job, index, plans, prefixes = cohort
    want, texts = want_of(job, prefixes, ignore_imputed)
    got = job.record_lines()
    assert len(got) == NC and job.record_lines_ms() > 0.0
    n_lines = n_text = 0
    for k in range(NC):
        assert got[k][0].tolist() == want[k][0].tolist(), k
        assert got[k][1] == want[k][1], k
        # the lines of the host's are exactly the records whose plan gives fewer than three values
        few = np.diff(calls.record_gl_offsets(plans[k]).astype(np.int64)) < 3
        assert np.array_equal(want[k][2], few) and few.any()
        assert np.array_equal(np.diff(got[k][0].astype(np.int64)) == 0, few)
        n_lines, n_text = n_lines + len(few), n_text + int((~few).sum())
    assert 3 * n_text >= n_lines   # at least a third of all lines carry text
    if ignore_imputed:
        assert any(b"\t.:.:" in w[1] for w in want)
    # one contig alone
    one = job.record_lines(1)
    assert one[1] == want[1][1] and one[0].tolist() == want[1][0].tolist()
    # the packed fetch and _first: the contigs' lines end to end, absolute offsets
    off, text, line_first, byte_first = job.record_lines_packed()
    assert text == b"".join(w[1] for w in want)
    assert line_first.tolist() == [0, plans[0].n_records, plans[0].n_records + plans[1].n_records]
    assert byte_first.tolist() == [0, len(want[0][1]), len(want[0][1]) + len(want[1][1])]
    assert off.tolist() == np.concatenate([want[0][0][:-1].astype(np.int64), want[1][0].astype(np.int64) + len(want[0][1])]).tolist()
    bound = sum(calls.record_lines_bound(plans[k].n_records, S, int(prefixes[k][0][-1]), sum(len(texts[s * NC + k][1]) for s in range(S))) for k in range(NC))
    assert len(text) < bound   # (some lines are the host's)
    lib, err = job._lib, C.create_string_buffer(256)
    n = C.c_uint64(0)
    assert lib.pg_job_record_lines_first(job.h, C.byref(n), None, None, err, 256) == 0 and n.value == NC
    # the device pointers and the lengths the fetches ask for
    d0 = None
    for k in range(NC):
        d_off, d_text, n_l, n_b = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        assert lib.pg_job_device_record_lines(job.h, k, C.byref(d_off), C.byref(d_text), C.byref(n_l), C.byref(n_b)) == 0
        assert n_l.value == plans[k].n_records and n_b.value == len(want[k][1]) and d_off.value and d_text.value
        d0 = d_text.value if k == 0 else d0
        assert d_text.value - d0 == int(byte_first[k])
    assert lib.pg_job_device_record_lines(job.h, NC, None, None, None, None) == -1
    buf = np.zeros(len(text) + 8, np.uint8)
    assert lib.pg_job_fetch_record_lines_packed(job.h, None, buf.ctypes.data, len(text) + 1, err, 256) == -1
    assert lib.pg_job_fetch_record_lines(job.h, 1, None, buf.ctypes.data, len(want[1][1]) - 1, err, 256) == -1
    assert lib.pg_job_fetch_record_lines(job.h, 1, None, buf.ctypes.data, len(want[1][1]), err, 256) == 0   # (off may be NULL)
    assert buf[:len(want[1][1])].tobytes() == want[1][1]
    assert lib.pg_job_fetch_record_lines(job.h, NC, None, buf.ctypes.data, 0, err, 256) == -1


def assert_stale(job):
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_lines(job, 0)
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_lines_packed(job)
    assert e.value.code == -1
    d = C.c_void_p()
    assert job._lib.pg_job_device_record_lines(job.h, 0, C.byref(d), None, None, None) == -1


def test_stale_after_a_run_a_plan_a_prefix_and_another_text_then_equal_again(cohort):
    job, index, plans, prefixes = cohort
    want, _ = want_of(job, prefixes, False)
    before = job.record_lines()
    assert [b[1] for b in before] == [w[1] for w in want]
    # a run: the text is stale, and the lines with it; the text alone does not bring them back
    job.run()
    assert_stale(job)
    with pytest.raises(hmm.PanGenieError) as e:   # (the lines do not form the text themselves)
        job.record_lines()
    assert e.value.code == -1
    job.record_text()
    assert_stale(job)
    assert [a[1] for a in job.record_lines()] == [b[1] for b in before]
    # a new plan drops the contig's prefix: that contig is left out until it has one again
    new = random_plan(np.random.default_rng(SEED + 2), index[1])
    job.record_plan(1, new)
    assert_stale(job)
    job.record_text()
    left_out = job.record_lines()
    assert left_out[0][1] == before[0][1] and left_out[1][1] == b"" and left_out[1][0].tolist() == [0]
    new_prefix = random_prefix(np.random.default_rng(SEED + 3), new.n_records)
    job.line_prefix(1, *new_prefix)
    assert_stale(job)
    got = job.record_lines()
    texts = job.record_text()
    w1 = joined(new_prefix, [texts[s * NC + 1] for s in range(S)])
    assert got[0][1] == before[0][1] and got[1][1] == w1[1] and got[1][0].tolist() == w1[0].tolist()
    job.record_plan(1, plans[1])   # (as the other tests of the module expect it)
    job.line_prefix(1, *prefixes[1])
    job.record_text()
    assert [a[1] for a in job.record_lines()] == [b[1] for b in before]
    # a new prefix alone
    other = random_prefix(np.random.default_rng(SEED + 4), plans[0].n_records)
    job.line_prefix(0, *other)
    assert_stale(job)
    got = job.record_lines()
    assert got[0][1] == joined(other, [job.record_text()[s * NC] for s in range(S)])[1] and got[1][1] == before[1][1]
    job.line_prefix(0, *prefixes[0])
    assert [a[1] for a in job.record_lines()] == [b[1] for b in before]
    # the text formed with the other ignore_imputed
    want_ii, _ = want_of(job, prefixes, True)
    assert_stale(job)
    assert [a[1] for a in job.record_lines()] == [w[1] for w in want_ii]
    job.record_text(ignore_imputed=False)
    assert_stale(job)
    assert [a[1] for a in job.record_lines()] == [b[1] for b in before]


def test_single_chains_one_without_a_prefix_and_one_without_a_plan():
    batches = [synthetic_panel(120, 16, 20, seed=SEED + 20 + i, multiallelic_frac=0.2) for i in range(3)]
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    job.run()
    rng = np.random.default_rng(SEED + 23)
    plans = [random_plan(rng, batches[0]), None, random_plan(rng, batches[2])]
    job.record_plan(0, plans[0])   # (no prefix)
    job.record_plan(2, plans[2])   # (contig 1 has no plan)
    prefix = random_prefix(rng, plans[2].n_records)
    job.line_prefix(2, *prefix)
    texts = job.record_text()
    got = job.record_lines()
    assert len(got) == 3
    for k in (0, 1):
        assert got[k][1] == b"" and got[k][0].tolist() == [0]   # left out, not an error
    want = joined(prefix, [texts[2]])   # single-member lines
    assert got[2][1] == want[1] and got[2][0].tolist() == want[0].tolist() and len(want[1]) > 0
    off, text, line_first, byte_first = job.record_lines_packed()
    assert text == want[1] and line_first.tolist() == [0, 0, 0, plans[2].n_records] and byte_first.tolist() == [0, 0, 0, len(want[1])]
    job.close()


def test_refusals():
    b = synthetic_panel(40, 16, 20, seed=SEED + 30)
    t = hmm.ProbabilityTable(*ARGS)
    plan = random_plan(np.random.default_rng(SEED + 31), b)
    rng = np.random.default_rng(SEED + 33)
    job = hmm.Job.cohort([b], [tuple([x] for x in synthetic_sample_counts(b, seed=SEED + 32))], t, hmm.make_params(1.26, False, 1e-5))
    prefix = random_prefix(rng, plan.n_records)
    with pytest.raises(hmm.PanGenieError) as e:   # a prefix before a plan
        job.line_prefix(0, *prefix)
    assert e.value.code == -1
    job.record_plan(0, plan)
    with pytest.raises(ValueError):               # a prefix with the wrong R
        job.line_prefix(0, *random_prefix(rng, plan.n_records + 1))
    bad = prefix[0].copy()
    bad[0] = 1
    with pytest.raises(hmm.PanGenieError) as e:   # offsets that do not start at 0
        job.line_prefix(0, bad, prefix[1])
    assert e.value.code == -1
    bad = prefix[0].copy()
    bad[1], bad[2] = max(int(bad[1]), int(bad[2])) + 1, min(int(bad[1]), int(bad[2]))
    with pytest.raises(hmm.PanGenieError) as e:   # ... or shrink
        job.line_prefix(0, bad, np.zeros(int(bad.max()) + 1, np.uint8))
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:   # an index contig the job does not have
        job.line_prefix(1, *prefix)
    assert e.value.code == -1
    job.line_prefix(0, *prefix)
    with pytest.raises(hmm.PanGenieError) as e:   # before pg_job_run
        job.record_lines()
    assert e.value.code == -1
    job.run()
    job.record_calls()
    job.record_gl()
    with pytest.raises(hmm.PanGenieError) as e:   # before the text is formed: the two families do not stand in for it
        job.record_lines()
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_lines(job, 0)
    assert e.value.code == -1
    text = job.record_text(0)
    got = job.record_lines(0)
    want = joined(prefix, [text])
    assert got[1] == want[1] and got[0].tolist() == want[0].tolist()
    lib, err = job._lib, C.create_string_buffer(256)
    buf = np.zeros(len(got[1]) + 8, np.uint8)
    assert lib.pg_job_fetch_record_lines(job.h, 0, None, buf.ctypes.data, len(got[1]) + 1, err, 256) == -1   # a fetch with a wrong length
    assert lib.pg_job_fetch_record_lines(job.h, 0, None, None, len(got[1]), err, 256) == -1
    job.close()
