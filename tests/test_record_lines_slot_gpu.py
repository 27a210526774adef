"""The record lines of jobs whose chains are index contigs of their own, over ONE slotted prefix per stride of chains
(pg_job_line_prefix_strided, pg_job_line_prefix_slotted, pg_job_record_lines; the SLOT instantiation of k_rlines_* of
pangenie_amd/csrc/pg_record_lines.hip).  (a) 3 x 2 chains over 2 panels, the three members of a stride
reduced to different paths: the same bubbles, allele ids of one id space, other k-mer counts per bubble.  (b) the same through
sampler.sample_cohort, 24 paths sampled to 5 and the reference path.  In both the test asserts that some record's UK differs
between two members of a stride, and every chain's lines are compared byte for byte with the join, in Python, of the chain's
OWN record_text and a prefix that carries the decimal n_kmers of pg_job_fetch at the slot.  (c) what makes the lines stale, and
that pg_job_line_prefix on one member changes that member alone.  (d) a plain and a slotted index contig in one job.  (e) the
refusals.  RANDOM BYTES as prefixes; the join has no arithmetic: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd import sampler as smp
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.record_calls_util import random_plan

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
SEED = 9900
NS, NC = 3, 2


def random_prefix(rng, R):
    """(off, bytes, slot): random bytes of 0 .. 79 per record; the slots at 0, at the end and inside"""
    lens = rng.integers(0, 80, R)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    kind = rng.integers(0, 3, R)
    slot = np.where(kind == 0, 0, np.where(kind == 1, lens, (rng.random(R) * (lens + 1)).astype(np.int64))).astype(np.uint32)
    return off, rng.integers(0, 256, int(off[-1]), dtype=np.uint8), slot


def cut(p, r):
    off, data = p[0], p[1]
    data = data.tobytes() if isinstance(data, np.ndarray) else data
    return data[int(off[r]):int(off[r + 1])]


def rec_var_of(plan):
    return np.repeat(np.arange(plan.n_variants), np.diff(plan.rec_off.astype(np.int64)))


def uk_of(job, g, plan):
    """UK of every record of chain g: pg_job_fetch's n_kmers of the record's bubble"""
    return job.fetch(g).n_kmers[rec_var_of(plan)].astype(np.int64)


def joined(prefix, uk, text):
    """(off, bytes, lines of the host's) of a chain that is an index contig of its own: the rule, as plain concatenation.
    uk None: a plain prefix."""
    R = len(prefix[0]) - 1
    lines = []
    for r in range(R):
        p, t = cut(prefix, r), cut(text, r)
        if uk is not None:
            at = int(prefix[2][r])
            p = p[:at] + str(int(uk[r])).encode() + p[at:]
        lines.append(b"" if len(t) == 0 else p + b"\t" + t + b"\n")
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.uint64)
    return off, b"".join(lines), np.array([len(l) == 0 for l in lines])


def lines_of(packed, ix):
    """(off relative to the contig's first byte, bytes) of index contig ix out of record_lines_packed()"""
    off, text, line_first, byte_first = packed
    l0, l1, b0, b1 = int(line_first[ix]), int(line_first[ix + 1]), int(byte_first[ix]), int(byte_first[ix + 1])
    o = off[l0:l1 + 1].astype(np.int64) - b0
    return o, text[b0:b1]


def assert_strides(job, plans, prefixes, ignore_imputed):
    """every chain's lines against its own text and its own UK; answers the UK per chain"""
    texts = job.record_text(ignore_imputed=ignore_imputed)
    packed = job.record_lines_packed()
    assert job.record_lines_ms() > 0.0
    uks, n_bytes = [], 0
    for g in range(NS * NC):
        c = g % NC
        uk = uk_of(job, g, plans[c])
        want = joined(prefixes[c], uk, texts[g])
        got = lines_of(packed, g)
        assert got[0].tolist() == want[0].tolist(), g
        assert got[1] == want[1], g
        # the lines of the host's are exactly the records whose text is empty
        empty = np.diff(texts[g][0].astype(np.int64)) == 0
        assert np.array_equal(np.diff(got[0]) == 0, empty) and np.array_equal(want[2], empty) and empty.any() and not empty.all()
        uks.append(uk)
        n_bytes += len(want[1])
    assert len(packed[1]) == n_bytes and packed[2].tolist() == np.concatenate([[0], np.cumsum([plans[g % NC].n_records for g in range(NS * NC)])]).tolist()
    bound = sum(calls.record_lines_bound_slotted(plans[g % NC].n_records, 1, int(prefixes[g % NC][0][-1]), len(texts[g][1])) for g in range(NS * NC))
    assert n_bytes < bound
    return uks


def assert_uk_differs_within_a_stride(uks):
    """otherwise one prefix with the number in its bytes would do, and the test would show nothing"""
    for c in range(NC):
        assert any((uks[c] != uks[s * NC + c]).any() for s in range(1, NS)), c


def attach(job, plans, prefixes):
    for c in range(NC):
        job.record_plan_strided(c, NC, plans[c])
        job.line_prefix_strided(c, NC, prefixes[c][0], prefixes[c][1], slot=prefixes[c][2])


@pytest.fixture(scope="module")
def strides():
    """3 x 2 single chains, chain s * NC + c = panel c with sample s's counts, reduced to 8 of its 16 paths (other ones per s)"""
    rng = np.random.default_rng(SEED)
    index = [synthetic_panel(300, 16, 20, seed=SEED + c, multiallelic_frac=0.2, zero_kmer_frac=0.05) for c in range(NC)]
    batches = []
    for s in range(NS):
        paths = np.sort(rng.choice(16, 8, replace=False))
        for c, ix in enumerate(index):
            counted = ix.with_counts(*synthetic_sample_counts(ix, seed=SEED + 10 + NC * s + c))
            batches.append(counted.update_paths(np.repeat(paths[:, None], ix.n_variants, axis=1)))
    for c in range(NC):   # one layout of bubbles, ids of one id space
        for s in range(1, NS):
            assert batches[s * NC + c].n_variants == batches[c].n_variants and set(batches[s * NC + c].allele_id) <= set(index[c].allele_id)
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.n_chains == NS * NC
    job.run()
    plans = [random_plan(rng, ix) for ix in index]
    prefixes = [random_prefix(rng, p.n_records) for p in plans]
    attach(job, plans, prefixes)
    yield job, index, plans, prefixes
    job.close()


@pytest.mark.parametrize("ignore_imputed", [False, True])
def test_a_stride_of_chains_shares_one_prefix_and_every_line_carries_its_own_uk(strides, ignore_imputed):
    job, index, plans, prefixes = strides
    uks = assert_strides(job, plans, prefixes, ignore_imputed)
    assert_uk_differs_within_a_stride(uks)
    assert any((uk == 0).any() for uk in uks) and any((uk >= 10).any() for uk in uks)   # one digit and two


def test_a_sampled_cohort_24_paths_to_5_and_the_reference():
    index = [synthetic_panel(300, 24, 20, seed=SEED + 40 + c, multiallelic_frac=0.3, max_alleles=8, zero_kmer_frac=0.05) for c in range(NC)]
    samples = []
    for s in range(NS):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=SEED + 50 + NC * s + c) for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    job, _, _ = smp.sample_cohort(index, samples, 5, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5), add_reference=True, want_paths=False)
    assert job.n_chains == NS * NC and all(b.n_paths == 6 for b in job.batches)
    job.run()
    rng = np.random.default_rng(SEED + 41)
    plans = [random_plan(rng, ix) for ix in index]
    prefixes = [random_prefix(rng, p.n_records) for p in plans]
    attach(job, plans, prefixes)
    for ignore_imputed in (False, True):
        uks = assert_strides(job, plans, prefixes, ignore_imputed)
        assert_uk_differs_within_a_stride(uks)   # (the reduced panels differ per sample)
    job.close()


def assert_stale(job):
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_lines(job, 0)
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:
        calls.fetch_record_lines_packed(job)
    assert e.value.code == -1
    d = C.c_void_p()
    assert job._lib.pg_job_device_record_lines(job.h, 0, C.byref(d), None, None, None) == -1


def test_stale_after_a_run_and_a_new_strided_prefix_and_a_prefix_on_one_member_changes_that_member_alone(strides):
    job, index, plans, prefixes = strides
    assert_strides(job, plans, prefixes, False)
    before = [lines_of(job.record_lines_packed(), g) for g in range(NS * NC)]
    # a run: the text is stale, and the lines with it; the text alone does not bring them back
    job.run()
    assert_stale(job)
    with pytest.raises(hmm.PanGenieError) as e:
        job.record_lines_packed()
    assert e.value.code == -1
    texts = job.record_text()
    assert_stale(job)
    assert [lines_of(job.record_lines_packed(), g)[1] for g in range(NS * NC)] == [b[1] for b in before]
    # a new strided prefix for contig 1: its three chains change, those of contig 0 do not
    other = random_prefix(np.random.default_rng(SEED + 2), plans[1].n_records)
    job.line_prefix_strided(1, NC, other[0], other[1], slot=other[2])
    assert_stale(job)
    packed = job.record_lines_packed()
    for g in range(NS * NC):
        want = joined(other, uk_of(job, g, plans[1]), texts[g]) if g % NC == 1 else before[g]
        assert lines_of(packed, g)[1] == want[1] and lines_of(packed, g)[0].tolist() == np.asarray(want[0]).tolist(), g
    # ... without slots: the stride's prefix as it is (the other stride still has slots: the same kernels carry both)
    job.line_prefix_strided(1, NC, other[0], other[1])
    assert_stale(job)
    packed = job.record_lines_packed()
    for g in range(NS * NC):
        want = joined(other, None, texts[g]) if g % NC == 1 else before[g]
        assert lines_of(packed, g)[1] == want[1], g
    job.line_prefix_strided(1, NC, prefixes[1][0], prefixes[1][1], slot=prefixes[1][2])
    assert [lines_of(job.record_lines_packed(), g)[1] for g in range(NS * NC)] == [b[1] for b in before]
    # pg_job_line_prefix on ONE member (chain 2: contig 0 of sample 1), plain and slotted: that member changes, nobody else
    mine = random_prefix(np.random.default_rng(SEED + 3), plans[0].n_records)
    for slot in (None, mine[2]):
        job.line_prefix(2, mine[0], mine[1], slot=slot)
        assert_stale(job)
        packed = job.record_lines_packed()
        for g in range(NS * NC):
            want = joined(mine, None if slot is None else uk_of(job, g, plans[0]), texts[g]) if g == 2 else before[g]
            assert lines_of(packed, g)[1] == want[1], (g, slot is None)
    # a new plan for that member drops its reference alone: it is left out, the stride's other members keep their prefix
    job.record_plan(2, plans[0])
    texts = job.record_text()
    packed = job.record_lines_packed()
    for g in range(NS * NC):
        assert lines_of(packed, g)[1] == (b"" if g == 2 else before[g][1]), g
    attach(job, plans, prefixes)   # (as the other tests of the module expect it)
    job.record_text()
    assert [lines_of(job.record_lines_packed(), g)[1] for g in range(NS * NC)] == [b[1] for b in before]


def test_a_plain_and_a_slotted_index_contig_in_one_job():
    batches = [synthetic_panel(700, 16, 20, seed=SEED + 20 + i, multiallelic_frac=0.2, zero_kmer_frac=0.05) for i in range(3)]
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    job.run()
    rng = np.random.default_rng(SEED + 23)
    plans = [random_plan(rng, b) for b in batches]
    prefixes = [random_prefix(rng, p.n_records) for p in plans]
    for k in range(3):
        job.record_plan(k, plans[k])
    job.line_prefix(0, prefixes[0][0], prefixes[0][1])                          # plain
    job.line_prefix(1, prefixes[1][0], prefixes[1][1], slot=prefixes[1][2])     # slotted
    job.line_prefix(2, prefixes[2][0], prefixes[2][1])                          # plain, behind the slotted one
    texts = job.record_text()
    packed = job.record_lines_packed()
    for k in range(3):
        want = joined(prefixes[k], uk_of(job, k, plans[k]) if k == 1 else None, texts[k])
        got = lines_of(packed, k)
        assert got[1] == want[1] and got[0].tolist() == want[0].tolist() and len(want[1]) > 0, k
        one = job.record_lines(k)
        assert one[1] == want[1] and one[0].tolist() == want[0].tolist(), k
    # with the slotted prefix gone the plain kernels run again: the plain contigs' bytes are the same
    job.line_prefix(1, prefixes[1][0], prefixes[1][1])
    again = job.record_lines_packed()
    for k in (0, 2):
        assert lines_of(again, k)[1] == lines_of(packed, k)[1], k
    assert lines_of(again, 1)[1] == joined(prefixes[1], None, texts[1])[1]
    job.close()


def test_refusals(strides):
    _, index, plans, _ = strides
    rng = np.random.default_rng(SEED + 30)
    t = hmm.ProbabilityTable(*ARGS)
    batches = [index[c] for _ in range(2) for c in range(NC)]   # 2 x 2 single chains
    job = hmm.Job(batches, t, hmm.make_params(1.26, False, 1e-5))
    prefix = random_prefix(rng, plans[0].n_records)

    def refused(*args, **kw):
        with pytest.raises(hmm.PanGenieError) as e:
            job.line_prefix_strided(*args, **kw)
        assert e.value.code == -1

    refused(0, NC, prefix[0], prefix[1], slot=prefix[2])                 # before a plan
    job.record_plan(0, plans[0])
    refused(0, NC, prefix[0], prefix[1], slot=prefix[2])                 # a member of the stride without a plan
    job.record_plan_strided(0, NC, plans[0])
    job.record_plan_strided(1, NC, plans[1])
    refused(0, 0, prefix[0], prefix[1], slot=prefix[2])                  # pg_job_record_plan_strided's: no contigs,
    refused(NC, NC, prefix[0], prefix[1], slot=prefix[2])                # a contig that is none of them,
    refused(0, 3, prefix[0], prefix[1], slot=prefix[2])                  # 4 index contigs are no multiple of 3
    with pytest.raises(ValueError):                                      # the wrong R, the wrong number of slots
        job.line_prefix_strided(0, NC, *random_prefix(rng, plans[0].n_records + 1)[:2])
    with pytest.raises(ValueError):
        job.line_prefix_strided(0, NC, prefix[0], prefix[1], slot=prefix[2][:-1])
    bad = prefix[0].copy()
    bad[0] = 1
    refused(0, NC, bad, np.concatenate([prefix[1], prefix[1][:1]]), slot=np.zeros(len(prefix[2]), np.uint32))   # offsets that do not start at 0
    for r in (0, len(prefix[2]) // 2, len(prefix[2]) - 1):               # a slot beyond its prefix
        beyond = prefix[2].copy()
        beyond[r] = int(prefix[0][r + 1] - prefix[0][r]) + 1
        refused(0, NC, prefix[0], prefix[1], slot=beyond)
        with pytest.raises(hmm.PanGenieError) as e:
            job.line_prefix(0, prefix[0], prefix[1], slot=beyond)
        assert e.value.code == -1
    # members whose plans differ in their number of records
    fewer = random_plan(np.random.default_rng(SEED + 31), index[0], max_records=1)
    assert fewer.n_records != plans[0].n_records
    job.record_plan(NC, fewer)
    refused(0, NC, prefix[0], prefix[1], slot=prefix[2])
    job.record_plan_strided(0, NC, plans[0])
    # nothing was attached by any of them: every contig is left out of the lines
    job.run()
    job.record_text()
    packed = job.record_lines_packed()
    assert packed[1] == b"" and packed[3].tolist() == [0] * 5
    job.line_prefix_strided(0, NC, prefix[0], prefix[1], slot=prefix[2])
    packed = job.record_lines_packed()
    assert len(lines_of(packed, 0)[1]) > 0 and lines_of(packed, 0)[1] == lines_of(packed, NC)[1] and lines_of(packed, 1)[1] == b""
    job.close()
