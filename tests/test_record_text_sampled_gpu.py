"""The record text of a sampled cohort: 4 samples x 2 contigs x 300 bubbles, 40 panel paths sampled to
15 + 1 (a third of the bubbles multiallelic with up to 12 alleles, so the reduced panels keep bubbles of more than five), one
strided record plan per contig.  Every chain is its own index contig there, and the text is one packed buffer: the packed text
and its offsets equal the per-chain fetches laid end to end, text_first agrees with the lengths, and every chain's bytes are
the text put together in Python from that chain's own record calls, record GLs, coverage and k-mer counts
(tests/record_text_util.py), with ignore_imputed off and on."""
import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd import sampler as smp
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.record_calls_util import random_plan
from tests.record_gl_util import is_deferred
from tests.record_text_util import DEFERRED, assert_text, expected_text

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
SEED, NS, NC = 9400, 4, 2


@pytest.fixture(scope="module")
def world():
    index = [synthetic_panel(300, 40, 20, seed=SEED + c, multiallelic_frac=0.3, max_alleles=12, undefined_frac=0.05, local_alts=11, zero_kmer_frac=0.05)
             for c in range(NC)]
    samples = []
    for s in range(NS):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=SEED + 10 + NC * s + c) for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    job, _, _ = smp.sample_cohort(index, samples, 15, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5), add_reference=True, want_paths=False)
    assert job.n_chains == NS * NC and all(b.n_paths == 16 for b in job.batches)
    job.run()
    rng = np.random.default_rng(SEED + 1)
    plans = [random_plan(rng, ix) for ix in index]
    for c, p in enumerate(plans):
        job.record_plan_strided(c, NC, p)
    yield job, plans
    job.close()


@pytest.mark.parametrize("ignore_imputed", [False, True])
def test_packed_text_is_the_chains_texts_end_to_end_and_the_fields_text(world, ignore_imputed):
    job, plans = world
    off, text, first = job.record_text_packed(ignore_imputed)
    chains = [calls.fetch_record_text(job, g) for g in range(NS * NC)]
    assert text == b"".join(t for _, t in chains)
    lengths = [len(t) for _, t in chains]
    assert first.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist() and min(lengths) > 0
    assert off.tolist() == np.concatenate([o[:-1].astype(np.int64) + int(first[g]) for g, (o, _) in enumerate(chains)] + [[len(text)]]).tolist()
    calls_first, gl_first = job.record_first()
    assert len(off) == int(calls_first[-1]) + 1 and len(text) <= calls.record_text_bound(int(calls_first[-1]), int(gl_first[-1]))
    rec_all, gl_all = job.record_calls_packed()[0], job.record_gl_packed()[0]
    assert not is_deferred(gl_all).any() and not ((rec_all["flags"] & 0xFF) == DEFERRED).any()
    dots = 0
    for g in range(NS * NC):
        plan = plans[g % NC]
        rec, gl = rec_all[int(calls_first[g]):int(calls_first[g + 1])], gl_all[int(gl_first[g]):int(gl_first[g + 1])]
        res = job.fetch(g)
        rec_var = np.repeat(np.arange(plan.n_variants), np.diff(plan.rec_off.astype(np.int64)))
        no_call = (res.n_kmers[rec_var] == 0).astype(np.uint8) if ignore_imputed else None
        gl_off = calls.record_gl_offsets(plan)
        want_off, want_text, hosts = expected_text(rec, gl_off, gl, res.coverage[rec_var], no_call)
        assert np.array_equal(hosts, np.diff(gl_off.astype(np.int64)) < 3)
        assert_text(chains[g][0], chains[g][1], want_off, want_text, ("chain", g, ignore_imputed))
        dots += want_text.count(b".:.:")
    assert chains[0][1] != chains[NC][1]   # one plan, two samples, two texts
    assert dots > 0 or not ignore_imputed   # bubbles without k-mers: .:.: when imputed calls are ignored
