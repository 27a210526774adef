"""Sampled cohorts (include/pangenie_sampler.h: pg_sampler_cohort_new): haplotype sampling, panel reduction and the
genotyping job for many samples over ONE index.  Every chain must be, bit for bit, what pg_sampler_then_job gives for that
sample alone; the sampled paths what the oracle's sampler gives; the reduced panel what the host's update_paths gives."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from oracle import pyoracle as orc  # checker only
from pangenie_amd import hmm
from pangenie_amd import panel as pn
from pangenie_amd import sampler as smp
from pangenie_amd._lib import PgContigBatch, PgSampleCounts, u16p

pytestmark = pytest.mark.gpu

PANEL_FIELDS = ("kmer_off", "kmer_count", "allele_off", "allele_id", "allele_flags", "allele_kmer_off", "allele_kmer_mask", "path_allele")
TABLE, PARAMS = (18 // 4, 18 * 4, 2 * 18, 0.01), (1.26, False, 1e-5)


def panel(n_variants, n_paths, seed, a_lo=2, a_hi=4, undefined=0.02):
    """Seeded multiallelic panel shaped like the sampler's input: a mosaic of 8 founders, a few private alleles, every
    object with a_lo..a_hi alleles (some of them on no path), up to 14 k-mers per object."""
    rng = np.random.default_rng(seed)
    uks, pos = [], 1000
    mosaic = rng.integers(0, 8, n_paths)
    for v in range(n_variants):
        pos += int(rng.integers(1, 3000))
        A = int(rng.integers(a_lo, a_hi + 1))
        if v and rng.random() < 0.3:
            idx = rng.integers(0, n_paths, max(1, n_paths // 16))
            mosaic[idx] = rng.integers(0, 8, idx.size)
        p2a = rng.integers(0, A, 8)[mosaic]
        noise = rng.random(n_paths) < 0.05
        p2a = np.where(noise, rng.integers(0, A, n_paths), p2a)
        uk = pn.MultiallelicUniqueKmers(pos, p2a.tolist()) if A > 2 or rng.random() < 0.3 else pn.BiallelicUniqueKmers(pos, p2a.tolist())
        for a in sorted(set(p2a.tolist())):
            if rng.random() < undefined:
                uk.set_undefined_allele(a)
        for a in sorted(set(p2a.tolist())):
            for _ in range(int(rng.integers(0, 4))):
                if uk.size() < 14:
                    uk.insert_kmer(int(rng.choice([0, 3, 9])), [a] if rng.random() < 0.7 else [a, int(rng.integers(0, A))])
        uk.set_coverage(int(rng.integers(5, 40)))
        uks.append(uk)
    return pn.flatten(uks)


def fixture_panel():
    from pangenie_amd import cereal_io
    uks = cereal_io.load(Path(__file__).parent / "golden" / "region_UniqueKmersList.cereal").unique_kmers["chr1"]
    return pn.flatten(uks)


def draw_samples(index, n, seed):
    """n samples of read counts around the 'present' threshold of 3 (each sample its own mix) and local coverages."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n):
        p = rng.dirichlet(np.ones(6))
        kcs = [rng.choice(np.array([0, 1, 2, 3, 4, 11], np.uint16), int(b.kmer_off[-1]), p=p).astype(np.uint16) for b in index]
        covs = [rng.integers(5, 40, b.n_variants).astype(np.uint16) for b in index]
        out.append((kcs, covs))
    return out


@pytest.fixture(scope="module")
def cohort_index():
    wide = panel(60, 40, 13, a_lo=6, a_hi=12)
    assert (np.diff(wide.allele_off) >= 6).mean() > 0.9       # objects of 6-12 alleles: wide columns in the reduced panels
    return [fixture_panel(), panel(150, 64, 11, 2, 4), panel(120, 215, 12, 2, 3), wide, panel(10, 30, 14).slice(0, 0)]


def check_cohort(index, samples, size, add_reference, params, oracle=True, parity_chains=()):
    t = hmm.ProbabilityTable(*TABLE)
    job, sampled, best = smp.sample_cohort(index, samples, size, t, params, add_reference=add_reference)
    nc = len(index)
    assert job.n_chains == len(samples) * nc
    job.run()
    got = job.fetch_all()
    picks = []
    for s, (kcs, covs) in enumerate(samples):
        own = [b.with_counts(kc, cv) for b, kc, cv in zip(index, kcs, covs)]
        alone, a_sampled, a_best = smp.sample_then_job(own, size, t, params, add_reference=add_reference)
        alone.run()
        want = alone.fetch_all()
        for c, b in enumerate(own):
            g = s * nc + c
            assert np.array_equal(sampled[s][c], a_sampled[c]), (s, c)
            assert best[s][c].tolist() == a_best[c].tolist(), (s, c)
            dev, ref_panel = job.batches[g], alone.batches[c]
            assert dev.n_paths == ref_panel.n_paths
            for f in PANEL_FIELDS:
                assert np.array_equal(getattr(dev, f), getattr(ref_panel, f)), (s, c, f)
            r, w = got[g], want[c]
            assert r.n_columns == w.n_columns, (s, c)
            for f in ("lik", "lik_exp", "kept", "n_kmers", "coverage"):
                assert np.array_equal(getattr(r, f), getattr(w, f)), (s, c, f)
            if params.run_phasing:
                assert np.array_equal(r.haplotype_1, w.haplotype_1) and np.array_equal(r.haplotype_2, w.haplotype_2), (s, c)
            if b.n_variants == 0:
                continue
            if oracle:
                o_paths, o_best = orc.sampler_run(b, size)
                assert np.array_equal(sampled[s][c], o_paths) and best[s][c].tolist() == o_best.tolist(), (s, c)
                rows = np.vstack([o_paths, np.zeros((1, b.n_variants), np.uint32)]) if add_reference else o_paths
                host = b.update_paths(rows)
                for f in PANEL_FIELDS:
                    assert np.array_equal(getattr(dev, f), getattr(host, f)), (s, c, f)
                if g in parity_chains:
                    from tests.parity_util import assert_parity
                    ref = orc.genotype_contig(host, orc.OracleTable(*TABLE), orc.make_params(*PARAMS))
                    assert_parity(host, r, ref)
        alone.close()
        picks.append(np.concatenate([sampled[s][c].ravel() for c in range(nc)]))
    # samples sharing one index picked different paths: nothing of one sample's passes leaks into another's
    assert len({p.tobytes() for p in picks}) >= 2
    job.close()
    return job


@pytest.mark.parametrize("size,add_reference", [(15, True), (15, False), (3, True), (3, False)])
def test_cohort_equals_one_sample_at_a_time(cohort_index, size, add_reference):
    samples = draw_samples(cohort_index, 5, 100 + size + int(add_reference))
    p = hmm.make_params(*PARAMS)
    oracle = size == 15
    check_cohort(cohort_index, samples, size, add_reference, p, oracle=oracle, parity_chains=(1, 6, 8) if oracle else ())


def test_cohort_general_kernel(cohort_index, monkeypatch):
    """PG_SAMPLER_KERNEL=general: the saturating kernel (masks from the chain's own picks in LDS) over the shared index."""
    monkeypatch.setenv("PG_SAMPLER_KERNEL", "general")
    samples = draw_samples(cohort_index, 4, 7)
    check_cohort(cohort_index, samples, 15, True, hmm.make_params(*PARAMS), oracle=True)
    assert smp.last_ms()[1] == 0


def test_cohort_run_phasing(cohort_index):
    samples = draw_samples(cohort_index, 3, 21)
    p = hmm.make_params(*PARAMS, run_phasing=True)
    check_cohort(cohort_index, samples, 15, True, p, oracle=False)


def one_variant_contig(total, undefined=False):
    """One variant, two paths, both carrying allele 0, whose k-mers are the variant's first `total` ones."""
    mask = (1 << total) - 1 if total < 32 else 0xFFFFFFFF
    return pn.ContigBatch(2, np.array([1000], np.uint64), np.array([20], np.uint16), np.array([0, total], np.uint32),
                          np.zeros(total, np.uint16), np.array([0, 1], np.uint32), np.array([0], np.uint16),
                          np.array([1 if undefined else 0], np.uint8), np.array([0], np.uint16), np.array([mask], np.uint32),
                          np.array([0, 0], np.uint16))


def test_emission_costs_every_case_exactly():
    """present = 0..32 (one sample each) against total = 1..32 (one contig each), an allele without k-mers and an undefined
    allele: with size = 1 the best score of a one-variant contig is that allele's cost, formed on the device from the
    33 x 33 table; it equals pg_sampler_emission_costs (host) and the oracle wherever present <= total."""
    index = [one_variant_contig(total) for total in range(1, 33)] + [one_variant_contig(0), one_variant_contig(5, undefined=True)]
    rng = np.random.default_rng(3)
    samples = []
    for present in range(33):
        kcs = []
        for b in index:
            K = int(b.kmer_off[-1])
            kc = rng.integers(0, 3, K).astype(np.uint16)                  # 0..2: absent
            kc[:min(present, K)] = rng.integers(3, 60, min(present, K))   # >= 3: present
            kcs.append(kc)
        samples.append((kcs, [np.array([20], np.uint16) for _ in index]))
    t = hmm.ProbabilityTable(*TABLE)
    job, sampled, best = smp.sample_cohort(index, samples, 1, t)
    job.close()
    seen = set()
    for present, (kcs, covs) in enumerate(samples):
        for c, b in enumerate(index):
            own = b.with_counts(kcs[c], covs[c])
            want = int(smp.emission_costs(own)[0])
            assert want == int(orc.sampler_emission_costs(own)[0])
            assert int(best[present][c][0]) == want, (present, c)
            if c < 32 and present == 0:
                assert want == 25
            seen.add(want)
    assert seen == set(range(16)) | {25, 50}                       # 1/32 present: 15


def test_upload_counts_per_sample_only(cohort_index):
    t = hmm.ProbabilityTable(*TABLE)
    samples = draw_samples(cohort_index, 2, 5)
    job, _, _ = smp.sample_cohort(cohort_index, samples, 4, t, want_paths=False)
    job.close()
    ix2, ps2 = smp.last_h2d_bytes()
    per_sample = sum(2 * int(b.kmer_off[-1]) for b in cohort_index)
    assert ps2 == 2 * per_sample
    job, _, _ = smp.sample_cohort(cohort_index, samples + draw_samples(cohort_index, 2, 6), 4, t, want_paths=False)
    job.close()
    ix4, ps4 = smp.last_h2d_bytes()
    assert ps4 == 4 * per_sample and ix4 == ix2 > 0
    ms = smp.last_phase_ms()
    assert ms["total"] > 0 and ms["passes"] > 0


def test_errors(cohort_index):
    t = hmm.ProbabilityTable(*TABLE)
    p = hmm.make_params(*PARAMS)
    samples = draw_samples(cohort_index, 2, 9)
    small = [cohort_index[3]]                                    # 40 paths
    small_samples = [([kc[3]], [cv[3]]) for kc, cv in samples]

    def code(fn):
        with pytest.raises(hmm.PanGenieError) as e:
            fn()
        return e.value.code

    assert code(lambda: smp.sample_cohort(cohort_index, [], 3, t)) == -1                  # no samples
    assert code(lambda: smp.sample_cohort(cohort_index, samples, 0, t)) == -1             # no pass
    assert code(lambda: smp.sample_cohort(small, small_samples, 40, t)) == -1             # as many passes as paths
    assert code(lambda: smp.sample_cohort(small, small_samples, 41, t)) == -1
    huge = pn.ContigBatch(65535, np.array([10], np.uint64), np.array([5], np.uint16), np.array([0, 0], np.uint32), np.zeros(0, np.uint16),
                          np.array([0, 1], np.uint32), np.array([0], np.uint16), np.array([0], np.uint8), np.array([0], np.uint16),
                          np.array([0], np.uint32), np.zeros(65535, np.uint16))
    assert code(lambda: smp.sample_cohort([huge], [([np.zeros(0, np.uint16)], [np.array([5], np.uint16)])], 1, t)) == -3
    with pytest.raises(ValueError):                                                         # lengths checked on the host
        smp.sample_cohort(small, [([small_samples[0][0][0][:-1]], small_samples[0][1])], 3, t)
    # the C ABI itself: null arguments, a sample without counts for a contig that has k-mers
    lib = smp._hip()
    arr = (PgContigBatch * 1)(small[0].as_c())
    cs, keep = smp.marshal_samples(small, small_samples)
    err = C.create_string_buffer(512)
    h = C.c_void_p()
    ld = C.c_longdouble(25000.0)
    call = lambda idx, n_s, smpl, table, out: lib.pg_sampler_cohort_new(0, 1, idx, n_s, smpl, 3, 0, 1.26, ld, 10, table, C.byref(p),
                                                                         None, None, out, err, 512)
    assert call(None, 2, cs, t.h, C.byref(h)) == -1
    assert call(arr, 2, None, t.h, C.byref(h)) == -1
    assert call(arr, 2, cs, None, C.byref(h)) == -1
    assert call(arr, 2, cs, t.h, None) == -1
    no_counts = (u16p * 1)()                                     # NULL entry
    bad = (PgSampleCounts * 1)()
    bad[0].kmer_count = no_counts
    bad[0].coverage = cs[0].coverage
    assert call(arr, 1, bad, t.h, C.byref(h)) == -1 and b"k-mer counts" in err.value
    assert h.value is None
    # and after all of that a valid call still works
    assert call(arr, 2, cs, t.h, C.byref(h)) == 0
    hmm.Job.from_handle(h.value, t, p).close()
    del keep
