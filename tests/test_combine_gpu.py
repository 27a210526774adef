"""Path subsets combined on the device through a job (pg_job_combine_plan / pg_job_combine / pg_job_combined_calls,
pangenie_amd/csrc/pg_combine.hip): two contigs of 300 variants over 12 paths, each genotyped over three subsets of 4 paths
(panel.flatten(..., only_paths)) as ONE job of six chains in two groups.  The combined bins of every group against
GenotypingResult.combine over the same job's fetched bins in the order of the group, bit for bit; the calls against normalize ->
get_likeliest_genotype -> get_genotype_quality on that; every combined likelihood against the CPU oracle's per-subset results
combined the same way (1e-6 relative, the project's parity bound).  Reversed groups, a cohort, the refusals; the other sweep mode
(fused) once, on the same panel without its objects of 6 .. 12 alleles, which a fused job does not take."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import calls, hmm
from pangenie_amd.panel import UniqueKmers, flatten, synthetic_panel, synthetic_sample_counts
from tests.calls_util import assert_calls
from tests.combine_util import LD, assert_bins, calls_yardstick, combined_yardstick

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
SUBSETS = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]


def unique_kmers_of(batch):
    """the UniqueKmers objects a synthetic contig stands for (every k-mer on the alleles whose window holds it)"""
    V, H = batch.n_variants, batch.n_paths
    pa = batch.path_allele.reshape(V, H)
    out = []
    for v in range(V):
        a0, a1 = int(batch.allele_off[v]), int(batch.allele_off[v + 1])
        k0, k1 = int(batch.kmer_off[v]), int(batch.kmer_off[v + 1])
        uk = UniqueKmers(int(batch.variant_pos[v]), pa[v], a1 - a0 == 2)
        uk.set_coverage(int(batch.coverage[v]))
        for k in range(k1 - k0):
            on = [int(batch.allele_id[s]) for s in range(a0, a1)
                  if 0 <= k - int(batch.allele_kmer_off[s]) < 32 and (int(batch.allele_kmer_mask[s]) >> (k - int(batch.allele_kmer_off[s]))) & 1]
            uk.insert_kmer(int(batch.kmer_count[k0 + k]), on)
        for s in range(a0, a1):
            if batch.allele_flags[s] & 1 and int(batch.allele_id[s]) in uk.alleles:
                uk.set_undefined_allele(int(batch.allele_id[s]))
        out.append(uk)
    return out


def make_panel(wide):
    """per contig the three subset batches over one list of index objects"""
    contigs = []
    for c in range(2):
        full = synthetic_panel(300, 12, 20, seed=9100 + c, multiallelic_frac=0.2, **(dict(wide_frac=0.02, wide_at=(0, 151, 299)) if wide else {}))
        uks = unique_kmers_of(full)
        contigs.append([flatten(uks, s) for s in SUBSETS])
    A = np.concatenate([np.diff(sub[0].allele_off.astype(np.int64)) for sub in contigs])
    assert ((A >= 3) & (A <= 5)).sum() > 0.12 * len(A) and A.max() <= 12 and (6 <= (A > 5).sum() if wide else A.max() <= 5)
    for sub in contigs:   # one layout per contig, whatever the paths
        for b in sub[1:]:
            assert np.array_equal(b.allele_off, sub[0].allele_off) and np.array_equal(b.allele_id, sub[0].allele_id) and b.n_paths == 4
    return contigs


@pytest.fixture(scope="module")
def panel():
    return make_panel(True)


@pytest.fixture(scope="module")
def narrow_panel():
    """the same without the objects of 6 .. 12 alleles: a job over those always sweeps in chunks (their columns' posteriors are k_post's)"""
    return make_panel(False)


def carried(batch):
    """[sumA] allele slot on a selected path; [V] some selected path carries a defined non-reference allele (a column)"""
    V, H = batch.n_variants, batch.n_paths
    pa = batch.path_allele.reshape(V, H)
    slot_v = np.repeat(np.arange(V), np.diff(batch.allele_off.astype(np.int64)))
    on = (pa[slot_v] == batch.allele_id[:, None]).any(axis=1)
    col = np.zeros(V, bool)
    np.logical_or.at(col, slot_v, on & (batch.allele_id != 0) & ((batch.allele_flags & 1) == 0))
    return on, col


def test_the_panel_has_what_the_union_of_key_sets_is_about(panel):
    """on the CPU: some object has an allele that one subset alone carries, some variant is a column in one subset and not in another"""
    for sub in panel:
        on, col = zip(*[carried(b) for b in sub])
        assert (np.sum(on, axis=0) == 1).any()
        assert (np.any(col, axis=0) & ~np.all(col, axis=0)).any()


def job_yardstick(job, results, groups):
    out = []
    for g in groups:
        b = job.batches[g[0]]
        want, deferred = combined_yardstick(b.allele_off, b.allele_id, [results[c].kept for c in g], [results[c].allele_present for c in g],
                                            [results[c].lik for c in g], [results[c].lik_exp for c in g])
        out.append((b, want, deferred))
    return out


def check_groups(job, groups, what):
    """combined bins == the yardstick over the job's own fetched bins, calls == the yardstick's; pg_job_calls and pg_job_fetch untouched"""
    before = job.fetch_all()
    calls_before = job.calls()
    job.combine()
    bins = job.combined()
    recs = job.combined_calls()
    after = job.fetch_all()
    for r0, r1 in zip(before, after):
        assert np.array_equal(r0.lik, r1.lik) and np.array_equal(r0.lik_exp, r1.lik_exp) and np.array_equal(r0.kept, r1.kept)
        assert np.array_equal(r0.allele_present, r1.allele_present)
    for c0, c1 in zip(calls_before, job.calls()):
        assert np.array_equal(c0, c1)
    n_keys = n_ok = 0
    yard = job_yardstick(job, before, groups)
    for g, (b, want, deferred) in enumerate(yard):
        assert bins[g].dtype == calls.COMBINED_DTYPE and len(bins[g]) == int(b.geno_off[-1]) and len(recs[g]) == b.n_variants
        assert np.array_equal(bins[g], job.combined(g)) and np.array_equal(recs[g], job.combined_calls(g))
        k, d = assert_bins(b.allele_off, b.allele_id, bins[g], want, deferred, (what, g))
        assert d == 0   # (the panels' likelihoods are nowhere near 2^-16300)
        n_keys += k
        assert assert_calls(recs[g], calls_yardstick(want), (what, g)) == []
        n_ok += int((recs[g]["flags"] == calls.PG_CALL_OK).sum())
    assert job.combine_ms() > 0.0 and job.combined_calls_ms() > 0.0
    return bins, recs, yard, n_keys, n_ok


@pytest.mark.parametrize("mode", ["fused", "chunked"])
def test_six_chains_in_two_groups_against_the_host_route_and_the_oracle(panel, narrow_panel, mode, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", mode)
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    batches = [b for sub in (panel if mode == "chunked" else narrow_panel) for b in sub]
    groups = [[0, 1, 2], [3, 4, 5]]
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.sweep_mode()[0] == mode, job.plan()
    job.run()
    job.combine_plan(groups)
    assert job._lib.pg_job_n_groups(job.h) == 2
    bins, recs, yard, n_keys, n_ok = check_groups(job, groups, mode)
    assert n_keys > 1500 and n_ok > 300
    # keys that one chain alone would not have, variants that one chain alone would not call
    single = job.fetch_all()
    for g, grp in enumerate(groups):
        b = batches[grp[0]]
        present = bins[g]["flags"] != 0
        own = [np.repeat(r.kept.astype(bool), np.diff(b.geno_off.astype(np.int64))) for r in (single[c] for c in grp)]
        assert all((present & ~o).any() for o in own)
    if mode == "fused":   # (the other sweep mode, once: the rest hangs on the bins alone)
        job.close()
        return
    # the same groups in reversed order give the reversed yardstick (and it is another one)
    rev = [g[::-1] for g in groups]
    job.combine_plan(rev)
    bins_r, recs_r, yard_r, _, _ = check_groups(job, rev, "reversed")
    assert any(((x["m"] != y["m"]) | (x["e"] != y["e"])).any() for x, y in zip(bins, bins_r))
    assert all(np.array_equal(x["flags"], y["flags"]) for x, y in zip(bins, bins_r))
    # the oracle's per-subset results combined the same way: 1e-6 relative on every combined likelihood, the same GT wherever
    # the oracle's own best two values differ by more than 1e-9
    from oracle import pyoracle as orc
    job.combine_plan(groups)
    job.combine()
    bins, recs = job.combined(), job.combined_calls()
    worst = 0.0
    n_gt = 0
    for g, grp in enumerate(groups):
        b = batches[grp[0]]
        refs = [orc.genotype_contig(batches[c], orc.OracleTable(*ARGS), orc.make_params(1.26, False, 1e-5)) for c in grp]
        goff = b.geno_off.astype(np.int64)
        total = np.zeros(int(goff[-1]), LD)
        held = np.zeros(int(goff[-1]), bool)
        slot_v = np.repeat(np.arange(b.n_variants), np.diff(b.allele_off.astype(np.int64)))
        for r in refs:   # GenotypingResult::combine over the chains that hold the key, in the order of the group
            h = np.zeros(int(goff[-1]), bool)
            for v in range(b.n_variants):
                if not r.kept[v]:
                    continue
                p = r.allele_present[int(b.allele_off[v]):int(b.allele_off[v + 1])].astype(bool)
                h[goff[v]:goff[v + 1]] = (p[:, None] & p[None, :])[np.triu_indices(len(p))]
            total = np.where(h, total + r.lik, total)
            held |= h
        assert np.array_equal(held, bins[g]["flags"] != 0)
        got = calls.combined_to_longdouble(bins[g])
        nz = held & (total > 0)
        rel = np.abs((got[nz] - total[nz]) / total[nz]).astype(np.float64)
        worst = max(worst, float(rel.max()))
        assert (got[held & (total == 0)] == 0).all()
        for v in range(b.n_variants):
            t = total[goff[v]:goff[v + 1]][held[goff[v]:goff[v + 1]]]
            if len(t) == 0 or t.sum() <= 0:
                continue
            q = np.sort(t / t.sum())
            if len(q) > 1 and q[-1] - q[-2] <= 1e-9:
                continue
            k = int(np.flatnonzero(held[goff[v]:goff[v + 1]])[int(np.argmax(t))])
            A = int(b.allele_off[v + 1] - b.allele_off[v])
            sa, sb = [(x, y) for x in range(A) for y in range(x, A)][k]
            ids = b.allele_id[int(b.allele_off[v]):int(b.allele_off[v + 1])]
            assert int(recs[g][v]["flags"]) == calls.PG_CALL_OK and (int(recs[g][v]["allele_1"]), int(recs[g][v]["allele_2"])) == (int(ids[sa]), int(ids[sb])), (g, v)
            n_gt += 1
    print("combined likelihoods against the oracle: worst relative error", worst, "genotypes compared", n_gt)
    assert worst <= 1e-6 and n_gt > 300
    job.close()


def test_a_cohort_has_groups_per_sample(panel):
    """pg_cohort_new over the six subset batches as index contigs, two samples: twelve chains, four groups"""
    index = [b for sub in panel for b in sub]
    samples = []
    for s in range(2):
        kcs, covs = [], []
        for c, sub in enumerate(panel):
            kc, cov = synthetic_sample_counts(sub[0], seed=9200 + 10 * s + c)   # one sample, one set of counts per contig
            kcs += [kc] * 3
            covs += [cov] * 3
        samples.append((kcs, covs))
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    assert job.n_chains == 12
    groups = [[6 * s + 3 * c + k for k in range(3)] for s in range(2) for c in range(2)]
    job.run()
    job.combine_plan(groups)
    bins, recs, yard, n_keys, n_ok = check_groups(job, groups, "cohort")
    assert n_keys > 3000 and n_ok > 600
    assert not np.array_equal(recs[0], recs[2])   # two samples, two sets of calls
    # a new batch of samples invalidates the run: combine, the calls and the fetches are refused until the next one
    job.upload_begin(samples[::-1])
    job.upload_end()
    for refused in (job.combine, job.combined_calls, lambda: job.combined(0)):
        with pytest.raises(hmm.PanGenieError) as e:
            refused()
        assert e.value.code == -1
    job.run()
    with pytest.raises(hmm.PanGenieError) as e:   # the calls want the combine of THIS run
        job.combined_calls()
    assert e.value.code == -1
    job.combine()
    swapped = job.combined_calls()
    assert np.array_equal(swapped[0], recs[2]) and np.array_equal(swapped[3], recs[1])
    job.close()


def test_plan_refusals_and_a_second_plan(panel):
    batches = [b for sub in panel for b in sub]
    other = synthetic_panel(300, 4, 20, seed=9300, multiallelic_frac=0.2)     # 300 variants of another layout
    short = batches[0].slice(0, 200)
    b1 = batches[1]
    ids = type(b1)(b1.n_paths, b1.variant_pos, b1.coverage, b1.kmer_off, b1.kmer_count, b1.allele_off, b1.allele_id.copy(), b1.allele_flags,
                   b1.allele_kmer_off, b1.allele_kmer_mask, b1.path_allele.copy())
    multi = int(np.flatnonzero(np.diff(ids.allele_off.astype(np.int64)) > 2)[0])
    a0 = int(ids.allele_off[multi])
    ids.allele_id[a0 + 1:int(ids.allele_off[multi + 1])] += 1                 # the same alleles per variant, other ids
    ids.path_allele.reshape(300, 4)[multi][ids.path_allele.reshape(300, 4)[multi] > 0] += 1
    job = hmm.Job(batches + [other, short, ids], hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    lib, err = job._lib, C.create_string_buffer(512)

    def refused(groups, code=-1):
        with pytest.raises(hmm.PanGenieError) as e:
            job.combine_plan(groups)
        assert e.value.code == code, (groups, e.value)
        assert lib.pg_job_n_groups(job.h) == n_before
    n_before = 0
    with pytest.raises(hmm.PanGenieError) as e:   # combine before any plan: refused (and before the run)
        job.combine()
    assert e.value.code == -1
    refused([])                      # no group
    refused([[0, 1], []])            # an empty group
    refused([[0, 1, 9]])             # a chain the job does not have
    refused([[0, 1, 1]])             # a chain twice in one group
    refused([[0, 1], [2, 1]])        # ... in two
    refused([[0, 7]])                # another number of variants
    refused([[0, 6]])                # other alleles per variant
    refused([[1, 8]])                # other allele ids
    refused([[3, 4], [1, 8]])        # ... in the second group: nothing is attached
    assert lib.pg_job_combine_plan(job.h, 1, None, None, err, 512) == -1
    job.combine_plan([[0, 1, 2]])    # a plan may come before the run
    n_before = 1
    with pytest.raises(hmm.PanGenieError) as e:   # combine before the run
        job.combine()
    assert e.value.code == -1
    job.run()
    with pytest.raises(hmm.PanGenieError) as e:   # calls before combine
        job.combined_calls()
    assert e.value.code == -1
    with pytest.raises(hmm.PanGenieError) as e:   # fetch before combine
        job.combined(0)
    assert e.value.code == -1
    d, n = C.c_void_p(), C.c_uint64()
    assert lib.pg_job_device_combined(job.h, 0, C.byref(d), C.byref(n)) == -1
    job.combine()
    assert lib.pg_job_device_combined(job.h, 0, C.byref(d), C.byref(n)) == 0 and n.value == int(batches[0].geno_off[-1]) and d.value
    assert lib.pg_job_device_combined_calls(job.h, 0, C.byref(d), C.byref(n)) == -1
    first = job.combined(0)
    refused([[0, 6]])                # a refused plan leaves the one the job has
    assert np.array_equal(job.combined(0), first)
    rec = job.combined_calls(0)
    assert lib.pg_job_device_combined_calls(job.h, 0, C.byref(d), C.byref(n)) == 0 and n.value == 300
    # a second plan replaces the first: other groups, nothing combined yet
    job.combine_plan([[2, 0], [3], [4, 5]])
    assert lib.pg_job_n_groups(job.h) == 3
    with pytest.raises(hmm.PanGenieError) as e:
        job.combined(0)
    assert e.value.code == -1
    job.combine()
    res = job.fetch_all()
    three = job.combined()
    b = batches[3]
    own = np.ldexp(res[3].lik.astype(LD), res[3].lik_exp.astype(np.int64))
    present = three[1]["flags"] != 0
    assert present.any() and (calls.combined_to_longdouble(three[1])[present] == own[present]).all()   # a group of one: the chain's own bins
    assert np.array_equal(job.combined_calls(1), job.calls(3))
    assert len(three[0]) == len(first) and not np.array_equal(three[0], first)
    assert lib.pg_job_fetch_combined(job.h, 3, three[0].ctypes.data, err, 512) == -1   # no such group
    job.close()
    # a job without run_genotyping has no bins to combine
    job = hmm.Job(batches[:3], hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5, run_genotyping=False, run_phasing=True))
    with pytest.raises(hmm.PanGenieError) as e:
        job.combine_plan([[0, 1, 2]])
    assert e.value.code == -1
    job.close()
