"""Shared by the tests of the records of combined groups (tests/test_combined_records_edges_gpu.py,
tests/test_combined_records_gpu.py): the yardstick — per variant the GenotypingResult that tests/combine_util.combined_yardstick
forms over the chains of a group in np.longdouble, normalize() on it, then per record of the plan what
pangenie_amd/genotyping_result.py gives: record_call (fold_onto_record, an empty map as 0/0 with likelihood 1,
get_specific_likelihoods over the defined alleles, likeliest genotype, quality) and the texts of get_all_likelihoods
(tests/record_gl_util.text_of_log) — and the panel of tests/test_combine_gpu.py with a record plan per contig.  Nothing of
pangenie_amd/calls.py or of the kernels forms the expected values."""
import numpy as np

from pangenie_amd.genotyping_result import GenotypingResult, fold_onto_record, record_call
from pangenie_amd.panel import UniqueKmers, flatten, synthetic_panel
from tests.record_calls_util import random_plan
from tests.record_gl_util import texts_of_likelihoods

SUBSETS = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
PLAN_SEED = 20261020


def records_yardstick(plan, want):
    """want: per variant the combined GenotypingResult over allele ids (not normalised).  Answers per record
    (allele_1, allele_2, gq, empty) or None for ./. as tests/record_calls_util.assert_record_calls takes them, and per record
    the texts of its GL values as tests/record_gl_util.assert_record_gl takes them."""
    assert len(want) == plan.n_variants
    calls_want, gl_want = [], []
    for v, combined in enumerate(want):
        res = GenotypingResult()
        res.genotype_to_likelihood = dict(combined.genotype_to_likelihood)
        res.normalize()
        for r in range(int(plan.rec_off[v]), int(plan.rec_off[v + 1])):
            own, vcf = plan.record(r)
            g, gq = record_call(res, own, vcf)
            calls_want.append(None if g is None else (int(g[0]), int(g[1]), int(gq), res.contains_no_likelihoods()))
            f = fold_onto_record(res, own)
            if f.contains_no_likelihoods():
                f.add_to_likelihood(0, 0, 1.0)
            defined = [a for a, x in enumerate(vcf) if int(x) != 0xFFFF]
            gl = f.get_specific_likelihoods(defined) if len(defined) < len(vcf) else f
            gl_want.append(texts_of_likelihoods(gl.get_all_likelihoods(len(defined))))
    assert len(calls_want) == plan.n_records
    return calls_want, gl_want


def records_of(plan, variants):
    """the records of the given variants"""
    return [r for v in variants for r in range(int(plan.rec_off[v]), int(plan.rec_off[v + 1]))]


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
    """the panel of tests/test_combine_gpu.py: 2 contigs x 300 variants x 12 paths, per contig the three subset batches of 4 paths
    over one list of index objects; `wide`: with objects of 6 .. 12 alleles (a job over those sweeps in chunks)"""
    contigs = []
    for c in range(2):
        full = synthetic_panel(300, 12, 20, seed=9100 + c, multiallelic_frac=0.2, **(dict(wide_frac=0.02, wide_at=(0, 151, 299)) if wide else {}))
        uks = unique_kmers_of(full)
        contigs.append([flatten(uks, s) for s in SUBSETS])
    for sub in contigs:   # one layout per contig, whatever the paths
        for b in sub[1:]:
            assert np.array_equal(b.allele_off, sub[0].allele_off) and np.array_equal(b.allele_id, sub[0].allele_id) and b.n_paths == 4
    return contigs


def panel_plans(panel, seed=PLAN_SEED):
    """a random record plan per contig: up to 3 records a bubble, a tenth of the non-reference record alleles undefined"""
    rng = np.random.default_rng(seed)
    return [random_plan(rng, sub[0], max_records=3, undefined=0.1) for sub in panel]


def plan_coverage(panel, plans):
    """(records, records of multi-record bubbles, records with an undefined allele, records of bubbles with more than 5 alleles)"""
    n = multi = undef = wide = 0
    for sub, plan in zip(panel, plans):
        A = np.diff(sub[0].allele_off.astype(np.int64))
        per = np.diff(plan.rec_off.astype(np.int64))
        n += plan.n_records
        multi += int(per[per > 1].sum())
        wide += int(per[A > 5].sum())
        undef += sum(1 for r in range(plan.n_records) if (plan.record(r)[1] == 0xFFFF).any())
    return n, multi, undef, wide


def one_entry_short(plan, batch):
    """a copy of `plan` whose map of ONE record lacks the entry of its bubble's highest allele id; answers (plan, variant)"""
    from pangenie_amd.calls import RecordPlan
    A = np.diff(batch.allele_off.astype(np.int64))
    v = int(np.flatnonzero(A >= 3)[2])
    r = int(plan.rec_off[v + 1]) - 1
    n_ids = int(batch.allele_id[int(batch.allele_off[v]):int(batch.allele_off[v + 1])].max()) + 1
    assert int(plan.map_off[r + 1] - plan.map_off[r]) == n_ids
    mp = np.delete(plan.map[:int(plan.map_off[-1])], int(plan.map_off[r + 1]) - 1)
    map_off = plan.map_off.copy()
    map_off[r + 1:] -= 1
    return RecordPlan(plan.rec_off, map_off, mp, plan.n_alleles[:plan.n_records], plan.vcf_off, plan.vcf_index[:int(plan.vcf_off[-1])]), v
