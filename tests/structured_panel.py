"""Panels of UniqueKmers objects with the structure the C ABI allows and `pangenie_amd.panel.synthetic_panel` never
builds (include/pangenie_hmm.h; reference src/uniquekmers.hpp, src/kmerpath.cpp): allele ids that are not the slots,
objects without allele 0, k-mers on several alleles and on none, masks with holes, windows that overlap, two-allele
objects of more than 32 k-mers, several undefined alleles in any slot, all paths on one non-reference allele.  A plain
helper module of tests/test_structured_panel_cpu.py and tests/test_structured_objects_gpu.py: the generator, a census of
what a panel holds, and the reference's emission loop restated in numpy long double.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from pangenie_amd.panel import PEAK, ContigBatch

LD = np.longdouble
K_SET = (0, 1, 2, 5, 16, 17, 20, 31, 32, 33, 40, 63, 64, 65, 100, 129)
K_SMALL = tuple(k for k in K_SET if k <= 32)
K_LARGE = tuple(k for k in K_SET if k > 32)
OUTLIER_COUNTS = (300, 2000, 60000)
OUTLIER_P = (0.4, 0.4, 0.2)   # (the oracle's Poisson term is a loop up to the count: the largest is the rarest)
AMAX = 5   # PG_AMAX: a column with more distinct alleles on its paths is a wide column
TABLE_ARGS = (6, 108, 54)   # cov_min, cov_max, count_max of the tests' ProbabilityTable: coverages 3 and 400 lie outside
CHAIN_LENGTHS = (330, 1, 2, 3, 97, 64, 65)   # first and last columns, the meeting point, a single column


def _membership(batch: ContigBatch, v: int) -> np.ndarray:
    """bool [A, K]: k-mer k lies on allele slot s <=> bit k - off of its mask, 0 <= k - off < 32 (src/kmerpath.cpp:33-48)."""
    a0, a1 = int(batch.allele_off[v]), int(batch.allele_off[v + 1])
    K = int(batch.kmer_off[v + 1] - batch.kmer_off[v])
    on = np.zeros((a1 - a0, K), bool)
    for s in range(a1 - a0):
        off, mask = int(batch.allele_kmer_off[a0 + s]), int(batch.allele_kmer_mask[a0 + s])
        for bit in range(32):
            if (mask >> bit) & 1 and off + bit < K:
                on[s, off + bit] = True
    return on


def _draw_counts(index: ContigBatch, rng, peak: int):
    """A sample's read counts over `index`: its genotype follows two panel paths; counts are Poisson around 0, peak / 2 and
    peak by the k-mer's copy number; 3 % are far outside (the largest gives every copy number probability 0 without
    regularisation).  Coverage as synthetic_panel's, with a few values outside the table's box."""
    V, H = index.n_variants, index.n_paths
    pa = index.path_allele.reshape(V, H)
    counts = np.zeros(int(index.kmer_off[-1]) if V else 0, np.int64)
    for v in range(V):
        k0, k1 = int(index.kmer_off[v]), int(index.kmer_off[v + 1])
        ids = index.allele_id[index.allele_off[v]:index.allele_off[v + 1]].tolist()
        g = rng.integers(0, H, size=2)
        if k1 == k0:
            continue
        on = _membership(index, v)
        cn = on[ids.index(int(pa[v, g[0]]))].astype(np.int64) + on[ids.index(int(pa[v, g[1]]))]
        c = rng.poisson(np.where(cn == 0, 0.1, cn * (peak / 2.0)))
        far = rng.random(k1 - k0) < 0.03
        c = np.where(far, rng.choice(OUTLIER_COUNTS, size=k1 - k0, p=OUTLIER_P), c)
        counts[k0:k1] = c
    cov = peak - 3 + rng.integers(0, 7, size=V)
    odd = rng.random(V)
    cov = np.where(odd < 0.01, 3, np.where(odd < 0.02, 400, cov))
    return counts.astype(np.uint16), cov.astype(np.uint16)


def structured_panel(V: int, H: int, seed: int, *, biallelic: bool = False, bi_small_share: float = 0.6,
                     wide: bool = True, peak: int = PEAK) -> ContigBatch:
    """Deterministic panel of V objects over H paths.  `bi_small_share`: about that share of the objects has two alleles
    and at most 32 k-mers (what pg_shim.cpp's classify_index_contig keys prep_fast on); biallelic: every object has two
    alleles (bi_small_share = 1: and at most 32 k-mers); wide: a tenth of the objects has 6 .. 12 alleles spread over
    the paths."""
    rng = np.random.Generator(np.random.PCG64(seed))
    V, H = int(V), int(H)
    pos = np.cumsum(50 + rng.integers(0, 1200, size=V, dtype=np.int64)).astype(np.uint64) + 10000
    p2 = 1.0 if biallelic else min(0.85, bi_small_share + 0.15)
    p_small = min(1.0, bi_small_share / p2)
    kmer_off, allele_off = [0], [0]
    aid, afl, akoff, akmask, paths = [], [], [], [], []
    for v in range(V):
        u = rng.random()
        is_wide = False
        if u < p2:
            A = 2
        elif wide and u > 0.9:
            A, is_wide = int(rng.integers(6, 13)), True
        else:
            A = int(rng.integers(3, 6))
        # ---- number of k-mers
        if A == 2:
            small = rng.random() < p_small
            pool = K_SMALL if small else K_LARGE
            w = np.array([0.7 if k == 0 else 1.0 for k in pool])
        else:
            pool = K_SET
            w = np.array([0.7 if k == 0 else 1.0 for k in pool])
        K = int(rng.choice(pool, p=w / w.sum()))
        # ---- allele ids: ascending, distinct, from 0 .. A + 6
        u = rng.random()
        if u < 0.25:
            ids = list(range(A))
        elif u < 0.40:
            ids = sorted(rng.choice(np.arange(1, A + 7), size=A, replace=False).tolist())
        else:
            ids = [0] + sorted(rng.choice(np.arange(1, A + 7), size=A - 1, replace=False).tolist())
        # ---- undefined alleles: up to two, any slot whose id is not 0; they carry no k-mers
        und = [False] * A
        u = rng.random()
        n_und = 2 if u < 0.08 else (1 if u < 0.22 else 0)
        cand = [s for s in range(A) if ids[s] != 0]
        for s in rng.permutation(cand)[:n_und].tolist():
            und[s] = True
        # ---- k-mer membership: a window of up to 32 k-mers per defined allele, filled with density 0.15 / 0.5 / 1
        for s in range(A):
            off, mask = 0, 0
            if K > 0 and not und[s]:
                w0 = int(rng.integers(0, K))
                n = min(K, w0 + 32) - w0
                hit = np.flatnonzero(rng.random(n) < rng.choice((0.15, 0.5, 1.0)))
                if hit.size:   # offset = the first index set (KmerPath's rule)
                    off = w0 + int(hit[0])
                    mask = int(sum(1 << int(h - hit[0]) for h in hit))
            aid.append(ids[s]); afl.append(1 if und[s] else 0); akoff.append(off); akmask.append(mask)
        # ---- paths
        u = rng.random()
        if is_wide:
            slots = rng.integers(0, A, size=H)
        elif u < 0.08:
            slots = np.zeros(H, np.int64)
        elif u < 0.16:
            slots = np.full(H, int(rng.integers(1, A)), np.int64)
        else:
            wgt = rng.random(A) + 0.05
            slots = rng.choice(A, size=H, p=wgt / wgt.sum())
        paths.append(np.asarray(ids, np.int64)[slots])
        kmer_off.append(kmer_off[-1] + K)
        allele_off.append(allele_off[-1] + A)
    index = ContigBatch(H, pos, np.zeros(V, np.uint16), np.array(kmer_off, np.uint32), np.zeros(kmer_off[-1], np.uint16),
                        np.array(allele_off, np.uint32), np.array(aid, np.uint16), np.array(afl, np.uint8),
                        np.array(akoff, np.uint16), np.array(akmask, np.uint32),
                        (np.concatenate(paths) if V else np.zeros(0)).astype(np.uint16))
    counts, cov = _draw_counts(index, rng, peak)
    return index.with_counts(counts, cov)


def structured_counts(index: ContigBatch, seed: int, peak: int = PEAK):
    """(kmer_count u16 [sumK], coverage u16 [V]) of another sample over the same index."""
    return _draw_counts(index, np.random.Generator(np.random.PCG64(seed)), peak)


CENSUS_CLASSES = ("ids_not_slots", "no_id_0", "kmer_on_two_alleles", "kmer_on_no_allele", "mask_with_hole", "two_alleles_K_gt_32",
                  "three_to_five_alleles_K_gt_64", "K_0", "K_32_33_64_65", "two_undefined", "undefined_not_last",
                  "all_paths_one_nonref", "wide_column")
MULTI_CLASSES = ("three_to_five_alleles_K_gt_64",)
WIDE_CLASSES = ("wide_column",)


def census(batch) -> dict:
    """Number of objects of `batch` (a ContigBatch, or a list of them: the sum) in each class of CENSUS_CLASSES."""
    if isinstance(batch, (list, tuple)):
        out = dict.fromkeys(CENSUS_CLASSES, 0)
        for b in batch:
            for k, n in census(b).items():
                out[k] += n
        return out
    out = dict.fromkeys(CENSUS_CLASSES, 0)
    V, H = batch.n_variants, batch.n_paths
    pa = batch.path_allele.reshape(V, H)
    for v in range(V):
        a0, a1 = int(batch.allele_off[v]), int(batch.allele_off[v + 1])
        A, K = a1 - a0, int(batch.kmer_off[v + 1] - batch.kmer_off[v])
        ids = batch.allele_id[a0:a1].tolist()
        und = (batch.allele_flags[a0:a1] & 1).astype(bool)
        on = _membership(batch, v)
        per_kmer = on.sum(axis=0)
        out["ids_not_slots"] += ids != list(range(A))
        out["no_id_0"] += 0 not in ids
        out["kmer_on_two_alleles"] += bool((per_kmer >= 2).any())
        out["kmer_on_no_allele"] += bool((per_kmer == 0).any())
        holes = False
        for m in batch.allele_kmer_mask[a0:a1].tolist():
            holes = holes or (m & (m + 1)) != 0   # not a run of ones from bit 0
        out["mask_with_hole"] += holes
        out["two_alleles_K_gt_32"] += A == 2 and K > 32
        out["three_to_five_alleles_K_gt_64"] += 3 <= A <= 5 and K > 64
        out["K_0"] += K == 0
        out["K_32_33_64_65"] += K in (32, 33, 64, 65)
        out["two_undefined"] += int(und.sum()) >= 2
        out["undefined_not_last"] += bool(und[:-1].any())
        on_paths = set(pa[v].tolist())
        out["all_paths_one_nonref"] += len(on_paths) == 1 and 0 not in on_paths
        out["wide_column"] += len(on_paths) > AMAX
    return {k: int(n) for k, n in out.items()}


def n_bi_small(batch: ContigBatch) -> int:
    """objects with two alleles and at most 32 k-mers: what classify_index_contig counts as n_bi"""
    A = np.diff(batch.allele_off.astype(np.int64))
    K = np.diff(batch.kmer_off.astype(np.int64))
    return int(((A == 2) & (K <= 32)).sum())


def emission_restatement(batch: ContigBatch, table, v: int):
    """EmissionProbabilityComputer of object v (reference src/emissionprobabilitycomputer.cpp:9-53) over all allele slots
    in numpy long double: ([A, A] products, all_zeros).  `table`: anything with get(coverage, count) -> three long
    doubles, the probabilities of copy numbers 0, 1, 2."""
    a0, a1 = int(batch.allele_off[v]), int(batch.allele_off[v + 1])
    A = a1 - a0
    k0, k1 = int(batch.kmer_off[v]), int(batch.kmer_off[v + 1])
    und = (batch.allele_flags[a0:a1] & 1).astype(bool)
    on = _membership(batch, v).astype(np.int64)
    cov = int(batch.coverage[v])
    both = und[:, None] & und[None, :]
    one = (und[:, None] | und[None, :]) & ~both
    result = np.ones((A, A), LD)
    third, half = LD(1) / LD(3), LD("0.5")
    for k in range(k1 - k0):
        p = np.asarray(table.get(cov, int(batch.kmer_count[k0 + k])), LD)
        c = on[:, None, k] + on[None, :, k]
        known = p[c]
        two = half * (p[np.minimum(c, 1)] + p[np.minimum(c, 1) + 1])   # (the reference asserts c < 2 where it is used)
        three = third * (p[0] + p[1] + p[2])
        result = result * np.where(both, three, np.where(one, two, known))
    return result, not bool((result > 0).any())


# ---------------------------------------------------------------------------------------------
#  the panels of tests/test_structured_objects_gpu.py, by name (tests/test_structured_panel_cpu.py checks the census of each)
# ---------------------------------------------------------------------------------------------
def _spec(H, seed, lengths=CHAIN_LENGTHS, **kw):
    return (int(H), int(seed), tuple(lengths), tuple(sorted(kw.items())))


GPU_PANELS = {}
for _H in (13, 16, 27, 32, 41, 64):
    GPU_PANELS[f"mixed_h{_H}"] = _spec(_H, 100000 + 100 * _H, wide=False)
    GPU_PANELS[f"mixed_wide_h{_H}"] = _spec(_H, 200000 + 100 * _H, wide=True)
for _H, _seed in ((16, 301600), (64, 306450)):   # (seeds at which no chain, the shortest included, is half k_prep_bi's objects)
    GPU_PANELS[f"few_bi_h{_H}"] = _spec(_H, _seed, bi_small_share=0.3)
for _H in (100, 128):
    GPU_PANELS[f"mixed_wide_h{_H}"] = _spec(_H, 200000 + 100 * _H, wide=True)
GPU_PANELS["mixed_h128"] = _spec(128, 112800, wide=False)
GPU_PANELS["mixed_wide_h200"] = _spec(200, 220020, lengths=(60,), bi_small_share=0.3, wide=True)
GPU_PANELS["emission_h16"] = _spec(16, 401600, lengths=(120,), wide=True)
for _H in (16, 32, 64):
    GPU_PANELS[f"bi_h{_H}"] = _spec(_H, 500010 + 100 * _H, biallelic=True)
    GPU_PANELS[f"bi_small_h{_H}"] = _spec(_H, 600000 + 100 * _H, biallelic=True, bi_small_share=1.0)
GPU_PANELS["cohort_h16"] = _spec(16, 701600, lengths=(161, 64), wide=True)
GPU_PANELS["cohort_h64"] = _spec(64, 706400, lengths=(161, 64), wide=True)


@lru_cache(maxsize=None)
def gpu_panel(name: str):
    """The chains of the named job as a tuple of ContigBatch (shared between tests: read, never written)."""
    H, seed, lengths, kw = GPU_PANELS[name]
    batches = tuple(structured_panel(v, H, seed + i, **dict(kw)) for i, v in enumerate(lengths))
    if name in REG0_PANELS:
        from oracle import pyoracle as orc   # (test infrastructure, as this module)
        table = orc.OracleTable(*TABLE_ARGS, 0.0)
        batches = tuple(clear_of_denormal_products(b, table) for b in batches)
    return batches


# The reference's long doubles turn denormal below 2^-16382 and lose a mantissa bit per binary order of magnitude from there
# down to 2^-16445.  A column whose emission products lie there is, in the reference itself, rounding noise that the
# normalisation then spreads over the chain (tests/parity_util.py allows for it in a bin's own value only).  Without
# regularisation a product can land anywhere; the panels the GPU tests run without regularisation are chosen so that none does:
# every positive product stays 2^332 (1e100: room for the transition factors and the normalised column it is multiplied with)
# above the denormal range.
DENORMAL_RISK_BELOW = np.ldexp(LD(1), -16382 + 332)
REG0_PANELS = ("mixed_wide_h16", "mixed_wide_h64", "bi_h64", "emission_h16")


def denormal_risk(batch: ContigBatch, table) -> list:
    """the objects with a positive emission product below DENORMAL_RISK_BELOW under `table`"""
    out = []
    for v in range(batch.n_variants):
        E, _ = emission_restatement(batch, table, v)
        if ((E > 0) & (E < DENORMAL_RISK_BELOW)).any():
            out.append(v)
    return out


def clear_of_denormal_products(batch: ContigBatch, table) -> ContigBatch:
    """`batch` with the first k-mer of every object of denormal_risk() read 60000 times: every product of such an object is then
    exactly 0 (an all-zero object, which both sides treat alike) instead of a value the reference cannot hold."""
    kc = batch.kmer_count.copy()
    for v in denormal_risk(batch, table):
        kc[int(batch.kmer_off[v])] = 60000
    return batch.with_counts(kc, batch.coverage)
