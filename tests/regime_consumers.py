"""The regime jobs of tests/transition_regimes.py as input of every per-variant consumer (helpers of
tests/test_regime_consumers_cpu.py and tests/test_regime_consumers_gpu.py; no test here, and nothing of transition_regimes.py is
changed): calls, record calls, record GL, record text, record lines, combined bins and their calls and records had met job-made
bins at make_params(1.26, False, 1e-5) with the regularised table only — no all-zero variant, no tie, no flat posterior, no record
left to the host in the middle of a chain's packed text.

FAMILIES names the families by the route the consumers take (one 64-path chain in pieces; three chains of 16 / 27 / 64 paths with
multiallelic and wide objects; wide columns through aux slots; 200 paths; a cohort with index-level arrays and plans shared per index
contig; a cohort with bubbles of up to 40 alleles, whose records reach the wave-per-record kernels), each under every regime.
tie_job() is a seventh job: uniform transitions — every column independent of the others — over chains of 12, 24 and 48 paths (and a
fourth of 12, the singleton of the combine plan) whose TIE variants carry no k-mer and have their reference allele on two thirds of
the paths, so that the bins are (n0^2, 2 n0 n1, n1^2) = (64, 64, 16) (H / 12)^2 and 0/0 ties with 0/1 exactly; BALANCED variants
(n0 = n1: GL(0/0) = GL(1/1) under a unique 0/1) and ordinary ones stand among them.  A tie is, by the rule below, a record whose
answer a 1e-6 change of the bins overturns, so it is left out of the end-to-end comparison like any other: tie_job's chains have
1500 variants for their ten ties, which keeps them under the 1 % cap that holds for every case.

What is left out of the end-to-end comparison (device vs the yardstick on the ORACLE's bins; GT and GQ only): a variant or record
whose own answer on the oracle's bins is unstable under a relative change of 1e-6 of the bins (tests/parity_util.py: REL_TOL) —
the margin between the best and any other normalised likelihood within 2e-6 * best of 0 or of the reference's 1e-10 tie window's
edge, or -10 log10(1 - best) within 1e-5 of an integer.  Evaluated in long double on the oracle's bins alone (unstable()), shared
by both tests so that both count the same records.  One kind of record is compared by a rule of its own instead of being left out:
a prob_wrong of a few 2^-64 quanta, where rounding moves GQ between 10000, 192, 189 ... (gq_allowed(): GT identical, GQ among the
values rounding can give).
Reference: src/genotypingresult.cpp:118-210, src/graph.cpp:217-273, src/variant.cpp:357-384."""
from __future__ import annotations

import zlib
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from pangenie_amd.genotyping_result import fold_onto_record, results_from_flat
from pangenie_amd.panel import ContigBatch, synthetic_panel
from tests import transition_regimes as tr
from tests.parity_util import REL_TOL
from tests.record_calls_util import random_plan

LD = np.longdouble
FAMILIES = ("lean, sparse, in pieces", "general, chunked", "wide, fused", "generic", "split path, cohort",
            "split path, cohort, objects of more than 32 alleles")
WIDE_FAMILY = FAMILIES[5]
TIE = "tie_job"
TIE_PATHS = (12, 24, 48, 12)
TIE_V = 1500
TIE_SEED = 3001
N_TIES = 10
LEFT_OUT_MAX = 0.01
TIE_WINDOW = LD("0.0000000001")   # src/genotypingresult.cpp:172
# the environment of tie_job: the general kernel at every padded path count (48 paths of two-allele objects are k_sweep_leanx's otherwise)
TIE_ENV = SimpleNamespace(mode="chunked", kernels="general", chunk_cols=64, piece_chunks=None,
                          want=("k_sweep<16,4><1>", "k_sweep<32,8><1>", "k_sweep<64,16><1>", "k_post"), unwanted=("k_sweep_lean",))


def cases():
    """(family, regime, regularisation) of every case; tie_job last"""
    return [(f, r[0], reg) for f in FAMILIES for r in tr.REGIMES for reg in tr.FAMILY[f].regs] + [(TIE, "uniform", 0.01)]


def case_id(c):
    return f"{c[0]}-{c[1]}-reg{c[2]}"


def env(case):
    return TIE_ENV if case[0] == TIE else tr.FAMILY[case[0]]


# ---- tie_job --------------------------------------------------------------------------------------------------------------------
def _without_kmers(b: ContigBatch, variants, path_rows) -> ContigBatch:
    """`b` with the given two-allele variants stripped of their k-mers and of any undefined flag, their paths' alleles replaced"""
    V, H = b.n_variants, b.n_paths
    K = np.diff(b.kmer_off.astype(np.int64))
    keep = np.ones(int(b.kmer_off[-1]), bool)
    pa = b.path_allele.reshape(V, H).copy()
    flags, koff, kmask = b.allele_flags.copy(), b.allele_kmer_off.copy(), b.allele_kmer_mask.copy()
    for v, row in zip(variants, path_rows):
        a0, a1 = int(b.allele_off[v]), int(b.allele_off[v + 1])
        assert a1 - a0 == 2
        keep[int(b.kmer_off[v]):int(b.kmer_off[v + 1])] = False
        K[v] = 0
        flags[a0:a1], koff[a0:a1], kmask[a0:a1] = 0, 0, 0
        pa[v] = row
    kmer_off = np.zeros(V + 1, np.uint32)
    np.cumsum(K, out=kmer_off[1:])
    return ContigBatch(H, b.variant_pos, b.coverage, kmer_off, b.kmer_count[keep], b.allele_off, b.allele_id, flags, koff, kmask, pa.reshape(-1))


@lru_cache(maxsize=None)
def tie_job():
    """-> (index, None, chains, plans, ties, balanced): four chains (every chain its own index contig), a record plan per chain,
    and per chain the variants that tie and those that are balanced.  Per chain: variant 0 is no column (every path on the reference
    allele), so the tie at variant 1 is the chain's first kept column; the tie at V - 1 is its last; one tie is the variant whose
    first record is record 256 k of the chain's plan; seven more in between."""
    chains, plans, ties, balanced = [], [], [], []
    for c, H in enumerate(TIE_PATHS):
        base = synthetic_panel(TIE_V, H, 20, seed=TIE_SEED + c, zero_kmer_frac=0.02)
        plan = random_plan(np.random.default_rng(TIE_SEED + 100 + c), base)
        bal = [60 + 140 * i for i in range(10)]
        fixed = [1, TIE_V - 1] + [130 + 190 * i for i in range(7)]
        at_256 = [v for v in range(2, TIE_V - 1) if int(plan.rec_off[v]) % 256 == 0 and v not in bal and v not in fixed]
        if not at_256:
            raise ValueError(f"tie_job: chain {c} has no free variant whose first record is a multiple of 256")
        tie = sorted(fixed + [at_256[0]])
        assert len(set(tie)) == N_TIES and not set(tie) & set(bal)
        n0 = 2 * H // 3
        assert 3 * n0 == 2 * H
        row = lambda zeros: np.concatenate([np.zeros(zeros, np.uint16), np.ones(H - zeros, np.uint16)])
        b = _without_kmers(base, [0] + tie + bal, [row(H)] + [row(n0)] * len(tie) + [row(H // 2)] * len(bal))
        chains.append(b)
        plans.append(plan)
        ties.append(tie)
        balanced.append(bal)
    return tuple(chains), None, tuple(chains), tuple(plans), tuple(ties), tuple(balanced)


# ---- regularisation 0: variants whose bins are all zero -------------------------------------------------------------------------------
# The bins of a kept variant are all zero only if the backward column there is (src/hmm.cpp:347-368): every path pair's emission at
# the NEXT column is 0 while that object's emissions are not ALL 0 (then get_emission_probability answers 1 for every pair:
# src/emissionprobabilitycomputer.cpp:24-32).  The unregularised table's only exact zeros are those of counts far beyond its
# range, and they are 0 for every copy number: the jobs of transition_regimes.py hold no such variant under any regime (measured:
# none in 15 cases).  So the regularisation-0 cases here run family_job's chains with two changes: at a few variants every path
# carries allele 1 and the read counts are 27 on the k-mers of allele 0 and 0 elsewhere; and the table's entry (coverage, 27) is
# exactly 0 for copy number 0 (ProbabilityTable::modify_probability).  Every genotype a path pair can form there has copy
# number 0 on a k-mer seen 27 times, the genotypes with allele 0 do not: the variant BEFORE has all-zero bins, the forward column
# AT it falls back to uniform.  And one variant a chain (deep_target) gets read counts of a few hundred on all its k-mers, chosen by
# the table itself so that its largest emission product is about 2^-16340: its bins lie below the 2^-16300 under which the device
# leaves call, values and text to the host and above the long double's denormals — a deferred record in the middle of
# a chain's packed text, which no honest draw of counts gives (the window is 25 decades of 4900).
ZERO_COUNT = 27


def zero_table(table):
    """the table of the regularisation-0 cases (hmm.ProbabilityTable or the oracle's): P(count 27 | copy number 0) = 0 at every coverage"""
    for cov in range(tr.TABLE_ARGS[0], tr.TABLE_ARGS[1]):
        p = table.get(cov, ZERO_COUNT)
        table.modify(cov, ZERO_COUNT, 0.0, p[1], p[2])
    return table


def zero_targets(ix: ContigBatch) -> list:
    """the variants changed in a regularisation-0 case: the one before each is meant to have all-zero bins (the chain's first
    column, both sides of column 64, two in a row, the one before the last)"""
    V = ix.n_variants
    out = []
    for t in (1, 31, 32, 64, 65, 120, V - 1):
        while t < V and int(ix.allele_kmer_mask[int(ix.allele_off[t])]) == 0:   # (allele 0 needs k-mers of its own)
            t += 1
        if t < V and t not in out:
            out.append(t)
    return out


def _zero_index(ix: ContigBatch) -> ContigBatch:
    V, H = ix.n_variants, ix.n_paths
    pa, flags = ix.path_allele.reshape(V, H).copy(), ix.allele_flags.copy()
    for t in zero_targets(ix):
        pa[t] = 1
        flags[int(ix.allele_off[t]) + 1] = 0
    return ContigBatch(H, ix.variant_pos, ix.coverage, ix.kmer_off, ix.kmer_count, ix.allele_off, ix.allele_id, flags, ix.allele_kmer_off,
                       ix.allele_kmer_mask, pa.reshape(-1))


def deep_target(ix: ContigBatch) -> int:
    """the variant of a regularisation-0 case whose bins are meant to lie below the device's 2^-16300: a two-allele object with
    k-mers on both alleles, away from zero_targets"""
    taken = {t + d for t in zero_targets(ix) for d in (-2, -1, 0, 1)}
    for v in range(100, ix.n_variants - 2):
        a0 = int(ix.allele_off[v])
        if int(ix.allele_off[v + 1]) - a0 == 2 and v not in taken and ix.allele_kmer_mask[a0] and ix.allele_kmer_mask[a0 + 1] and not ix.allele_flags[a0 + 1]:
            return v
    raise ValueError("no variant for deep_target")


DEEP_LOG2 = (-16355, -16325)   # where the largest emission of deep_target is put: H^2 <= 2^12 path pairs at most below it, the bins stay normal long doubles (>= 2^-16382) under 2^-16300


@lru_cache(maxsize=None)
def _deep_counts(cov: int, n0: int, n1: int):
    """read counts (c + 1 on the first m k-mers, c on the others) at which the largest of the three genotypes' emission products of
    a two-allele object — n0 k-mers on allele 0, then n1 on allele 1 — lies within DEEP_LOG2, by the unregularised table itself"""
    from oracle import pyoracle as orc
    table = zero_table(orc.OracleTable(*tr.TABLE_ARGS, 0.0))
    cn = np.array([[2] * n0 + [0] * n1, [1] * (n0 + n1), [0] * n0 + [2] * n1])   # copy number of every k-mer under 0/0, 0/1, 1/1
    lo, hi = (LD(x) * np.log10(LD(2)) for x in DEEP_LOG2)
    for c in range(100, 900):
        with np.errstate(divide="ignore"):
            logs = [np.log10(table.get(cov, c)), np.log10(table.get(cov, c + 1))]
        for m in range(n0 + n1):
            top = max(sum(logs[1 if k < m else 0][cn[g][k]] for k in range(n0 + n1)) for g in range(3))
            if lo <= top <= hi:
                return c, m
    raise ValueError("no counts put the emissions into DEEP_LOG2")


def _zero_counts(ix: ContigBatch, kmer_count: np.ndarray, coverage: np.ndarray) -> np.ndarray:
    kc = kmer_count.copy()
    d = deep_target(ix)
    a0, k0 = int(ix.allele_off[d]), int(ix.kmer_off[d])
    n0, n1 = (bin(int(ix.allele_kmer_mask[a0 + i])).count("1") for i in (0, 1))
    assert int(ix.allele_kmer_off[a0]) == 0 and int(ix.allele_kmer_off[a0 + 1]) == n0 and int(ix.kmer_off[d + 1]) - k0 == n0 + n1
    c, m = _deep_counts(int(coverage[d]), n0, n1)
    kc[k0:k0 + n0 + n1] = c
    kc[k0:k0 + m] = c + 1
    for t in zero_targets(ix):
        k0, a0 = int(ix.kmer_off[t]), int(ix.allele_off[t])
        kc[k0:int(ix.kmer_off[t + 1])] = 0
        first, n = k0 + int(ix.allele_kmer_off[a0]), bin(int(ix.allele_kmer_mask[a0])).count("1")
        kc[first:first + n] = ZERO_COUNT
    return kc


@lru_cache(maxsize=None)
def _zero_job(case):
    index, samples, chains = tr.family_job(*case)
    new_index = tuple(_zero_index(ix) for ix in index)
    if samples is None:
        new_index = tuple(ix.with_counts(_zero_counts(ix, ix.kmer_count, ix.coverage), ix.coverage) for ix in new_index)
        return new_index, None, new_index
    new_samples = [([_zero_counts(ix, kc, cv) for ix, kc, cv in zip(index, kcs, covs)], list(covs)) for kcs, covs in samples]
    new_chains = tuple(ix.with_counts(kcs[c], covs[c]) for kcs, covs in new_samples for c, ix in enumerate(new_index))
    return new_index, new_samples, new_chains


# ---- jobs, oracle results, plans, prefixes, combine plans ---------------------------------------------------------------------------
def job_of(case):
    """-> (index, samples, chains) as tr.family_job gives them (regularisation 0: with the changes above)"""
    return tie_job()[:3] if case[0] == TIE else _zero_job(case) if case[2] == 0.0 else tr.family_job(*case)


def table_of(case, cls):
    """the case's table: cls(*TABLE_ARGS, regularisation), and at regularisation 0 zero_table of it"""
    t = cls(*tr.TABLE_ARGS, case[2])
    return zero_table(t) if case[2] == 0.0 else t


_own_oracle = {}


def oracle_of(case):
    """the CPU oracle's result of every chain (computed once, shared, never written)"""
    if case[0] != TIE and case[2] != 0.0:
        return tr.oracle_chains(*case)
    if case not in _own_oracle:
        from oracle import pyoracle as orc
        table, params = table_of(case, orc.OracleTable), orc.make_params(*tr.regime_params(case[1]))
        _own_oracle[case] = tuple(orc.genotype_contig(b, table, params) for b in job_of(case)[2])
    return _own_oracle[case]


def index_of_chain(case, c: int) -> int:
    index, samples, _ = job_of(case)
    return c % len(index) if samples is not None else c


def _with_identity_records(plan, batch, above: int):
    """`plan` with one more record — every bubble allele its own record allele, all of them defined — on every bubble of more than
    `above` alleles: A (A + 1) / 2 values a record, which random_plan's records of at most six alleles never have"""
    from pangenie_amd.calls import RecordPlan
    bubbles = []
    for v in range(plan.n_variants):
        recs = []
        for r in range(int(plan.rec_off[v]), int(plan.rec_off[v + 1])):
            own, vcf = plan.record(r)
            recs.append(([int(x) for x in own], [int(x) != 0xFFFF for x in vcf]))
        a0, a1 = int(batch.allele_off[v]), int(batch.allele_off[v + 1])
        n_ids = int(batch.allele_id[a0:a1].max()) + 1
        if a1 - a0 > above:
            recs.append((list(range(n_ids)), [True] * n_ids))
        bubbles.append(recs)
    return RecordPlan.from_records(bubbles)


@lru_cache(maxsize=None)
def plans_of(family: str):
    """a random_plan per index contig (1 - 3 records a bubble, a tenth of the record alleles undefined); the plans depend on the
    index's alleles alone, so every regime and regularisation of a family shares them.  The 40-allele family: an identity record
    more on every bubble of more than 32 alleles."""
    if family == TIE:
        return tie_job()[3]
    index = tr.family_job(family, "strong", 0.01)[0]
    rng = np.random.default_rng(zlib.crc32(family.encode()))
    plans = [random_plan(rng, ix) for ix in index]
    if family == WIDE_FAMILY:
        plans = [_with_identity_records(p, ix, tr.IX_THREAD_AMAX) for p, ix in zip(plans, index)]
    return tuple(plans)


def prefixes_of(family: str):
    """short random fixed columns per index contig (tests/test_record_lines_gpu.py: random_prefix)"""
    from tests.test_record_lines_gpu import random_prefix
    rng = np.random.default_rng(zlib.crc32(family.encode()) + 1)
    return [random_prefix(rng, p.n_records) for p in plans_of(family)]


def combine_plans(case):
    """the combine plans a case is run with, one after the other ([] for the families that are no cohort): a group of three chains
    over one index contig and a singleton.  The 40-allele cohort has two chains in all and a chain may be listed once, so it
    runs its pair, then its two singletons."""
    if case[0] == TIE:
        return [[[0, 1, 2], [3]]]
    if case[0] == "split path, cohort":
        return [[[0, 2, 4], [5, 1], [3]]]   # chain = sample * 2 + contig
    if case[0] == WIDE_FAMILY:
        return [[[0, 1]], [[1], [0]]]
    return []


# ---- the yardstick on long-double bins, and what is unstable --------------------------------------------------------------------------
QUANTUM = np.ldexp(LD(1), -64)   # the spacing of long doubles in [0.5, 1): 1 - best is a whole number of these


def _gq(wrong) -> int:
    return int(-10 * np.log10(wrong)) if wrong > 0 else 10000


def unstable(values) -> bool:
    """of the normalised likelihoods of one map (one variant's, or one record's after fold and get_specific_likelihoods): a relative
    change of REL_TOL of the bins may change GT or GQ — the margin between the best and any other value within 2e-6 * best of 0
    or of the tie window's edge, or -10 log10(1 - best) within 1e-5 of an integer.  Such a variant or record is left out."""
    x = np.asarray(values, LD)
    if x.size == 0 or not x.max() > 0:
        return False
    i = int(np.argmax(x))
    best = x[i]
    d = best - np.delete(x, i)
    eps = LD(2 * REL_TOL) * best
    if d.size and bool(((np.abs(d) <= eps) | (np.abs(d - TIE_WINDOW) <= eps)).any()):
        return True
    wrong = LD(1) - best
    if wrong > 0:
        q = LD(-10) * np.log10(wrong)
        return bool(abs(q - np.rint(q)) <= LD("0.00001"))
    return False


MAX_QUANTA = 4096   # (a record that merges every allele of a 40-allele bubble adds 820 values)


def gq_allowed(values, roundings: int = 2, extra_quanta=0):
    """None, or the GQ values that rounding alone decides between.  The host forms prob_wrong as 1 - best, a whole number k of
    2^-64 quanta, and GQ is 10000 at k = 0, 192 at k = 1, 189 at k = 2, 187, 186 ...: where the TRUE prob_wrong — the sum of the
    other values, which long double holds to 19 digits however small — is a few quanta, the last bit of a bin decides k, and the
    oracle's bins (64-bit mantissas) and the device's (fp64 mantissas, and 1e-15 apart) need not round alike.  What the first GPU
    run of tie_job showed: 10000 against 192 and 189 on records the two rules above keep, a few in a thousand.  Up to 7 % of a
    case's variants have such a prob_wrong (two decades of the thirty it spreads over); of the records, 0 to three quarters
    (the regularisation-0 cases: flat posteriors under records that merge alleles; profiles/r30_regime_consumers.txt).  They are NOT left out: GT must be identical and
    GQ must be one of _gq(k * 2^-64) for the k within `roundings` roundings of the true value, each rounding worth at most
    min(true prob_wrong, one quantum) — the sum and the quotient; for a record one more per key folded and the second quotient.
    A prob_wrong far below a quantum gives exactly 1 whatever the last bits are: None, compared exactly, like everything else —
    as long as best is ONE normalised value.  A record's best may be the sum of several bubble keys (a record that merges
    alleles; all of them: a single key whose value is the sum of every normalised value, 1 up to rounding, for which the
    reference itself prints 10000, 192 or 189): every further term is worth min(the term, one quantum) (`extra_quanta`, in quanta).
    More than MAX_QUANTA candidates: the values differ because an integer lies between them, which unstable() is about."""
    x = np.asarray(values, LD)
    if x.size == 0 or not x.max() > 0:
        return None
    true_wrong = np.delete(x, int(np.argmax(x))).sum() if x.size > 1 else LD(0)
    if not (true_wrong > 0 or extra_quanta):
        return None
    slop = LD(roundings) * min(true_wrong, QUANTUM) + LD(extra_quanta) * QUANTUM
    lo, hi = max(true_wrong * LD(1 - 2 * REL_TOL) - slop, LD(0)), true_wrong * LD(1 + 2 * REL_TOL) + slop
    k_lo, k_hi = int(np.rint(lo / QUANTUM)) if lo < 1 else 1 << 64, int(np.rint(hi / QUANTUM)) if hi < 1 else 1 << 64
    if k_hi - k_lo > MAX_QUANTA or _gq(k_lo * QUANTUM) == _gq(k_hi * QUANTUM):
        return None
    return frozenset(_gq(k * QUANTUM) for k in range(k_lo, k_hi + 1))


def same_call(got, want, allowed) -> bool:
    """a call (allele_1, allele_2, gq[, ...]) or None against the oracle-side answer and its gq_allowed"""
    if got is None or want is None or allowed is None:
        return (got and tuple(got[:3])) == (want and tuple(want[:3]))
    return tuple(got[:2]) == tuple(want[:2]) and got[2] in allowed


def _call(gl):
    g = gl.get_likeliest_genotype()
    if g[0] < 0:
        return None
    wrong = LD(1) - gl.get_genotype_likelihood(*g)
    return int(g[0]), int(g[1]), (int(-10 * np.log10(wrong)) if wrong > 0.0 else 10000)


def answers(batch, lik_ld, kept, allele_present, plan, variants=None):
    """The yardstick (pangenie_amd/genotyping_result.py, long double) on one chain's bins given AS long doubles: per variant
    (allele_1, allele_2, gq) or None, whether that is unstable, whether every bin of a kept variant is zero and whether the ./. is
    a non-unique maximum, its gq_allowed; per record of `plan` (allele_1, allele_2, gq, empty) or None, whether that is unstable, its
    gq_allowed.  `variants`:
    only these (the others' entries are None / False)."""
    V = batch.n_variants
    zeros = np.zeros(V, np.uint16)
    shape = SimpleNamespace(n_variants=V, allele_off=np.asarray(batch.allele_off), allele_id=np.asarray(batch.allele_id), geno_off=batch.geno_off)
    out = SimpleNamespace(calls=[None] * V, unstable=np.zeros(V, bool), all_zero=np.zeros(V, bool), not_unique=np.zeros(V, bool),
                          gq_allowed=[None] * V, rec_calls=[None] * plan.n_records, rec_unstable=np.zeros(plan.n_records, bool),
                          rec_gq_allowed=[None] * plan.n_records)
    todo = set(range(V)) if variants is None else set(int(v) for v in variants)
    for v, res in enumerate(results_from_flat(shape, np.asarray(lik_ld, LD), kept, allele_present, zeros, zeros)):
        if v not in todo:
            continue
        vals = list(res.genotype_to_likelihood.values())
        out.all_zero[v] = bool(vals) and not any(x > 0 for x in vals)
        res.normalize()
        out.calls[v] = _call(res)
        out.not_unique[v] = out.calls[v] is None and any(x > 0 for x in vals)
        out.unstable[v] = unstable(list(res.genotype_to_likelihood.values()))
        out.gq_allowed[v] = gq_allowed(list(res.genotype_to_likelihood.values()))
        for r in range(int(plan.rec_off[v]), int(plan.rec_off[v + 1])):
            own, vcf = plan.record(r)
            f = fold_onto_record(res, own)
            if f.contains_no_likelihoods():
                f.add_to_likelihood(0, 0, 1.0)
            defined = [a for a, x in enumerate(vcf) if int(x) != 0xFFFF]
            gl = f.get_specific_likelihoods(defined) if len(defined) < len(vcf) else f
            c = _call(gl)
            out.rec_calls[r] = None if c is None else c + (res.contains_no_likelihoods(),)
            out.rec_unstable[r] = unstable(list(gl.genotype_to_likelihood.values()))
            if c is not None:
                best = tuple(sorted((defined[c[0]], defined[c[1]])))   # the record alleles of the likeliest genotype
                terms = sorted(x for (a, b), x in res.genotype_to_likelihood.items() if tuple(sorted((int(own[a]), int(own[b])))) == best)
                extra = sum((min(x, QUANTUM) for x in terms[:-1]), LD(0)) / QUANTUM   # (a term far below a quantum changes no bit of the sum)
                out.rec_gq_allowed[r] = gq_allowed(list(gl.genotype_to_likelihood.values()), roundings=3, extra_quanta=extra)
    return out


_oracle_answers = {}


def oracle_answers(case):
    """answers() on the oracle's bins of every chain of a case (computed once, shared, never written)"""
    if case not in _oracle_answers:
        plans = plans_of(case[0])
        _oracle_answers[case] = tuple(answers(b, ref.lik, ref.kept, ref.allele_present, plans[index_of_chain(case, c)])
                                      for c, (b, ref) in enumerate(zip(job_of(case)[2], oracle_of(case))))
    return _oracle_answers[case]


GQ_CLASSES = ("0-30", "31-100", "101-9999", "10000")


def gq_histogram(calls) -> list:
    """the called entries' GQ in four classes"""
    h = [0, 0, 0, 0]
    for c in calls:
        if c is not None:
            h[0 if c[2] <= 30 else 1 if c[2] <= 100 else 2 if c[2] < 10000 else 3] += 1
    return h


def census(case) -> dict:
    """what a case's chains hold, from the oracle's bins alone"""
    ans, refs = oracle_answers(case), oracle_of(case)
    n_var = sum(len(a.calls) for a in ans)
    n_rec = sum(len(a.rec_calls) for a in ans)
    hist = np.sum([gq_histogram(a.calls) for a in ans], axis=0)
    return {"variants": n_var, "records": n_rec,
            "kept": int(sum(int(np.asarray(r.kept, bool).sum()) for r in refs)),
            "all_zero": int(sum(int(a.all_zero.sum()) for a in ans)),
            "called": int(sum(sum(c is not None for c in a.calls) for a in ans)),
            "not_unique": int(sum(int(a.not_unique.sum()) for a in ans)),
            "gq": [int(x) for x in hist],
            "gq_within_quanta": [int(sum(sum(x is not None for x in a.gq_allowed) for a in ans)), int(sum(sum(x is not None for x in a.rec_gq_allowed) for a in ans))],
            "variants_left_out": int(sum(int(a.unstable.sum()) for a in ans)),
            "records_left_out": int(sum(int(a.rec_unstable.sum()) for a in ans))}
