"""Transition regimes and position gaps for every sweep family (helpers of tests/test_transition_regimes_cpu.py and
tests/test_transition_regimes_gpu.py; no test here).

The four per-column constants c0 = r^2, c1 = q r, c2 = q^2 and kappa (pg_kernels.hip: transition_consts; r = exp(-x),
q = (1 - exp(-x)) / H as the reference's 80-bit arithmetic rounds it, x = gap * 0.000004 * recombrate * effective_N / H) come
from four call sites (the two branches of records_unit, k_index_cols, k_index_cols_t) and feed about a dozen column steps.  REGIMES
are parameter triples at which those constants are nothing like the r = 1 - 1e-10, q = 1e-13, kappa = 1 of the suite's usual
make_params(1.26, False, 1e-5); regime_panel() gives a panel positions whose gaps reach q == 0 (gaps of 1, 2, 3 and 7 bp next to
gaps of a few 2^-64 quanta) and, at effective_N = 25000, an fp64-denormal r and r == 0.  FAMILIES is one small job per step
formulation, with the environment that plans it and the kernel names its plan must hold (pg_shim.cpp: kSweep, kBins, kPrepName).
Reference: src/transitionprobabilitycomputer.cpp:8-39.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from pangenie_amd.panel import ContigBatch, synthetic_panel, synthetic_sample_counts

LD = np.longdouble
TABLE_ARGS = (6, 108, 54)   # cov_min, cov_max, count_max; the regularisation (0.01, or 0.0) follows
MIN_VARIANTS = 150
DBL_MIN = 2.2250738585072014e-308

# (name, recombrate, uniform, effective_N, gap rule)
REGIMES = (
    ("uniform", 1.26, True, 1e-5, "base"),
    ("strong", 1.26, False, 25000.0, "base"),
    ("weak", 0.001, False, 1e-5, "base"),
    ("quantised", 1e-9, False, 1e-5, "base"),
    ("underflow", 1.26, False, 25000.0, "base+large"),
)
REGIME = {r[0]: r for r in REGIMES}


def regime_params(regime):
    """(recombrate, uniform, effective_N) of a regime (a name or a row of REGIMES)"""
    row = REGIME[regime] if isinstance(regime, str) else regime
    return row[1], row[2], row[3]


def underflow_gaps(H: int):
    """(gap at which r = exp(-x) is an fp64 denormal: 715 <= x < 745; gap at which it is 0: x >= 800) at x = gap * 0.126 / H"""
    return int(math.ceil(715 * H / 0.126)), int(math.ceil(800 * H / 0.126))


def regime_gaps(V: int, H: int, regime) -> np.ndarray:
    """gaps[i] = pos[i] - pos[i - 1] (gaps[0]: from 10000) of regime_panel"""
    name, _, _, _, rule = REGIME[regime] if isinstance(regime, str) else regime
    if V < MIN_VARIANTS:
        raise ValueError(f"regime_panel needs at least {MIN_VARIANTS} variants, got {V}")
    rng = np.random.Generator(np.random.PCG64([zlib.crc32(name.encode()), V]))
    gaps = 50 + rng.integers(0, 1200, size=V, dtype=np.int64)
    gaps[20:23] = 1
    gaps[60], gaps[61] = 1, 2
    gaps[100:104] = (3, 1, 1, 7)
    if rule == "base+large":
        denormal, zero = underflow_gaps(H)
        gaps[30] = gaps[75] = denormal
        gaps[110] = zero
    return gaps


def _with_positions(batch: ContigBatch, pos: np.ndarray) -> ContigBatch:
    return ContigBatch(batch.n_paths, np.ascontiguousarray(pos, np.uint64), batch.coverage, batch.kmer_off, batch.kmer_count, batch.allele_off,
                       batch.allele_id, batch.allele_flags, batch.allele_kmer_off, batch.allele_kmer_mask, batch.path_allele)


def regime_panel(batch: ContigBatch, regime) -> ContigBatch:
    """`batch` with the positions of the regime (a new ContigBatch: the other arrays are shared and the caller's batch is not written)"""
    gaps = regime_gaps(batch.n_variants, batch.n_paths, regime)
    return _with_positions(batch, (10000 + np.cumsum(gaps)).astype(np.uint64))


def offset_panel(batch: ContigBatch, offset: int) -> ContigBatch:
    """the same panel with every position shifted by `offset`"""
    return _with_positions(batch, batch.variant_pos + np.uint64(offset))


def column_x(batch: ContigBatch, kept: np.ndarray, regime):
    """Of every kept column but the first: x = gap * 0.000004 * recombrate * effective_N / H to the kept column before it, in long
    double as the reference forms it (src/transitionprobabilitycomputer.cpp:14-16)."""
    recomb, _, N = regime_params(regime)
    pos = batch.variant_pos[np.asarray(kept, bool)].astype(np.int64)
    distance = np.diff(pos).astype(LD) * LD("0.000004") * LD(recomb) * LD(N)
    return distance / LD(batch.n_paths)


def regime_census(batch: ContigBatch, kept: np.ndarray, regime) -> dict:
    """What the kept columns of a chain hold under a regime, from the positions alone (numpy, fp64 and long double)."""
    x = column_x(batch, kept, regime)
    with np.errstate(under="ignore"):
        quanta = (LD(1) - np.exp(-x)) * np.ldexp(LD(1), 64)   # q * H * 2^64 of the reference's 80-bit 1 - expl(-x)
        r64 = np.exp(-x.astype(np.float64))
        rld = np.exp(-x)
    zero = quanta == 0
    run = longest = 0
    for z in zero:
        run = run + 1 if z else 0
        longest = max(longest, run)
    return {"q_zero": int(zero.sum()), "q_few": int(((quanta > 0) & (quanta <= 16)).sum()), "q_more": int((quanta > 16).sum()),
            "longest_q_zero_run": longest,
            "r_denormal": int(((r64 > 0) & (r64 < DBL_MIN)).sum()), "r_zero": int((r64 == 0.0).sum()),
            "r_ld_positive_there": bool((rld[r64 < DBL_MIN] > 0).all())}


def predecessor_census(batch: ContigBatch, kept: np.ndarray, min_alleles: int = 0) -> int:
    """the kept columns (of objects with more than `min_alleles` alleles), not the chain's first, whose variant follows one that is
    not kept: where the gap to the variant before is not the gap to the column before"""
    k = np.asarray(kept, bool)
    A = np.diff(batch.allele_off.astype(np.int64))
    return int((k[1:] & ~k[:-1] & (np.cumsum(k)[:-1] > 0) & (A[1:] > min_alleles)).sum())


# ---- the families ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Family:
    name: str
    panels: tuple                 # (V, H, K, seed, synthetic_panel keywords) per batch (cohort: per index contig)
    mode: str | None              # PG_SWEEP_MODE (None: the planner's own choice)
    kernels: str | None           # PG_KERNELS
    chunk_cols: int = 64          # PG_CHUNK_COLS
    piece_chunks: int | None = None   # PG_PIECE_CHUNKS
    want: tuple = ()              # the plan names every one of these ...
    unwanted: tuple = ()          # ... and none of these
    cohort_seeds: tuple = ()      # split path: synthetic_sample_counts seeds, one sample each (over every index contig: seed + contig)
    regs: tuple = (0.01,)         # regularisations the family runs with (0.0: with the suite's zeroed and 60000 counts)
    other: tuple = field(default=())   # (PG_KERNELS, want, unwanted) of the device path it is run beside


_WIDE = dict(wide_frac=0.05, wide_at=(0, 80, 159))
FAMILIES = (
    Family("lean, sparse, in pieces", ((260, 64, 20, 2701, {}),), "chunked", None, 64, 1,
           ("k_sweep_lean<1> (sparse: every 64th column stored, in 3 pieces with k_refill_lean beside them)", "k_sweep_lean<3>", "k_refill_lean", "k_post"),
           regs=(0.01, 0.0), other=("general", ("k_sweep<64,16><1>", "k_post"), ("k_sweep_lean", "k_refill_lean"))),
    Family("lean, dense", ((260, 64, 20, 2701, {}),), "chunked", None, 7, None,
           ("phase 1 = k_sweep_lean<1>;", "k_sweep_lean<3>", "k_post"), ("k_refill_lean", "sparse")),
    Family("lean-x 64", ((200, 64, 20, 2711, dict(multiallelic_frac=0.3)), (170, 50, 20, 2712, {})), "chunked", None, 64, None,
           ("k_sweep_leanx<1>", "k_prep_m4", "k_post")),
    Family("lean-x 128", ((150, 128, 20, 2721, dict(multiallelic_frac=0.3)), (150, 100, 20, 2722, {})), "chunked", None, 64, None,
           ("k_sweep_leanx<1>", "k_post")),
    Family("general, chunked", ((200, 16, 20, 2731, dict(multiallelic_frac=0.3)), (200, 27, 20, 2732, dict(multiallelic_frac=0.2)),
                                (160, 64, 20, 2733, _WIDE)), "chunked", None, 19, None,
           ("k_sweep<16,4><1>", "k_sweep<32,8><1>", "k_sweep<64,16><1>", "k_post")),
    Family("generic", ((150, 200, 20, 2741, dict(multiallelic_frac=0.2)),), None, None, 64, None, ("k_sweep_generic<1>",)),
    Family("triangle lean", ((200, 64, 20, 2751, {}), (200, 64, 20, 2752, {}), (200, 64, 20, 2753, {}), (151, 64, 20, 2754, {})), "fused", None, 64, None,
           ("k_sweep_lean_tri<1>", "k_sweep_lean2", "k_bins_lean2"),
           other=("nolean2,notri", ("k_sweep_lean<1>", "k_sweep<64,16><2>", "bins = k_bins\n"), ("k_sweep_lean_tri", "k_sweep_lean2", "k_bins_lean2"))),
    Family("triangle lean-x", tuple((200, 64, 20, 2761 + i, dict(multiallelic_frac=0.3)) for i in range(3)), "fused", None, 64, None,
           ("k_sweep_leanx_tri", "k_sweep_leanx2", "k_bins_q")),
    Family("wide, fused", tuple((160, 64, 20, 2771 + i, dict(multiallelic_frac=0.2, **_WIDE)) for i in range(2)), "fused", None, 64, None,
           ("k_sweep_leanx_triw", "wide columns to their aux slots", "k_bins_wide")),
    Family("128 paths, fused", tuple((150, 128, 20, 2781 + i, {}) for i in range(2)), "fused", None, 64, None,
           ("k_sweep<128,32><1>", "k_sweep<128,32><2>", "bins = k_bins\n")),
    Family("16 / 32 paths, fused", ((200, 16, 20, 2791, {}), (200, 16, 20, 2792, dict(multiallelic_frac=0.3)), (200, 21, 20, 2793, dict(multiallelic_frac=0.2)),
                                    (200, 32, 20, 2794, {})), "fused", "nosmall", 64, None,
           ("k_sweep<16,4><1>", "k_sweep<16,4><2>", "k_sweep<32,8><1>", "k_sweep<32,8><2>", "k_bins_thin", "k_bins_lean2"), ("k_sweep_small16",)),
    Family("small16, per-sample preparation", tuple((200, 16, 20, 2801 + i, {}) for i in range(4)), "fused", "small,nosplit", 64, None,
           ("k_sweep_small16<1>", "k_sweep_small16<2>", "k_records"), ("k_index_cols", "k_prep_s_", "k_bins_s")),
    Family("split path, cohort", ((200, 16, 20, 2811, {}), (200, 16, 20, 2812, dict(multiallelic_frac=0.3, wide_frac=0.03))), "fused", "small", 64, None,
           ("k_index_cols", "k_prep_s_bi", "k_sweep_small16<2>", "k_sweep_small16x<2>", "k_bins_s"),
           cohort_seeds=(2821, 2831, 2841), regs=(0.01, 0.0),
           other=("small,nosplit", ("k_records", "k_sweep_small16<2>", "k_sweep_small16x<2>"), ("k_index_cols", "k_prep_s_", "k_bins_s"))),
    # (beyond the issue's table: k_index_cols itself takes only the objects of more than PG_IX_THREAD_AMAX = 32 alleles, every other
    #  column of a split chain is k_index_cols_t's — and no panel above holds such an object)
    Family("split path, cohort, objects of more than 32 alleles", ((200, 16, 40, 2852, dict(multiallelic_frac=0.3, max_alleles=40)),), "fused", "small", 64, None,
           ("k_index_cols", "k_prep_s_bi + k_prep_s_m4 + k_prep_s_w", "k_sweep_small16x<2>", "k_bins_s"), cohort_seeds=(2861, 2871),
           other=("small,nosplit", ("k_records", "k_sweep_small16x<2>"), ("k_index_cols", "k_prep_s_", "k_bins_s"))),
)
IX_THREAD_AMAX = 32   # pg_split.h: PG_IX_THREAD_AMAX
FAMILY = {f.name: f for f in FAMILIES}


def _reg0_counts(kmer_count: np.ndarray) -> np.ndarray:
    """the suite's usual counts without regularisation: exact zeros in the table's answers, so that forward columns fall back to
    uniform and backward columns are all zero (tests/test_parity_gpu.py: test_unregularized_table_zero_emissions_vs_oracle)"""
    kc = kmer_count.copy()
    kc[::3] = 0
    kc[1::17] = 60000
    return kc


def family_job(name: str, regime: str, reg: float):
    """-> (index, samples, chains) of a family's job under a regime and a regularisation (shared between tests: read, never written).
    index: the batches the job is made of (a cohort's index contigs); samples: None, or the cohort's [(counts, coverages)] per sample;
    chains: one ContigBatch per chain in the job's order (a cohort: sample * n_contigs + contig), what the oracle is run on."""
    fam = FAMILY[name]
    return _job(tuple((V, H, K, seed, tuple(sorted(kw.items()))) for V, H, K, seed, kw in fam.panels), fam.cohort_seeds, regime, reg)


@lru_cache(maxsize=None)
def _job(panels, cohort_seeds, regime, reg):   # (families over the same panels share their job and its oracle results)
    index = []
    for V, H, K, seed, kw in panels:
        b = regime_panel(synthetic_panel(V, H, K, seed=seed, **dict(kw)), regime)
        if reg == 0.0 and not cohort_seeds:
            b = b.with_counts(_reg0_counts(b.kmer_count), b.coverage)
        index.append(b)
    if not cohort_seeds:
        return tuple(index), None, tuple(index)
    samples = []
    for s in cohort_seeds:
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=s + c) for c, ix in enumerate(index)])
        if reg == 0.0:
            kcs = [_reg0_counts(kc) for kc in kcs]
        samples.append((list(kcs), list(covs)))
    chains = tuple(ix.with_counts(kcs[c], covs[c]) for kcs, covs in samples for c, ix in enumerate(index))
    return tuple(index), samples, chains


_oracle_results = {}


def oracle_chains(name: str, regime: str, reg: float):
    """the CPU oracle's result of every chain of family_job(name, regime, reg): computed once per (panels, regime, regularisation),
    shared, never written"""
    chains = family_job(name, regime, reg)[2]
    if id(chains) not in _oracle_results:
        from oracle import pyoracle as orc   # (test infrastructure, as this module)
        table = orc.OracleTable(*TABLE_ARGS, reg)
        params = orc.make_params(*regime_params(regime))
        _oracle_results[id(chains)] = (chains, tuple(orc.genotype_contig(b, table, params) for b in chains))
    return _oracle_results[id(chains)][1]


def cases():
    """(family, regime, regularisation) of every case of the main test"""
    return [(f.name, r[0], reg) for f in FAMILIES for r in REGIMES for reg in f.regs]


# ---- the grid of the transition entry point -------------------------------------------------------------------------------------
GRID_H = (1, 16, 64, 128, 200)
GRID_GAPS = (1, 2, 7, 43, 44, 50, 1249)
GRID_FROM = 10000
TIE_WINDOW = 0.01     # a grid point whose long-double x * 2^64 lies this close to a half-integer is a tie of rint: left out
TIE_SHARE_MAX = 0.05
P2_FLOOR = 1e-280     # below it every value is at or under the fp64 denormal range (the reference's long double is not)


def grid_gaps(H: int):
    """the gaps of the grid at H paths: the small ones and the three large gaps regime_panel puts on an `underflow` chain (two of
    the three are the same gap: two values)"""
    return GRID_GAPS + underflow_gaps(H)


def grid():
    """[(regime name, recombrate, uniform, effective_N, H, gap)]"""
    return [(name, recomb, uniform, N, H, gap) for name, recomb, uniform, N, _ in REGIMES for H in GRID_H for gap in grid_gaps(H)]


def is_tie(recomb, uniform, N, H, gap) -> bool:
    """x * 2^64 (long double, as the reference forms x) within TIE_WINDOW of a half-integer, where 1 - exp(-x) is rounded to 2^-64
    quanta (x < ln 2 and below 2^52 quanta): the device's fp64 x may fall on the other side of the tie, one quantum away."""
    if uniform:
        return False
    x = LD(gap) * LD("0.000004") * LD(recomb) * LD(N) / LD(H)
    s = x * np.ldexp(LD(1), 64)
    if not (x < LD("0.6931471805599453") and s < np.ldexp(LD(1), 52)):
        return False
    frac = s - np.floor(s)
    return bool(abs(frac - LD("0.5")) < LD(TIE_WINDOW))
