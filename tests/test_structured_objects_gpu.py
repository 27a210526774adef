"""The per-variant kernels on objects `synthetic_panel` never builds (tests/structured_panel.py): allele ids that are not the
slots, objects without allele 0, k-mers on several alleles and on none, masks with holes, two-allele objects of more than 32
k-mers, several undefined alleles in any slot, all paths on one non-reference allele.  Every case runs the device, checks on the
job's plan that the kernels it is meant to reach are the ones planned, and compares every chain with the CPU oracle (1e-6 relative
on every bin, identical calls, kept, allele_present, n_kmers, coverage); two device paths side by side agree within 1e-10; a second
run of every job gives the same bits.  Kernel names: kPrepName and the sweep and bins tables of pangenie_amd/csrc/pg_shim.cpp.
The panels (tests/structured_panel.py: GPU_PANELS) are held to their census by tests/test_structured_panel_cpu.py; those run at
regularisation 0 hold no emission product near the reference's denormal range (REG0_PANELS).
Reference: src/emissionprobabilitycomputer.cpp:9-53, src/kmerpath.cpp:33-48, src/columnindexer.cpp:24-31, src/hmm.cpp:175-405."""
import numpy as np
import pytest

from pangenie_amd import hmm
from tests.parity_util import assert_parity, log_parity
from tests.structured_panel import TABLE_ARGS, census, gpu_panel, structured_counts

pytestmark = pytest.mark.gpu

PARAMS = (1.26, False, 1e-5)
PREP_LISTS = "per run k_prep_bi + k_prep_m4 + k_prep + k_records"
PREP_BI = "per run k_prep_bi + k_records"
PREP_W = "per run k_prep + k_records"
PREP_S_BI = "k_index_cols); per run k_prep_s_bi"
PREP_S_LISTS = "k_index_cols); per run k_prep_s_bi + k_prep_s_m4 + k_prep_s_w"
SPLIT_INDEX = "index pass once (k_index_scan, k_compact, k_index_cols)"
HP_KERNEL = {16: "k_sweep<16,4>", 32: "k_sweep<32,8>", 64: "k_sweep<64,16>", 128: "k_sweep<128,32>"}
_refs = {}
_seen = set()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _pad(H):
    return next(hp for hp in (16, 32, 64, 128, 256) if H <= hp)


def _oracle(orc, key, batches, reg):
    """the oracle's results of a job's chains: computed once per (panel, regularisation), shared, never written"""
    if (key, reg) not in _refs:
        table = orc.OracleTable(*TABLE_ARGS, reg)
        _refs[(key, reg)] = [orc.genotype_contig(b, table, orc.make_params(*PARAMS)) for b in batches]
    return _refs[(key, reg)]


def _agree(got, other, tol=1e-10):
    for a, c in zip(got, other):
        a, c = a.likelihoods_ld(), c.likelihoods_ld()
        den = np.maximum(np.abs(a), np.abs(c))
        worst = float(np.where(den > 0, np.abs(a - c) / np.where(den > 0, den, 1), 0).max()) if a.size else 0.0
        assert worst < tol, worst


def _device(monkeypatch, batches, reg, mode, kernels, want, unwanted=(), cohort=None):
    """One job under PG_SWEEP_MODE = mode and PG_KERNELS = kernels: the plan names every kernel of `want` and none of `unwanted`;
    run twice, the same bits; -> (results, plan)."""
    monkeypatch.setenv("PG_SWEEP_MODE", mode)
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    if kernels:
        monkeypatch.setenv("PG_KERNELS", kernels)
    else:
        monkeypatch.delenv("PG_KERNELS", raising=False)
    table, params = hmm.ProbabilityTable(*TABLE_ARGS, reg), hmm.make_params(*PARAMS)
    job = hmm.Job(list(batches), table, params) if cohort is None else hmm.Job.cohort(list(batches), cohort, table, params)
    try:
        plan = job.plan()
        assert job.sweep_mode()[0] == mode, plan
        for name in want:
            assert name in plan, (name, plan)
        for name in unwanted:
            assert name not in plan, (name, plan)
        job.run()
        got = job.fetch_all()
        job.run()
        again = job.fetch_all()
    finally:
        job.close()
    for r, r2 in zip(got, again):
        assert np.array_equal(r.lik, r2.lik) and np.array_equal(r.lik_exp, r2.lik_exp)
        assert np.array_equal(r.kept, r2.kept) and np.array_equal(r.allele_present, r2.allele_present)
    return got, plan


def _parity(orc, name, got, reg, label):
    batches = gpu_panel(name)
    if name not in _seen:
        _seen.add(name)
        log_parity(f"structured panel {name}: census {census(list(batches))}")
    worst = 0.0
    for b, r, ref in zip(batches, got, _oracle(orc, name, batches, reg)):
        worst = max(worst, assert_parity(b, r, ref))
    log_parity(f"structured objects, {label}, panel {name}, regularisation {reg}: worst relative error {worst:.3e}")


def _phase1_chunked(H, wide):
    hp = _pad(H)
    # (64 and 128 padded paths: chains without a wide object on the lean-x step, those with one on the general kernel)
    return ([HP_KERNEL[hp] + "<1>"] if hp < 64 else ["k_sweep_leanx<1>"] + ([HP_KERNEL[hp] + "<1>"] if wide else []))


# ---- 1: chunked, mixed objects, at least half of them k_prep_bi's -------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("H", [13, 16, 27, 32, 41, 64])
def test_chunked_mixed_objects_on_the_three_preparation_kernels(H, wide, orc, monkeypatch):
    name = f"mixed_wide_h{H}" if wide else f"mixed_h{H}"
    got, _ = _device(monkeypatch, gpu_panel(name), 0.01, "chunked", None, [PREP_LISTS, "k_post"] + _phase1_chunked(H, wide))
    _parity(orc, name, got, 0.01, "chunked, k_prep_bi + k_prep_m4 + k_prep")


# ---- 2: few two-allele objects (k_prep for everything), and more than 64 paths -------------------------------------------------
@pytest.mark.parametrize("H", [16, 64])
def test_chunked_few_biallelic_objects_all_on_k_prep(H, orc, monkeypatch):
    name = f"few_bi_h{H}"
    got, _ = _device(monkeypatch, gpu_panel(name), 0.01, "chunked", None, [PREP_W, HP_KERNEL[H] + "<1>", "k_post"], ["k_prep_bi", "k_prep_m4"])
    _parity(orc, name, got, 0.01, "chunked, prep_fast = 0")


@pytest.mark.parametrize("H", [100, 128, 200])
def test_chunked_more_than_64_paths_all_on_k_prep(H, orc, monkeypatch):
    name = f"mixed_wide_h{H}"
    want = ["k_sweep_generic<1>"] if H == 200 else _phase1_chunked(H, True)
    got, _ = _device(monkeypatch, gpu_panel(name), 0.01, "chunked", None, [PREP_W, "k_post"] + want, ["k_prep_bi", "k_prep_m4"])
    _parity(orc, name, got, 0.01, "chunked, more than 64 paths")


# ---- 3: one wave per object for everything against the default -----------------------------------------------------------------
@pytest.mark.parametrize("H", [16, 64])
def test_prepwave_against_the_three_preparation_kernels(H, orc, monkeypatch):
    name = f"mixed_wide_h{H}"
    default, _ = _device(monkeypatch, gpu_panel(name), 0.01, "chunked", None, [PREP_LISTS])
    wave, _ = _device(monkeypatch, gpu_panel(name), 0.01, "chunked", "prepwave", [PREP_W], ["k_prep_bi", "k_prep_m4"])
    _parity(orc, name, default, 0.01, "chunked, default preparation")
    _parity(orc, name, wave, 0.01, "chunked, PG_KERNELS=prepwave")
    _agree(default, wave)


# ---- 4: the emission entry point -------------------------------------------------------------------------------------------------
def test_emission_table_of_structured_objects(orc):
    """k_emission_single against the oracle's table on every object of one mixed panel with wide objects: 1e-9 relative, the same
    all_zeros flag (the bar of test_emission_vs_oracle_on_the_fly_entries), with and without regularisation."""
    (b,) = gpu_panel("emission_h16")
    for reg in (0.01, 0.0):
        t, ot = hmm.ProbabilityTable(*TABLE_ARGS, reg), orc.OracleTable(*TABLE_ARGS, reg)
        worst, n_zero = 0.0, 0
        for v in range(b.n_variants):
            got, got_flag = hmm.emission_table(b, t, v)
            want, want_flag = orc.emission_table(b, ot, v)
            assert got_flag == want_flag, (reg, v)
            n_zero += want_flag
            den = np.maximum(np.abs(got), np.abs(want))
            rel = np.where(den > 0, np.abs(got - want) / np.where(den > 0, den, 1), 0)
            worst = max(worst, float(rel.max()))
            assert float(rel.max()) < 1e-9, (reg, v, float(rel.max()))
        assert (n_zero == 0) if reg else (n_zero >= 5)
        log_parity(f"structured objects, k_emission_single, panel emission_h16, regularisation {reg}: worst relative error {worst:.3e}")


# ---- 5: fused, 16 paths: the split path, k_bins_x, the general kernel -----------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_fused_16_paths_split_path_nosplit_and_general_kernel(wide, orc, monkeypatch):
    name = "mixed_wide_h16" if wide else "mixed_h16"
    b = gpu_panel(name)
    split, _ = _device(monkeypatch, b, 0.01, "fused", "small",
                       [SPLIT_INDEX, PREP_S_LISTS, "k_sweep_small16x<1>", "k_sweep_small16x<2>", "k_bins_s"] + (["k_bins_wide_s"] if wide else []))
    nosplit, _ = _device(monkeypatch, b, 0.01, "fused", "small,nosplit",
                         [PREP_LISTS, "k_sweep_small16x<1>", "k_sweep_small16x<2>", "k_bins_x"] + (["k_bins_wide"] if wide else []), ["k_prep_s_", "k_bins_s"])
    if wide:   # (a wide column on the general kernel at 16 paths is k_post's: such a job is chunked)
        general, _ = _device(monkeypatch, b, 0.01, "chunked", "nosmall", [PREP_LISTS, "k_sweep<16,4><1>", "k_post"], ["k_sweep_small16", "k_prep_s_"])
    else:
        general, _ = _device(monkeypatch, b, 0.01, "fused", "nosmall", [PREP_LISTS, "k_sweep<16,4><1>", "k_sweep<16,4><2>", "k_bins_thin"],
                             ["k_sweep_small16", "k_prep_s_"])
    _parity(orc, name, split, 0.01, "fused, PG_KERNELS=small (split path)")
    _parity(orc, name, nosplit, 0.01, "fused, PG_KERNELS=small,nosplit")
    _parity(orc, name, general, 0.01, "PG_KERNELS=nosmall")
    _agree(split, nosplit)
    _agree(split, general)


# ---- 6: fused, 32 padded paths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [27, 32])
def test_fused_32_padded_paths(H, orc, monkeypatch):
    name = f"mixed_h{H}"
    got, _ = _device(monkeypatch, gpu_panel(name), 0.01, "fused", None, [PREP_LISTS, "k_sweep<32,8><1>", "k_sweep<32,8><2>", "k_bins_thin"])
    _parity(orc, name, got, 0.01, "fused, k_sweep<32,8>")


# ---- 7: fused, 64 padded paths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 41])
def test_fused_64_padded_paths_narrow_columns(H, orc, monkeypatch):
    """64 paths: triangle storage, phase 1 on k_sweep_leanx_tri, phase 2 on k_sweep_leanx2, k_bins_q; 41 paths (no triangles): the
    general kernel and k_bins.  Against PG_KERNELS=noleanx2 (k_bins)."""
    name = f"mixed_h{H}"
    b = gpu_panel(name)
    want = ["k_sweep_leanx_tri", "k_sweep_leanx2", "k_bins_q"] if H == 64 else ["k_sweep<64,16><1>", "k_sweep<64,16><2>", "bins = k_bins\n"]
    got, _ = _device(monkeypatch, b, 0.01, "fused", None, [PREP_LISTS] + want)
    other, _ = _device(monkeypatch, b, 0.01, "fused", "noleanx2", [PREP_LISTS, "k_sweep<64,16><2>", "bins = k_bins\n"], ["k_sweep_leanx2", "k_bins_q"])
    _parity(orc, name, got, 0.01, "fused, default")
    _parity(orc, name, other, 0.01, "fused, PG_KERNELS=noleanx2")
    _agree(got, other)


@pytest.mark.parametrize("H,reg", [(64, 0.01), (41, 0.01), (64, 0.0)])
def test_fused_64_padded_paths_wide_columns(H, reg, orc, monkeypatch):
    """wide columns leave phase 2 through their aux slots, k_bins_wide forms their bins (64 paths: phase 1 on k_sweep_leanx_triw);
    against the chunked job of PG_KERNELS=nowidef; regularised and not (all-zero objects, fall-back columns)."""
    name = f"mixed_wide_h{H}"
    b = gpu_panel(name)
    got, _ = _device(monkeypatch, b, reg, "fused", None,
                     [PREP_LISTS, "wide columns to their aux slots", "k_bins_wide"] + (["k_sweep_leanx_triw"] if H == 64 else ["k_sweep<64,16><1>"]))
    other, _ = _device(monkeypatch, b, reg, "chunked", "nowidef", [PREP_LISTS, "k_post"], ["aux slots", "k_bins_wide"])
    _parity(orc, name, got, reg, "fused, wide columns to aux slots")
    _parity(orc, name, other, reg, "chunked, PG_KERNELS=nowidef")
    _agree(got, other)


# ---- 8: fused, 128 paths ---------------------------------------------------------------------------------------------------------
def test_fused_128_paths(orc, monkeypatch):
    got, _ = _device(monkeypatch, gpu_panel("mixed_h128"), 0.01, "fused", None, [PREP_W, "k_sweep<128,32><1>", "k_sweep<128,32><2>", "bins = k_bins\n"],
                     ["k_prep_bi", "k_prep_m4"])
    _parity(orc, "mixed_h128", got, 0.01, "fused, k_sweep<128,32>")


# ---- 9: lean chains (every object two alleles, 64 paths) -------------------------------------------------------------------------
@pytest.mark.parametrize("small_only", [True, False])
def test_lean_chains_of_structured_objects(small_only, orc, monkeypatch):
    """Every object with at most 32 k-mers: k_prep_bi alone; the full set of k-mer counts: a lean chain whose objects of more than
    32 k-mers are k_prep's.  Chunked (k_sweep_lean, sparse phase 1) and fused (k_sweep_lean_tri, k_sweep_lean2, k_bins_lean2); the
    first against PG_KERNELS=general."""
    name = "bi_small_h64" if small_only else "bi_h64"
    b = gpu_panel(name)
    prep, never = ([PREP_BI], ["k_prep_m4", "k_prep +"]) if small_only else ([PREP_LISTS], [])
    chunked, _ = _device(monkeypatch, b, 0.01, "chunked", None, prep + ["k_sweep_lean<1> (sparse", "k_sweep_lean<3>", "k_post"], never)
    fused, _ = _device(monkeypatch, b, 0.01, "fused", None, prep + ["k_sweep_lean_tri<1>", "k_sweep_lean2", "k_bins_lean2"], never)
    _parity(orc, name, chunked, 0.01, "chunked, lean chains")
    _parity(orc, name, fused, 0.01, "fused, lean chains")
    _agree(chunked, fused)
    if small_only:
        general, _ = _device(monkeypatch, b, 0.01, "chunked", "general", [PREP_BI, "k_sweep<64,16><1>"], ["k_sweep_lean"])
        _parity(orc, name, general, 0.01, "chunked, PG_KERNELS=general")
        _agree(chunked, general)


def test_lean_chains_without_regularisation(orc, monkeypatch):
    got, _ = _device(monkeypatch, gpu_panel("bi_h64"), 0.0, "fused", None, [PREP_LISTS, "k_sweep_lean_tri<1>", "k_sweep_lean2", "k_bins_lean2"])
    _parity(orc, "bi_h64", got, 0.0, "fused, lean chains")


# ---- 10: every object two alleles, 16 and 32 paths -------------------------------------------------------------------------------
@pytest.mark.parametrize("small_only", [True, False])
def test_fused_biallelic_16_paths_small_kernel_and_class_sums(small_only, orc, monkeypatch):
    name = "bi_small_h16" if small_only else "bi_h16"
    b = gpu_panel(name)
    small, plan = _device(monkeypatch, b, 0.01, "fused", "small", [SPLIT_INDEX, PREP_S_BI, "k_sweep_small16<1>", "k_sweep_small16<2>", "k_bins_s"],
                          ["k_sweep_small16x"] + (["k_prep_s_w"] if small_only else []))
    assert small_only or "k_prep_s_w" in plan, plan
    general, _ = _device(monkeypatch, b, 0.01, "fused", "nosmall", [PREP_BI if small_only else PREP_LISTS, "k_sweep<16,4><1>", "k_sweep<16,4><2>", "k_bins_lean2"],
                         ["k_sweep_small16", "k_prep_s_"])
    _parity(orc, name, small, 0.01, "fused, PG_KERNELS=small (k_sweep_small16)")
    _parity(orc, name, general, 0.01, "fused, PG_KERNELS=nosmall (class sums)")
    _agree(small, general)


def test_fused_biallelic_32_paths(orc, monkeypatch):
    """32 paths, every object two alleles: per-thread partials and k_bins_thin (the class sums of k_bins_lean2 need the whole
    half-chain in one wave — 16 paths, and 32 only in a build with 16 rows per lane, which the shipped one is not: a plan that
    names k_bins_lean2 here would mean the build has changed, and this case with it)."""
    got, _ = _device(monkeypatch, gpu_panel("bi_h32"), 0.01, "fused", None, [PREP_LISTS, "k_sweep<32,8><1>", "k_sweep<32,8><2>", "k_bins_thin"],
                     ["k_bins_lean2"])
    _parity(orc, "bi_h32", got, 0.01, "fused, two-allele objects at 32 paths")


# ---- 11 (the rest of it): the split path without regularisation -----------------------------------------------------------------
def test_split_path_without_regularisation(orc, monkeypatch):
    got, _ = _device(monkeypatch, gpu_panel("mixed_wide_h16"), 0.0, "fused", "small",
                     [SPLIT_INDEX, PREP_S_LISTS, "k_sweep_small16x<1>", "k_bins_s", "k_bins_wide_s"])
    _parity(orc, "mixed_wide_h16", got, 0.0, "fused, PG_KERNELS=small (split path)")


# ---- 12: cohorts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [16, 64])
def test_cohort_over_structured_contigs(H, orc, monkeypatch):
    """Three samples (structured_counts) over an index of two structured contigs; every (sample, contig) chain against the oracle on
    that sample's counts.  16 paths: the split path (PG_KERNELS=small); 64 paths: wide columns through aux slots."""
    name = f"cohort_h{H}"
    index = gpu_panel(name)
    samples = []
    for s in range(3):
        kcs, covs = zip(*[structured_counts(ix, 9000 + 100 * H + 10 * s + c) for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    want = [SPLIT_INDEX, PREP_S_LISTS, "k_sweep_small16x<1>", "k_bins_s", "k_bins_wide_s"] if H == 16 else [PREP_LISTS, "wide columns to their aux slots", "k_bins_wide"]
    got, _ = _device(monkeypatch, index, 0.01, "fused", "small" if H == 16 else None, want, cohort=samples)
    assert len(got) == 3 * len(index)
    table = orc.OracleTable(*TABLE_ARGS, 0.01)
    worst = 0.0
    for s in range(3):
        for c, ix in enumerate(index):
            b = ix.with_counts(samples[s][0][c], samples[s][1][c])
            worst = max(worst, assert_parity(b, got[s * len(index) + c], orc.genotype_contig(b, table, orc.make_params(*PARAMS))))
    log_parity(f"structured panel {name}: census {census(list(index))}")
    log_parity(f"structured objects, cohort of 3 samples, panel {name}: worst relative error {worst:.3e}")
