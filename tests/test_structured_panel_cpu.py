"""The structured panels (tests/structured_panel.py) as inputs, on the CPU alone: every panel of
tests/test_structured_objects_gpu.py holds the object classes it is there for, most of its variants are columns, and
without regularisation a good share of its objects has all-zero emissions; the oracle's emission products on such
objects against a second restatement of the reference's loop (src/emissionprobabilitycomputer.cpp:9-53) and its
recursion against the dense-matrix restatement of tests/test_oracle_bruteforce.py; the shares that pg_shim.cpp's
classify_index_contig routes the preparation kernels by."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests.structured_panel import (CENSUS_CLASSES, GPU_PANELS, MULTI_CLASSES, REG0_PANELS, TABLE_ARGS, WIDE_CLASSES, census, denormal_risk,
                                    emission_restatement, gpu_panel, n_bi_small, structured_counts, structured_panel)
from tests.test_oracle_bruteforce import brute_force

LD = np.longdouble
PARAMS = (1.26, False, 1e-5)


def _all_zero_share(batches, reg):
    # (the restatement's flag: the same as the oracle's on every object, test_oracle_emissions_match_the_restatement)
    table = orc.OracleTable(*TABLE_ARGS, reg)
    n = sum(emission_restatement(b, table, v)[1] for b in batches for v in range(b.n_variants))
    return n / sum(b.n_variants for b in batches)


@pytest.mark.parametrize("name", sorted(GPU_PANELS))
def test_gpu_panels_hold_what_they_are_there_for(name):
    H, _, _, kw = GPU_PANELS[name]
    kw = dict(kw)
    batches = list(gpu_panel(name))
    got = census(batches)
    skip = set()
    if kw.get("biallelic"):
        skip |= set(MULTI_CLASSES) | set(WIDE_CLASSES)
        if kw.get("bi_small_share") == 1.0:
            skip.add("two_alleles_K_gt_32")   # (every object has at most 32 k-mers: by construction)
    if H < 8 or not kw.get("wide", True):
        skip |= set(WIDE_CLASSES)
    for cls in CENSUS_CLASSES:
        if cls not in skip:
            assert got[cls] >= 3, (name, cls, got)
    V = sum(b.n_variants for b in batches)
    table = orc.OracleTable(*TABLE_ARGS, 0.01)
    # (which variants are columns does not depend on the counts: without the far counts the oracle's Poisson terms are short loops)
    kept = sum(int(orc.genotype_contig(b.with_counts(np.zeros_like(b.kmer_count), b.coverage), table, orc.make_params(*PARAMS)).kept.sum())
               for b in batches)
    assert kept >= 0.7 * V, (name, kept, V)
    assert _all_zero_share(batches, 0.01) == 0.0
    assert 0.05 <= _all_zero_share(batches, 0.0) <= 0.40


def test_structured_panel_is_deterministic_and_counts_are_another_sample():
    a, b = structured_panel(50, 16, 77), structured_panel(50, 16, 77)
    for f in ("variant_pos", "coverage", "kmer_off", "kmer_count", "allele_off", "allele_id", "allele_flags", "allele_kmer_off",
              "allele_kmer_mask", "path_allele"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    kc, cov = structured_counts(a, 78)
    assert kc.shape == a.kmer_count.shape and cov.shape == a.coverage.shape and kc.dtype == np.uint16
    assert not np.array_equal(kc, a.kmer_count)
    kc2, cov2 = structured_counts(a, 78)
    assert np.array_equal(kc, kc2) and np.array_equal(cov, cov2)
    # the ABI's own rules: ids ascending, masks inside the object, offset = first k-mer set, undefined alleles carry none
    for v in range(a.n_variants):
        a0, a1 = int(a.allele_off[v]), int(a.allele_off[v + 1])
        K = int(a.kmer_off[v + 1] - a.kmer_off[v])
        ids = a.allele_id[a0:a1].astype(np.int64)
        assert (np.diff(ids) > 0).all() and ids.max() <= (a1 - a0) + 6
        assert set(a.path_allele.reshape(-1, 16)[v].tolist()) <= set(ids.tolist())
        for s in range(a0, a1):
            m, off = int(a.allele_kmer_mask[s]), int(a.allele_kmer_off[s])
            if m:
                assert m & 1 and off + m.bit_length() <= K and not (a.allele_flags[s] & 1)
            else:
                assert off == 0


@pytest.mark.parametrize("H", [5, 16, 64])
def test_oracle_emissions_match_the_restatement(H):
    """orc.emission_table against the reference's loop restated in numpy: the same flag, entries within 1e-16 relative (at
    most four roundings per k-mer, 129 k-mers, 2^-64 each)."""
    b = structured_panel(120, H, 8100 + H)
    for reg in (0.01, 0.0):
        table = orc.OracleTable(*TABLE_ARGS, reg)
        n_zero = 0
        for v in range(b.n_variants):
            want, want_flag = emission_restatement(b, table, v)
            got, got_flag = orc.emission_table(b, table, v)
            assert got_flag == want_flag, (H, reg, v)
            n_zero += want_flag
            if want_flag:
                continue   # (what the oracle hands out for an all-zero object is its own business: the flag is what is read)
            den = np.maximum(np.abs(got), np.abs(want))
            rel = np.where(den > 0, np.abs(got - want) / np.where(den > 0, den, 1), 0)
            assert float(rel.max()) <= 1e-16, (H, reg, v, float(rel.max()))
            assert ((got == 0) == (want == 0)).all()
        assert (n_zero == 0) if reg else (n_zero >= 6)


@pytest.mark.parametrize("V,H,wide", [(25, 4, False), (20, 6, False), (14, 12, True)])
def test_oracle_matches_dense_matrix_restatement_on_structured_panels(V, H, wide):
    b = structured_panel(V, H, 8200 + V + H, wide=wide)
    if wide:
        assert census(b)["wide_column"] >= 1
    for reg in (0.01, 0.0):
        table = orc.OracleTable(*TABLE_ARGS, reg)
        ref = orc.genotype_contig(b, table, orc.make_params(*PARAMS))
        lik, kept = brute_force(b, table, *PARAMS)
        assert (kept == ref.kept).all() and kept.sum() >= 0.5 * V
        den = np.maximum(np.abs(lik), np.abs(ref.lik))
        rel = np.where(den > 0, np.abs(lik - ref.lik) / np.where(den > 0, den, 1), 0)
        assert float(rel.max()) < 1e-13, (reg, float(rel.max()))
        assert ((lik == 0) == (ref.lik == 0)).all()


@pytest.mark.parametrize("H", [16, 64])
def test_shares_fall_on_the_intended_side_of_the_preparation_threshold(H):
    """classify_index_contig: prep_fast = 2 (k_prep_bi + k_prep_m4 + k_prep) iff at least half of a chain's objects have two alleles
    and at most 32 k-mers — pure Python over the arrays, so that the GPU cases cannot quietly route everything to k_prep."""
    many = gpu_panel(f"mixed_wide_h{H}")
    few = gpu_panel(f"few_bi_h{H}")
    for b in many:
        if b.n_variants >= 90:
            assert 2 * n_bi_small(b) >= b.n_variants
            A = np.diff(b.allele_off.astype(np.int64))
            K = np.diff(b.kmer_off.astype(np.int64))
            assert ((A >= 3) & (A <= 5) & (K <= 64)).sum() >= 3 and ((A == 2) & (K > 32)).sum() >= 3   # k_prep_m4's and k_prep's
    for b in few:
        assert 2 * n_bi_small(b) < b.n_variants
    for name in (f"bi_small_h{H}",):
        for b in gpu_panel(name):
            assert n_bi_small(b) == b.n_variants
    assert any(n_bi_small(b) < b.n_variants for b in gpu_panel(f"bi_h{H}"))


@pytest.mark.parametrize("name", REG0_PANELS)
def test_panels_run_without_regularisation_stay_clear_of_the_denormal_range(name):
    """No emission product of a panel that the GPU tests run at regularisation 0 lies within 2^332 of the reference's denormal
    range (tests/structured_panel.py: DENORMAL_RISK_BELOW), where the reference's own columns are rounding noise; the objects that
    were moved out of it (made all-zero objects) are few."""
    H, seed, lengths, kw = GPU_PANELS[name]
    table = orc.OracleTable(*TABLE_ARGS, 0.0)
    moved = 0
    for i, (V, b) in enumerate(zip(lengths, gpu_panel(name))):
        assert denormal_risk(b, table) == []
        raw = structured_panel(V, H, seed + i, **dict(kw))
        moved += len(denormal_risk(raw, table))
        assert int((raw.kmer_count != b.kmer_count).sum()) == len(denormal_risk(raw, table))
    assert 1 <= moved <= 0.02 * sum(lengths), moved
