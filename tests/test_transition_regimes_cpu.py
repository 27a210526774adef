"""The panels of tests/transition_regimes.py held to what they are meant to contain, from the CPU oracle alone: a later change to
synthetic_panel or to the helper must not quietly empty tests/test_transition_regimes_gpu.py.

  - the helper itself: positions only, the caller's batch untouched, the gap rules, the refusal of short panels;
  - the census of every family's chains per regime over the KEPT columns of the oracle's result (the transition of a column runs
    from the kept column before it): q == 0 columns next to columns of a few 2^-64 quanta, fp64-denormal r and r == 0 columns
    where the long-double exp(-x) is positive, kappa = H^2;
  - the documented fp64 range (include/pangenie_hmm.h, numeric contract): in every (panel, regime, regularisation) the reference's
    deepest nonzero bin lies within 10^-300 of its variant's largest bin, so that the GPU test compares every bin;
  - the tie exclusion of the transition grid stays within its 5 %;
  - the oracle's transition probabilities equal, bit for bit, those of the reference's own translation unit
    (oracle/_ref/libref_transitions.so: src/transitionprobabilitycomputer.cpp behind oracle/ref_transitions_shim.cpp).

`quantised`, "a column with more than 16 quanta": x * 2^64 = gap * 4e-20 * 2^64 / H = 0.738 * gap / H exceeds 16.5 at a gap of
1249 bp only below 56 paths, so chains of 64 and more paths reach it only across a variant that is not kept.  It is asserted on
every chain below 56 paths and, per family set, on the union of all chains.
"""
import numpy as np
import pytest

from pangenie_amd.panel import synthetic_panel
from tests import transition_regimes as tr

LD = np.longdouble
JOBS = sorted({(f.name, reg) for f in tr.FAMILIES for reg in f.regs})


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


# ---- the helper -----------------------------------------------------------------------------------------------------------------
def test_regime_panel_changes_positions_only_and_leaves_the_callers_batch():
    b = synthetic_panel(160, 64, 20, seed=3)
    before = {k: getattr(b, k).copy() for k in ("variant_pos", "coverage", "kmer_off", "kmer_count", "allele_off", "allele_id", "allele_flags",
                                                "allele_kmer_off", "allele_kmer_mask", "path_allele")}
    for name, *_ in tr.REGIMES:
        p = tr.regime_panel(b, name)
        assert p is not b and p.n_paths == b.n_paths and p.variant_pos is not b.variant_pos
        for k, v in before.items():
            assert np.array_equal(getattr(b, k), v), k
            if k != "variant_pos":
                assert np.array_equal(getattr(p, k), v), k
        gaps = np.diff(np.concatenate([[10000], p.variant_pos.astype(np.int64)]))
        assert np.array_equal(gaps, tr.regime_gaps(160, 64, name))
        assert list(gaps[20:23]) == [1, 1, 1] and list(gaps[60:62]) == [1, 2] and list(gaps[100:104]) == [3, 1, 1, 7]
        large = {30: 363175, 75: 363175, 110: 406350} if name == "underflow" else {}   # ceil(715 * 64 / 0.126), ceil(800 * 64 / 0.126)
        for i in range(160):
            if i in large:
                assert gaps[i] == large[i]
            elif not (20 <= i < 23 or i in (60, 61) or 100 <= i < 104):
                assert 50 <= gaps[i] < 1250
        assert np.array_equal(tr.regime_panel(b, name).variant_pos, p.variant_pos)   # (its own generator: the same every time)
    assert not np.array_equal(tr.regime_panel(b, "strong").variant_pos, tr.regime_panel(b, "weak").variant_pos)


def test_regime_panel_refuses_short_panels():
    with pytest.raises(ValueError):
        tr.regime_panel(synthetic_panel(149, 16, 20, seed=3), "strong")
    tr.regime_panel(synthetic_panel(150, 16, 20, seed=3), "underflow")


def test_offset_panel_shifts_every_position():
    b = tr.regime_panel(synthetic_panel(150, 16, 20, seed=3), "quantised")
    before = b.variant_pos.copy()
    o = tr.offset_panel(b, 1 << 33)
    assert o.variant_pos.dtype == np.uint64 and np.array_equal(b.variant_pos, before)
    assert np.array_equal(o.variant_pos.astype(object) - (1 << 33), before.astype(object))
    assert int(o.variant_pos.min()) > 1 << 33 and np.array_equal(o.kmer_count, b.kmer_count)


def test_families_are_the_table():
    assert len(tr.FAMILIES) == 14 and len(tr.FAMILY) == 14 and len(tr.REGIMES) == 5   # (the issue's thirteen and one of ours)
    seeds = [p[3] for f in tr.FAMILIES if f.name != "lean, dense" for p in f.panels] + [s + c for f in tr.FAMILIES for s in f.cohort_seeds for c in range(len(f.panels))]
    assert len(set(seeds)) == len(seeds)   # ("lean, dense" runs the panel of "lean, sparse, in pieces")
    for f in tr.FAMILIES:
        assert all(tr.MIN_VARIANTS <= p[0] <= 260 for p in f.panels), f.name
    assert [f.name for f in tr.FAMILIES if 0.0 in f.regs] == ["lean, sparse, in pieces", "split path, cohort"]
    assert len(tr.cases()) == (14 + 2) * 5


# ---- the census -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,reg", JOBS)
def test_census_of_every_chain(family, reg):
    union_more = 0
    for regime, *_ in tr.REGIMES:
        chains = tr.family_job(family, regime, reg)[2]
        for b, ref in zip(chains, tr.oracle_chains(family, regime, reg)):
            assert int(ref.kept.sum()) == ref.n_columns >= 100, (family, regime, ref.n_columns)
            c = tr.regime_census(b, ref.kept, regime)
            if regime == "quantised":
                assert c["q_zero"] >= 1 and c["q_few"] >= 1, (family, c)
                assert c["q_more"] >= 1 or b.n_paths >= 56, (family, b.n_paths, c)
                assert c["longest_q_zero_run"] <= 4, (family, c)
                assert c["r_denormal"] == 0 and c["r_zero"] == 0
                union_more += c["q_more"]
            elif regime == "underflow":
                assert c["r_denormal"] >= 1 and c["r_zero"] >= 1 and c["r_ld_positive_there"], (family, c)
                assert c["q_zero"] == 0
            elif regime == "strong":
                assert c["q_zero"] == 0 and c["r_denormal"] == 0 and c["r_zero"] == 0, (family, c)
            elif regime == "weak":
                assert c["q_zero"] == 0 and c["q_few"] == 0, (family, c)
    assert union_more >= 1 or all(p[1] >= 56 for p in tr.FAMILY[family].panels), family


@pytest.mark.parametrize("family,reg", JOBS)
def test_some_column_follows_a_variant_that_is_not_kept(family, reg):
    """a call site that took the variant before for the column before would show only there"""
    n = sum(tr.predecessor_census(b, ref.kept) for b, ref in zip(tr.family_job(family, "strong", reg)[2], tr.oracle_chains(family, "strong", reg)))
    assert n >= 1, family


def test_objects_of_more_than_32_alleles_are_kept_columns_of_a_split_chain():
    """k_index_cols proper (one wave per object) takes the objects of more than PG_IX_THREAD_AMAX alleles alone: the family made
    for it holds some, one of them behind a variant that is not kept, all with at most five alleles on the paths (narrow columns)."""
    name = "split path, cohort, objects of more than 32 alleles"
    for b, ref in zip(tr.family_job(name, "strong", 0.01)[2], tr.oracle_chains(name, "strong", 0.01)):
        A = np.diff(b.allele_off.astype(np.int64))
        big = (A > tr.IX_THREAD_AMAX) & (ref.kept > 0)
        assert big.sum() >= 5 and tr.predecessor_census(b, ref.kept, tr.IX_THREAD_AMAX) >= 1
        present = np.add.reduceat(ref.allele_present.astype(np.int64), b.allele_off[:-1].astype(np.int64))
        assert present[big].max() <= 5
    for f in tr.FAMILIES:   # (and no other family does: what the issue's table left out)
        if f.name != name:
            assert all(int(np.diff(b.allele_off.astype(np.int64)).max()) <= tr.IX_THREAD_AMAX for b in tr.family_job(f.name, "strong", 0.01)[0]), f.name


def test_quantised_more_than_16_quanta_somewhere_at_64_and_more_paths():
    """(the chains of 64 and more paths together: across variants that are not kept)"""
    n = 0
    for f in tr.FAMILIES:
        for b, ref in zip(tr.family_job(f.name, "quantised", 0.01)[2], tr.oracle_chains(f.name, "quantised", 0.01)):
            if b.n_paths >= 56:
                n += tr.regime_census(b, ref.kept, "quantised")["q_more"]
    assert n >= 1


def test_uniform_kappa_is_the_square_of_the_path_count(orc):
    """uniform: every transition is 1 (c0 = c1 = 0, c2 = 1 on the device), a column's row-pair sum kappa = c0 + 2 H c1 + H^2 c2 is H^2:
    4096 at 64 paths, nothing like the kappa = 1 the lean steps have run with."""
    recomb, uniform, N = tr.regime_params("uniform")
    assert uniform
    for H in sorted({p[1] for f in tr.FAMILIES for p in f.panels}):
        t = orc.transition_probs(10000, 10050, recomb, H, uniform, N)
        assert list(t) == [1, 1, 1]
        kappa = t[0] + 2 * (H - 1) * t[1] + (H - 1) ** 2 * t[2]   # (a state pair's H^2 predecessors: itself, 2 (H - 1) one switch away, (H - 1)^2 two)
        assert kappa == H * H
    for name, recomb, uniform, N, _ in tr.REGIMES:
        if not uniform:   # (the others: a proper distribution, kappa = 1)
            t = orc.transition_probs(10000, 10650, recomb, 64, uniform, N)
            assert abs(float(t[0] + 2 * 63 * t[1] + 63 * 63 * t[2]) - 1.0) < 1e-15, name


# ---- the documented fp64 range ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,reg", JOBS)
def test_deepest_bin_within_the_documented_range(family, reg):
    """A condition on the panels, not a tolerance: a panel that misses it gets another seed."""
    for regime, *_ in tr.REGIMES:
        for b, ref in zip(tr.family_job(family, regime, reg)[2], tr.oracle_chains(family, regime, reg)):
            go = b.geno_off.astype(np.int64)
            lik = np.concatenate([ref.lik, np.zeros(1, LD)])
            mx = np.repeat(np.maximum.reduceat(lik, go[:-1])[:b.n_variants], np.diff(go))
            nz = ref.lik > 0
            assert nz.any()
            assert (ref.lik[nz] >= mx[nz] * LD(10) ** -300).all(), (family, regime, reg, float(np.log10((ref.lik[nz] / mx[nz]).min())))


# ---- the grid of the transition entry point ---------------------------------------------------------------------------------------
def test_grid_is_the_issues_and_its_tie_exclusion_stays_small():
    g = tr.grid()
    assert len(g) == 5 * 5 * 9 and len(set(g)) == len(g)
    assert tr.grid_gaps(64) == (1, 2, 7, 43, 44, 50, 1249, 363175, 406350)
    ties = [p for p in g if tr.is_tie(*p[1:])]
    assert len(ties) <= tr.TIE_SHARE_MAX * len(g), ties
    # (what the window is about: at recombrate 1e-9 and 64 paths, x * 2^64 = 0.0115 * gap: 43 bp -> 0.4958, 44 bp -> 0.5073)
    assert tr.is_tie(1e-9, False, 1e-5, 64, 43) and tr.is_tie(1e-9, False, 1e-5, 64, 44) and not tr.is_tie(1e-9, False, 1e-5, 64, 50)


def test_oracle_transitions_equal_the_references_own_translation_unit(orc):
    """three long doubles, bit for bit, on the whole grid, ties included"""
    if orc.ref_transition_probs(1, 2, 1.26, 5, False, 25000.0) is None:
        pytest.skip("oracle/_ref/libref_transitions.so not built with ref_transition_probs (`make -C oracle ref`, where the reference's sources lie)")
    for name, recomb, uniform, N, H, gap in tr.grid():
        for frm in (tr.GRID_FROM, tr.GRID_FROM + (1 << 33)):
            got = orc.transition_probs(frm, frm + gap, recomb, H, uniform, N)
            want = orc.ref_transition_probs(frm, frm + gap, recomb, H, uniform, N)
            assert got.tobytes() == want.tobytes(), (name, H, gap, got, want)
