"""Every sweep family under transition regimes and position gaps it has never seen (tests/transition_regimes.py: REGIMES, FAMILIES):
uniform transitions (c0 = c1 = 0, c2 = 1, kappa = H^2), strong mixing at effective_N = 25000 (the default of make_params, of the
reference's HMM and of the drop-in adapter), q == 0 columns next to columns of a few 2^-64 quanta, and gaps at which r = exp(-x) is
an fp64 denormal (c0 = 0, c1 denormal) or 0 while the oracle's long double underflows at none of them.  The four call sites of
transition_consts (both branches of records_unit, k_index_cols, k_index_cols_t) and every step formulation that folds 2^-es into the
constants or predicts a column's scale through kappa are reached by one small job each.

Every case runs the device under the family's environment, checks on the job's plan that the kernels it is meant to reach are the
ones planned, runs twice (the same bits) and compares every chain with the CPU oracle under the same parameters (assert_parity: 1e-6
relative on EVERY bin, identical calls, kept, allele_present, n_kmers, coverage); tests/test_transition_regimes_cpu.py holds the
panels to the documented fp64 range that makes the unconditional comparison fair.  Two device paths side by side agree within
1e-10 (the bound of tests/test_structured_objects_gpu.py: _agree); positions shifted by 2^33 give the same bits; the transition
entry point meets the oracle on a grid of gaps, path counts and regimes.  The worst error of every case goes through log_parity
(profiles/r27_transition_regimes.txt is one run's output).

Kernel names: kPrepName and the sweep and bins tables of pangenie_amd/csrc/pg_shim.cpp.  Every name of the families' table is what
the planner prints for its shape: none had to be corrected, and no kernel is forced.  Where a name is part of another, the longer
text is asserted: "lean, dense" wants "phase 1 = k_sweep_lean<1>;" (no word of sparse) and k_refill_lean nowhere in the plan, not
only not in phase 1; "128 paths, fused" wants "bins = k_bins" at the end of its line; "lean, sparse, in pieces" wants its three
pieces.  One family beyond the table: k_index_cols proper (one wave per object) takes only the objects of more than 32 alleles,
every other column of a split chain is k_index_cols_t's, and the table's split cohort holds no such object — a wrong predecessor
column at that call site passed all of its cases, and fails "split path, cohort, objects of more than 32 alleles" (as measured
with a build that had such a mistake put in).
Reference: src/transitionprobabilitycomputer.cpp:8-39, src/hmm.cpp:175-405.
"""
import numpy as np
import pytest

from pangenie_amd import hmm
from tests import transition_regimes as tr
from tests.parity_util import assert_parity, log_parity

pytestmark = pytest.mark.gpu

OFFSET = 1 << 33
_ids = lambda c: f"{c[0]}-{c[1]}-reg{c[2]}"


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _agree(got, other, tol=1e-10):
    worst = 0.0
    for a, c in zip(got, other):
        a, c = a.likelihoods_ld(), c.likelihoods_ld()
        den = np.maximum(np.abs(a), np.abs(c))
        worst = max(worst, float(np.where(den > 0, np.abs(a - c) / np.where(den > 0, den, 1), 0).max()) if a.size else 0.0)
    assert worst < tol, worst
    return worst


def _device(monkeypatch, family, regime, reg, kernels, want, unwanted=(), offset=0):
    """One job of the family under its environment and PG_KERNELS = kernels: the plan names every kernel of `want` and none of
    `unwanted`; run twice, the same bits; -> results, one per chain."""
    fam = tr.FAMILY[family]
    for var, val in (("PG_SWEEP_MODE", fam.mode), ("PG_KERNELS", kernels), ("PG_CHUNK_COLS", fam.chunk_cols), ("PG_PIECE_CHUNKS", fam.piece_chunks)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    index, samples, chains = tr.family_job(family, regime, reg)
    if offset:
        index = [tr.offset_panel(b, offset) for b in index]
    table, params = hmm.ProbabilityTable(*tr.TABLE_ARGS, reg), hmm.make_params(*tr.regime_params(regime))
    job = hmm.Job(list(index), table, params) if samples is None else hmm.Job.cohort(list(index), samples, table, params)
    try:
        plan = job.plan()
        assert fam.mode is None or job.sweep_mode()[0] == fam.mode, plan
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
    assert len(got) == len(chains)
    for r, r2 in zip(got, again):
        assert np.array_equal(r.lik, r2.lik) and np.array_equal(r.lik_exp, r2.lik_exp)
        assert np.array_equal(r.kept, r2.kept) and np.array_equal(r.allele_present, r2.allele_present)
    return got


def _parity(family, regime, reg, got, label):
    worst = 0.0
    for b, r, ref in zip(tr.family_job(family, regime, reg)[2], got, tr.oracle_chains(family, regime, reg)):
        worst = max(worst, assert_parity(b, r, ref))
    log_parity(f"transition regimes, {family}, {label}, regime {regime}, regularisation {reg}: worst relative error {worst:.3e}")
    return worst


# ---- every family under every regime ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,regime,reg", tr.cases(), ids=[_ids(c) for c in tr.cases()])
def test_family_under_regime_vs_oracle(family, regime, reg, monkeypatch):
    fam = tr.FAMILY[family]
    got = _device(monkeypatch, family, regime, reg, fam.kernels, fam.want, fam.unwanted)
    _parity(family, regime, reg, got, f"PG_KERNELS={fam.kernels or '(default)'}")


# ---- two device paths side by side --------------------------------------------------------------------------------------------------
BESIDE = [(f.name, r[0], reg) for f in tr.FAMILIES if f.other for r in tr.REGIMES for reg in f.regs]


@pytest.mark.parametrize("family,regime,reg", BESIDE, ids=[_ids(c) for c in BESIDE])
def test_two_device_paths_agree(family, regime, reg, monkeypatch):
    """lean chains in pieces beside PG_KERNELS=general, triangle lean chains beside nolean2,notri, the split path beside small,nosplit:
    both meet the oracle and agree within 1e-10."""
    fam = tr.FAMILY[family]
    kernels, want, unwanted = fam.other
    got = _device(monkeypatch, family, regime, reg, fam.kernels, fam.want, fam.unwanted)
    other = _device(monkeypatch, family, regime, reg, kernels, want, unwanted)
    _parity(family, regime, reg, got, f"PG_KERNELS={fam.kernels or '(default)'} (beside {kernels})")
    _parity(family, regime, reg, other, f"PG_KERNELS={kernels}")
    worst = _agree(got, other)
    log_parity(f"transition regimes, {family}, regime {regime}, regularisation {reg}: the two device paths differ by {worst:.3e} at most")


# ---- positions are 64-bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["strong", "quantised"])
@pytest.mark.parametrize("family", ["lean, dense", "split path, cohort", "generic"])
def test_positions_shifted_by_2_33_give_the_same_bits(family, regime, monkeypatch):
    """Only differences of positions may matter (compact records of k_records, k_index_cols, full records of k_records): device only."""
    fam = tr.FAMILY[family]
    got = _device(monkeypatch, family, regime, 0.01, fam.kernels, fam.want, fam.unwanted)
    far = _device(monkeypatch, family, regime, 0.01, fam.kernels, fam.want, fam.unwanted, offset=OFFSET)
    for r, r2 in zip(got, far):
        assert np.array_equal(r.lik, r2.lik) and np.array_equal(r.lik_exp, r2.lik_exp) and np.array_equal(r.kept, r2.kept)


# ---- the transition entry point ------------------------------------------------------------------------------------------------------
def test_transition_probs_grid_vs_oracle(orc):
    """k_transition_single against the oracle's long double on gaps x path counts x regimes: 1e-9 relative on each of the three values
    wherever p^2 >= 1e-280 (the bar of the emission-table comparisons in tests/test_parity_gpu.py), exactly where the oracle's value is
    0 or 1; below that floor only 0 <= value <= 1e-279 (the reference's long double holds what fp64 cannot).  Ties of rint are left
    out (tests/transition_regimes.py: is_tie; their share is capped by tests/test_transition_regimes_cpu.py)."""
    worst = {name: 0.0 for name, *_ in tr.REGIMES}
    n = 0
    for name, recomb, uniform, N, H, gap in tr.grid():
        if tr.is_tie(recomb, uniform, N, H, gap):
            continue
        n += 1
        got = hmm.transition_probs(tr.GRID_FROM, tr.GRID_FROM + gap, recomb, H, uniform, N)
        want = orc.transition_probs(tr.GRID_FROM, tr.GRID_FROM + gap, recomb, H, uniform, N)
        assert np.all(np.isfinite(got)) and np.all(got >= 0), (name, H, gap, got)
        if float(want[0]) < tr.P2_FLOOR:
            assert np.all(got <= 1e-279), (name, H, gap, got, want)
            continue
        for g, w in zip(got, want):
            if w == 0 or w == 1:
                assert g == float(w), (name, H, gap, got, want)
            else:
                rel = abs(float((np.longdouble(g) - w) / w))
                worst[name] = max(worst[name], rel)
                assert rel < 1e-9, (name, H, gap, got, want, rel)
    assert n >= (1 - tr.TIE_SHARE_MAX) * len(tr.grid())
    for name, w in worst.items():
        log_parity(f"transition regimes, k_transition_single, regime {name}: worst relative error {w:.3e} over the grid")
