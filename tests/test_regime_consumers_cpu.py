"""The cases of tests/regime_consumers.py held to what they are for, from the CPU oracle and the long-double yardstick on the
oracle's bins alone (no device): a later change to synthetic_panel, to random_plan or to the helpers must not quietly empty
tests/test_regime_consumers_gpu.py.

  - every regularisation-0 case holds at least 5 kept variants whose bins are all zero — the variants before regime_consumers'
    zero_targets, on every chain — and at least 5 kept variants with a call; and one variant a chain (deep_target) whose largest
    bin lies between the long double's denormals and the 2^-16300 below which the device leaves a variant to the host;
  - `strong` and `underflow`, over all families: at least 30 called variants with GQ <= 30 and at least 30 with GQ 10000 or above 100;
  - tie_job: per chain at least 10 ./. from a non-unique maximum — every constructed tie within the reference's 1e-10 window, the
    first kept column, the last, and the one whose first record is a multiple of 256 among them — and balanced variants called 0/1
    with GL(0/0) == GL(1/1);
  - the 40-allele family: at least 3 records of more values than pgk_rtext_wide_values() (read from the library);
  - every case: at most 1 % of the records are left out of the end-to-end comparison (regime_consumers.unstable on the oracle's
    bins).  Measured: 0 in most cases, 0.25 % (tie_job: its own ties) at most.  The per-variant share is printed beside it: the
    regularisation-0 cohort under `weak` and `quantised` holds 21 such variants of 1200 (exact ties of columns that fell back to
    uniform), 5 records of 2361.
"""
import ctypes

import numpy as np
import pytest

from pangenie_amd import _lib, calls
from tests import regime_consumers as rc
from tests import transition_regimes as tr

LD = np.longdouble
CASES = rc.cases()


def test_the_cases_are_the_table():
    assert len(rc.FAMILIES) == 6 and all(f in tr.FAMILY for f in rc.FAMILIES)
    assert len(CASES) == 5 * (2 + 1 + 1 + 1 + 2 + 1) + 1 and CASES[-1][0] == rc.TIE
    assert [f for f in rc.FAMILIES if 0.0 in tr.FAMILY[f].regs] == ["lean, sparse, in pieces", "split path, cohort"]
    assert [len(tr.FAMILY[f].cohort_seeds) * len(tr.FAMILY[f].panels) for f in rc.FAMILIES] == [0, 0, 0, 0, 6, 2]
    for c in CASES:
        for plan in rc.combine_plans(c):
            flat = [x for g in plan for x in g]
            assert len(set(flat)) == len(flat) and max(flat) < len(rc.job_of(c)[2])
    assert max(len(g) for g in rc.combine_plans(CASES[-1])[0]) >= 3 and min(len(g) for g in rc.combine_plans(CASES[-1])[0]) == 1
    assert sorted(len(g) for g in rc.combine_plans(("split path, cohort", "strong", 0.01))[0]) == [1, 2, 3]


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == 0.0], ids=rc.case_id)
def test_regularisation_0_cases_hold_all_zero_variants_beside_called_ones(case):
    index, samples, chains = rc.job_of(case)
    for c, (b, ref, a) in enumerate(zip(chains, rc.oracle_of(case), rc.oracle_answers(case))):
        kept = np.asarray(ref.kept, bool)
        zero = np.flatnonzero(a.all_zero)
        assert kept[zero].all() and all(a.calls[v] is None for v in zero) and not a.not_unique[zero].any()
        before = [t - 1 for t in rc.zero_targets(index[rc.index_of_chain(case, c)])]
        assert set(before) <= set(zero.tolist()), (c, before, zero)   # on every chain, where they were put: column 0, 63 and 64, two in a row
        assert len(zero) >= 5 and sum(x is not None for x in a.calls) >= 5
        go = b.geno_off.astype(np.int64)
        assert all(not (ref.lik[go[v]:go[v + 1]] != 0).any() for v in zero)
        # the variant meant for the host: its largest bin a normal long double below the device's 2^-16300, and called all the same
        d = rc.deep_target(index[rc.index_of_chain(case, c)])
        top = ref.lik[go[d]:go[d + 1]].max()
        assert np.ldexp(LD(1), -16382) < top < np.ldexp(LD(1), -16300) and kept[d] and a.calls[d] is not None, (c, d, top)


def test_strong_and_underflow_hold_flat_and_certain_posteriors():
    low = high = 0
    for case in CASES:
        if case[1] in ("strong", "underflow"):
            h = rc.census(case)["gq"]
            low, high = low + h[0], high + h[2] + h[3]
    assert low >= 30 and high >= 30, (low, high)


def test_tie_job_ties_where_it_is_meant_to():
    case = CASES[-1]
    _, _, chains, plans, ties, balanced = rc.tie_job()
    assert [b.n_paths for b in chains] == list(rc.TIE_PATHS) and all(b.n_variants == rc.TIE_V >= 40 for b in chains)
    for c, (b, ref, a) in enumerate(zip(chains, rc.oracle_of(case), rc.oracle_answers(case))):
        kept = np.flatnonzero(np.asarray(ref.kept, bool))
        go, H = b.geno_off.astype(np.int64), LD(b.n_paths)
        assert len(ties[c]) == rc.N_TIES >= 10 and int(a.not_unique.sum()) >= 10
        assert ties[c][0] == int(kept[0]) == 1 and ties[c][-1] == int(kept[-1]) == rc.TIE_V - 1   # the first kept column, and the last
        assert any(int(plans[c].rec_off[v]) % 256 == 0 and int(plans[c].rec_off[v]) > 0 for v in ties[c])
        for v in ties[c]:
            x = ref.lik[go[v]:go[v + 1]] / ref.lik[go[v]:go[v + 1]].sum()
            assert a.not_unique[v] and a.calls[v] is None and a.unstable[v], (c, v, x)
            assert abs(x[0] - x[1]) < rc.TIE_WINDOW and abs(x[0] - LD(4) / 9) < 1e-15 and abs(x[2] - LD(1) / 9) < 1e-15, (c, v, x)   # (64, 64, 16)
            recs = range(int(plans[c].rec_off[v]), int(plans[c].rec_off[v + 1]))
            assert all(a.rec_calls[r] is None or plans[c].record(r)[0][1] == 0 or 0xFFFF in plans[c].record(r)[1] for r in recs)
        # (random_plan keeps both alleles apart and defined in about a fifth of a two-allele bubble's records: those tie as records too)
        assert sum(a.rec_calls[r] is None for v in ties[c] for r in range(int(plans[c].rec_off[v]), int(plans[c].rec_off[v + 1]))) >= 1
        for v in balanced[c]:
            x = ref.lik[go[v]:go[v + 1]]
            assert a.calls[v] == (0, 1, 3) and abs(x[0] - x[2]) <= 1e-18 * x[1] and not a.unstable[v], (c, v, x)
        ordinary = [v for v in kept if v not in ties[c] and v not in balanced[c]]
        assert sum(a.calls[v] is not None for v in ordinary) > 1000


def test_the_40_allele_family_holds_records_beyond_the_text_kernels_narrow_bound():
    f = _lib.load_hip().pgk_rtext_wide_values
    f.restype = ctypes.c_uint32
    wide_above = int(f())
    (plan,) = rc.plans_of(rc.WIDE_FAMILY)
    values = np.diff(calls.record_gl_offsets(plan).astype(np.int64))
    assert wide_above > 21 and int((values > wide_above).sum()) >= 3, (wide_above, np.sort(values)[-5:])
    assert int(values.max()) == 40 * 41 // 2


@pytest.mark.parametrize("case", CASES, ids=rc.case_id)
def test_at_most_one_percent_is_left_out_of_the_end_to_end_comparison(case):
    cen = rc.census(case)
    print(rc.case_id(case), cen)
    assert cen["records"] > 300 and cen["called"] > 100
    assert cen["records_left_out"] <= rc.LEFT_OUT_MAX * cen["records"], cen
