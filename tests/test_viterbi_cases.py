"""The constructed Viterbi cases of tests/viterbi_cases.py, on the CPU: the restatement that names the kernel condition a
case reaches gives the oracle's haplotypes, and the condition the case is named after occurs — in its state path, its
column values or its allele counts.  A case that loses its reach (a changed helper, another seed) fails here, not
silently on the device (tests/test_viterbi_edges_gpu.py runs the same cases through pg_viterbi.hip)."""
import numpy as np
import pytest

from tests import viterbi_cases as vc

CASES = vc.all_cases()


@pytest.fixture(scope="module")
def restated():
    memo = {}

    def get(case, regime):
        if (case.name, regime) not in memo:
            memo[case.name, regime] = vc.restate(case.batch, vc.oracle_table(case.table), regime)
        return memo[case.name, regime]
    return get


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_restatement_is_the_oracle(case, restated):
    """form 1 (four candidates) always, form 0 (the reference's O(H^4) scan) up to 16 paths"""
    for regime in case.regimes:
        r = restated(case, regime)
        for form in (1, 0) if case.H <= 16 else (1,):
            o = vc.oracle_result(case.name, regime, form)
            assert o.n_columns == r.cols.size and np.array_equal(np.flatnonzero(o.kept), r.cols), (regime, form)
            assert np.array_equal(o.hap1, r.hap1) and np.array_equal(o.hap2, r.hap2), (regime, form)


def test_every_family_is_there():
    names = [c.name for c in CASES]
    for H in (7, 16, 20, 32, 40, 64):
        for C in (1, 2, 31, 32, 33, 63, 64, 65, 97):
            assert "a_H%d_C%d" % (H, C) in names
    assert {c.H for c in CASES if c.name.startswith("b_")} == {6, 30, 64}
    assert {c.H for c in CASES if c.name.startswith("c_")} == {9, 16, 24, 32, 40, 64}
    assert {c.H for c in CASES if c.name.startswith("d_")} == {12, 16, 24, 48, 64}
    assert {c.H for c in CASES if c.name.startswith("f_")} == {1, 2, 15, 17, 31, 33, 48, 63}
    for c in CASES:
        if c.name.startswith("f_"):
            assert c.regimes == vc.FIVE
        if c.name.startswith("c_"):
            assert vc.NO_RECOMB in c.regimes and vc.FIXTURE in c.regimes
    for fam in "abcde":  # every family at every kernel width
        assert {vc.kernel_k(c.H) for c in CASES if c.name.startswith(fam + "_")} == {1, 2, 4}, fam


@pytest.mark.parametrize("case", [c for c in CASES if "C" in c.want], ids=lambda c: c.name)
def test_kept_column_count(case, restated):
    """the staging guards (cn < C, (blk + 1) BC < C, C > BC) are decided by the number of kept columns alone"""
    assert restated(case, case.regimes[0]).cols.size == case.want["C"]
    assert case.batch.n_variants - 1 == restated(case, case.regimes[0]).cols[-1]  # the chain ends on a kept variant


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith("b_")], ids=lambda c: c.name)
def test_backtrace_edges(case, restated):
    """k_vit_backtrack sees 64 columns per ballot: lane k holds column c - k of the walk's current column c.  A run of 64
    from c ends in lane 63 (r == 63), one of 65 or more takes the r == 64 continue path and, at 65, shows the change to
    lane 0 of the next ballot; a run of one column at the end is r == 0 at once, one at the start ends the walk on
    cr == 1, c == 0"""
    r = restated(case, case.regimes[0])
    runs = vc.runs_from_end(r.states)
    if "runs" in case.want:
        assert runs == case.want["runs"]
    else:
        assert len(runs) - 1 >= case.want["changes_at_least"]
    assert len(case.batch.kmer_off) - 1 == r.cols.size   # every variant is a column


def test_backtrace_edges_between_them():
    want = [tuple(c.want.get("runs", ())) for c in CASES if c.name.startswith("b_H64")]
    assert (129,) in want                                      # no change, C - 1 = 128, a last run of >= 129
    assert any(w[:1] == (64,) for w in want) and any(w[:1] == (65,) for w in want)   # runs of 64 / 65 that end on the last column
    mid = next(w for w in want if len(w) == 5)
    assert mid[0] == 1 and mid[-1] == 1 and mid[1] == 64 and mid[2] == 65   # changes at both ends; 63 and 64 below the walk's column


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith("c_")], ids=lambda c: c.name)
def test_exact_zeros(case, restated):
    n = case.H ** 2
    for regime in case.regimes:
        r = restated(case, regime)
        assert np.flatnonzero(r.zero_col).tolist() == case.want["zero"][regime], regime
    r = restated(case, vc.NO_RECOMB)
    zero = case.want["zero"][vc.NO_RECOMB]
    assert any(0 < z < r.cols.size - 1 for z in zero)                  # in the middle of the chain
    assert any(z in (vc.BC - 1, vc.BC) for z in zero)                  # right before / at the staged-block boundary
    assert ((r.zero_states > 0) & (r.zero_states < n)).sum() > 10      # only some states with all four products 0
    assert all(r.zero_states[z + 1] == 0 for z in zero if z + 1 < r.cols.size)  # the step after it sees a constant column
    # q == 0 by the table's regime too: no product but the state's own is > 0 there
    assert r.zero_states[1] > 0 and restated(case, vc.FIXTURE).zero_states[1] == 0


def test_exact_zeros_between_them():
    for H in (9, 16, 24, 32, 40, 64):
        zs = [(c.want["C"], c.want["zero"]) for c in CASES if c.name.startswith("c_H%d_" % H)]
        for regime in (vc.NO_RECOMB, vc.FIXTURE):
            assert any(C - 1 in z[regime] for C, z in zs), (H, regime)       # a zero last column (the c == C exit)
            assert any(C - 1 not in z[regime] for C, z in zs), (H, regime)   # ... and a live stretch after the last zero column
            assert any(vc.BC - 1 in z[regime] for C, z in zs), (H, regime)
        assert any(vc.BC in z[vc.NO_RECOMB] for C, z in zs), H


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith("d_")], ids=lambda c: c.name)
def test_wide_columns(case, restated):
    r = restated(case, case.regimes[0])
    wide = [c for c, v in enumerate(r.cols) if vc.alleles_on_paths(case.batch, int(v)) > vc.PG_AMAX]
    assert set(case.want["wide"]) <= set(wide)
    C = r.cols.size
    assert {0, 1, vc.BC - 1, vc.BC, vc.BC + 1, C - 1} <= set(wide)     # first, second, around the staged block, last
    assert len(wide) < C // 2                                         # most columns take the table in the record


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith("e_")], ids=lambda c: c.name)
def test_ties(case, restated):
    H, want = case.H, case.want
    V = case.batch.n_variants
    pa = case.batch.path_allele.reshape(V, H)
    r = restated(case, case.regimes[0])
    if "dup" in want:
        twins = sum(int(np.array_equal(pa[:, p], pa[:, q])) for p in range(H) for q in range(p))
        assert twins >= H // 2
        if "inlane" in case.name:
            assert all(np.array_equal(pa[:, 4 * j], pa[:, 4 * j + k]) for j in range(H // 4) for k in range(4))
        if "plus16" in case.name:
            assert all(np.array_equal(pa[:, p], pa[:, p + 16]) for p in list(range(16)) + list(range(32, 48)))
        # the best state has twins of the same value: the path sits on the LAST of them
        i, j = r.states[-1] // H, r.states[-1] % H
        assert not any(np.array_equal(pa[:, p], pa[:, i]) for p in range(i + 1, H))
    if "last_state" in want:
        assert (pa == pa[:, :1]).all() and (r.states == H * H - 1).all()
    if "diagonal" in want:
        assert (r.states // H == r.states % H).all() and r.states[0] != H * H - 1
    if "gap0" in want:
        pos = case.batch.variant_pos[r.cols]
        assert all(pos[c] == pos[c - 1] for c in want["gap0"]) and (np.diff(pos.astype(np.int64)) >= 0).all()
        assert int((np.diff(pos.astype(np.int64)) == 0).sum()) == len(want["gap0"])
    if "near_tie" in want:
        # some rows' maxima are below the column's maximum by less than 2^-56 of it: equal high doubles, different low ones
        assert (r.near_rows > 0).sum() >= 5
