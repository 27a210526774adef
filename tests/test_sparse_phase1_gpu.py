"""Sparse phase 1 of the lean chains of chunked jobs (DevContig::sparse): the chain stores every 64th column counted from the
phase boundary, k_refill_lean re-runs the 63 columns between two stored ones on the idle compute units, chunk by chunk in front of
k_post.  A refilled column comes from the same instructions as a stored one, so the results carry the same bits as with
PG_KERNELS=nosparse (every column by the chain) — and match the oracle at the bar of every parity test.

Kept columns per chain are set exactly (the kept variants behind — or in front of — the wanted ones lose their alternative
alleles): with mid = C / 2 the forward half has mid columns, the backward half C - mid.
"""
import numpy as np
import pytest

from pangenie_amd import hmm
from pangenie_amd.panel import default_table_args, synthetic_panel
from tests.parity_util import assert_parity

pytestmark = pytest.mark.gpu

S = 64
PARAMS = (1.26, False, 1e-5)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _oracle(orc, b, args):
    return orc.genotype_contig(b, orc.OracleTable(*args), orc.make_params(*PARAMS))


def _with_columns(orc, b, args, n_cols, front=0, kept=None):
    """b with `front` kept variants dropped at its start and exactly n_cols kept ones after them (kept: the panel's, if known)"""
    if kept is None:
        kept = np.flatnonzero(_oracle(orc, b, args).kept)
    assert kept.size >= front + n_cols, (kept.size, front, n_cols)
    pa = b.path_allele.reshape(b.n_variants, b.n_paths)
    pa[kept[:front], :] = 0                # (every selected path on the reference allele: not a column)
    pa[kept[front + n_cols:], :] = 0
    b._c = None
    return b


def _run(batches, args, sparse):
    job = hmm.Job(batches, hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS))
    plan = job.plan()
    assert ("k_refill_lean" in plan and "sparse" in plan) == sparse, plan
    job.run()
    first = job.fetch_all()
    job.run()   # (a resident job: the second run refills the same arena)
    again = job.fetch_all()
    job.close()
    for r, r2 in zip(first, again):
        assert np.array_equal(r.lik, r2.lik) and np.array_equal(r.lik_exp, r2.lik_exp)
    return first


def _same_bits(a, b):
    assert a.n_columns == b.n_columns
    assert np.array_equal(a.kept, b.kept)
    assert np.array_equal(a.lik_exp, b.lik_exp)
    assert np.array_equal(a.lik, b.lik), f"{int((a.lik != b.lik).sum())} of {a.lik.size} bins differ"


# columns per chain: one, two, three columns; halves below S (no checkpoint but the boundary one); of exactly S, S + 1 and
# 2 S - 1 columns in either half (odd C: the backward half is the longer one); 5 S + 17 per half — several chunks, a ragged
# leading piece —, and a chain of 3 S + 1 per half that ends chunks earlier than the longest (late refill launches and
# late k_post launches find chains without columns)
COLUMNS = (1, 2, 3, 80, 2 * S - 1, 2 * S, 2 * S + 1, 2 * S + 2, 2 * S + 3, 4 * S - 3, 4 * S - 2, 4 * S - 1, 6 * S + 2, 10 * S + 34, 10 * S + 35)


@pytest.fixture(scope="module")
def panels(orc):
    """the chains of COLUMNS and their oracle results, made once for both chunk sizes"""
    args = default_table_args()
    batches = [_with_columns(orc, synthetic_panel(n + 30, 64, 20, seed=500 + i), args, n) for i, n in enumerate(COLUMNS)]
    return batches, [_oracle(orc, b, args) for b in batches]


@pytest.mark.parametrize("K", [64, 128])
def test_sparse_phase1_same_bits_as_dense_and_oracle(K, panels, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    args = default_table_args()
    batches, refs = panels
    monkeypatch.delenv("PG_KERNELS", raising=False)
    sparse = _run(batches, args, True)
    monkeypatch.setenv("PG_KERNELS", "nosparse")
    dense = _run(batches, args, False)
    for n, b, r, d, ref in zip(COLUMNS, batches, sparse, dense, refs):
        assert r.n_columns == n
        _same_bits(r, d)
        assert_parity(b, r, ref)


def test_three_chains_of_unequal_length(orc, monkeypatch):
    """The short chains run out of columns chunks before the long one: its late refill launches walk chains without segments."""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    args = default_table_args()
    batches = [synthetic_panel(v, 64, 20, seed=700 + i) for i, v in enumerate((1400, 150, 517))]
    monkeypatch.delenv("PG_KERNELS", raising=False)
    sparse = _run(batches, args, True)
    monkeypatch.setenv("PG_KERNELS", "nosparse")
    dense = _run(batches, args, False)
    for b, r, d in zip(batches, sparse, dense):
        _same_bits(r, d)
        assert_parity(b, r, _oracle(orc, b, args))


@pytest.mark.parametrize("role", ["forward", "backward"])
def test_fallback_columns_on_and_around_checkpoints(role, orc, monkeypatch):
    """The unregularised table: forward columns that fall back to uniform, backward columns that are all zero.  Where they lie
    hangs on the panel; where the checkpoints lie on mid alone.  64 chains over ONE panel whose mid takes 64 consecutive values put
    every such column of the half on a checkpoint in one chain, directly behind one in another, last of its segment in a third:
    forward columns depend on the columns in front of them only, so kept variants are dropped at the END (mid = 70 .. 133);
    backward columns on those behind them, so they are dropped at the FRONT (two per chain: the column's distance to mid moves by
    one).  Every chain carries the bits of the dense run; four of them are compared with the oracle (the oracle takes a second
    per chain on this table; the dense path's own parity with it is tests/test_parity_gpu.py's).
    (Counts of 6000 where tests/test_parity_gpu.py puts 60000 — the oracle's time grows with the count: a Poisson weight of
    ln p <= 6000 (1 + ln 108 - ln 6000) = -18100 is an exact zero in the reference's long double all the same, ln 2^-16445 = -11399.)"""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    args = (6, 108, 54, 0.0)
    # (the column list hangs on the path alleles alone: taken from the panel before its counts are changed, at the default table)
    kept = np.flatnonzero(_oracle(orc, synthetic_panel(290, 64, 20, seed=6), default_table_args()).kept)
    batches = []
    for d in range(64):
        b = synthetic_panel(290, 64, 20, seed=6)
        b.kmer_count[::3] = 0
        b.kmer_count[1::17] = 6000
        batches.append(_with_columns(orc, b, args, 140 + 2 * d, kept=kept) if role == "forward" else _with_columns(orc, b, args, 268 - 2 * d, front=2 * d, kept=kept))
    monkeypatch.delenv("PG_KERNELS", raising=False)
    sparse = _run(batches, args, True)
    monkeypatch.setenv("PG_KERNELS", "nosparse")
    dense = _run(batches, args, False)
    for i, (b, r, d) in enumerate(zip(batches, sparse, dense)):
        assert r.n_columns == (140 + 2 * i if role == "forward" else 268 - 2 * i)
        _same_bits(r, d)
        if i % 21 == 0:
            assert_parity(b, r, _oracle(orc, b, args))


def test_chunk_size_that_is_no_multiple_of_64_keeps_the_dense_phase1(orc, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "96")
    monkeypatch.delenv("PG_KERNELS", raising=False)
    args = default_table_args()
    b = synthetic_panel(600, 64, 20, seed=41)
    (r,) = _run([b], args, False)
    assert_parity(b, r, _oracle(orc, b, args))
    # ... and so do chains that are not lean chains, beside lean ones that take it
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    mixed = [synthetic_panel(400, 64, 20, seed=1), synthetic_panel(400, 16, 20, seed=2)]
    job = hmm.Job(mixed, hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS))
    plan = job.plan()
    job.run()
    got = job.fetch_all()
    job.close()
    lines = [ln for ln in plan.splitlines() if "phase 1" in ln]
    assert len(lines) == 2 and sum("k_refill_lean" in ln for ln in lines) == 1, plan
    for bb, rr in zip(mixed, got):
        assert_parity(bb, rr, _oracle(orc, bb, args))
