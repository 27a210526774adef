"""The per-column scalars of sparse lean chains (pg_kernels.hip: lean_forward / lean_backward): fscale[c] / bscale[c] is written by
whoever writes column c — the chain at the columns it stores (its store-free step parks no scalar), a refill segment
(k_refill_lean) at the columns it forms; bsum by the chain alone, at the columns it stores.  Every bin k_post forms contains
1 / (fscale bscale) of its column, so an entry that nobody wrote, that was written for the wrong column or that is left over from an
earlier run shows in the bins: they must carry the bits of PG_KERNELS=nosparse2 and PG_KERNELS=nosparse, whose chains write every
scalar themselves, and match the oracle at the bar of every parity test.

Shapes: the smallest at which a segment's scalar writes can go wrong — chains of one to three columns (no segment; a one-column
chain), halves just below, on and just above a checkpoint, a ragged last piece; 64 chains over one panel with mid at 64 consecutive
values, so that segments start at every residue of the 64-entry scalar blocks they are flushed in; fall-back columns on a checkpoint
(the chain's entry) and inside a segment (the segment's); and a resident job run twice on different counts.
"""
import numpy as np
import pytest

from pangenie_amd import hmm
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts
from tests.parity_util import assert_parity
from tests.test_sparse_phase2_gpu import (PARAMS, S, _fallback_chains, _forward_column_fell_back, _n_columns, _oracle, _same_bits,
                                          _three_ways, _with_columns)

pytestmark = pytest.mark.gpu

COLUMNS = (1, 2, 3, 2 * S - 1, 2 * S, 2 * S + 1, 4 * S - 2, 10 * S + 35)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def panels(orc):
    """the chains of COLUMNS and their oracle results, made once for both chunk sizes"""
    args = default_table_args()
    batches = [_with_columns(orc, synthetic_panel(n + 30, 64, 20, seed=900 + i), args, n) for i, n in enumerate(COLUMNS)]
    return batches, [_oracle(orc, b, args) for b in batches]


@pytest.mark.parametrize("K", [64, 128])
def test_chains_around_the_checkpoints(K, panels, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    batches, refs = panels
    got = _three_ways(batches, default_table_args(), monkeypatch)
    for n, b, r, ref in zip(COLUMNS, batches, got, refs):
        assert r.n_columns == n
        assert_parity(b, r, ref)


N_LONG = 387   # columns of the longest of the 64 chains below


@pytest.fixture(scope="module")
def mid_chains(orc):
    """64 chains over ONE panel, C = 260 + 2 d + (d & 1): mid = 130 + d takes 64 consecutive values (C even and odd by turns), so the
    segments of either role and phase start and end at every residue of the 64-entry blocks the scalars are flushed in.  Two
    checkpoints in either half of phase 2; kept variants are dropped at the end."""
    args = default_table_args()
    kept = np.flatnonzero(_oracle(orc, synthetic_panel(430, 64, 20, seed=6), args).kept)
    assert kept.size >= N_LONG
    batches = [_with_columns(orc, synthetic_panel(430, 64, 20, seed=6), args, 260 + 2 * d + (d & 1), kept=kept) for d in range(64)]
    return args, batches, {d: _oracle(orc, batches[d], args) for d in (0, 63)}


@pytest.mark.parametrize("K", [64, 128])
def test_segments_at_every_residue_of_the_scalar_blocks(K, mid_chains, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    args, batches, refs = mid_chains
    got = _three_ways(batches, args, monkeypatch)
    for d, (b, r) in enumerate(zip(batches, got)):
        assert r.n_columns == 260 + 2 * d + (d & 1) and r.n_columns // 2 == 130 + d
        if d in refs:
            assert_parity(b, r, refs[d])


def test_second_run_on_other_counts_takes_no_scalar_of_the_first(orc, monkeypatch):
    """A resident job keeps fscale / bscale / bsum between runs.  Its second run, on another sample's counts, must write every
    entry it reads: the bits of a fresh job on those counts.  (An entry left from the first run belongs to other counts and
    shows in every bin of its column.)  Two chains: both halves with a leading piece, whole segments and a ragged last one."""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "128")
    monkeypatch.delenv("PG_KERNELS", raising=False)
    args = default_table_args()
    batches = [synthetic_panel(700, 64, 20, seed=31), synthetic_panel(300, 64, 20, seed=32)]
    table, params = hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS)
    job = hmm.Job(batches, table, params)
    assert "k_refill_lean (both halves)" in job.plan()
    job.run()
    first = job.fetch_all()
    for i, b in enumerate(batches):   # (in place: the job re-uploads from the arrays it was made with)
        kc, cov = synthetic_sample_counts(b, seed=77 + i)
        b.kmer_count[:] = kc
        b.coverage[:] = cov
    job.upload_run()
    second = job.fetch_all()
    job.close()
    fresh_job = hmm.Job(batches, table, params)
    fresh_job.run()
    fresh = fresh_job.fetch_all()
    fresh_job.close()
    for b, a, r, f in zip(batches, first, second, fresh):
        assert not np.array_equal(a.lik, r.lik)   # (the counts did change the posteriors)
        _same_bits(r, f)
        assert_parity(b, r, _oracle(orc, b, args))


# ---- fall-back columns ------------------------------------------------------------------------------------------------------
FALLBACK_CHAINS = (0, 1, 31, 63)   # of the 64 chains of tests/test_sparse_phase2_gpu.py's construction (mid = 130 + d)


@pytest.fixture(scope="module")
def fallback_sets(orc):
    out = {}
    for role in ("forward", "backward"):
        args, batches = _fallback_chains(orc, role)
        batches = [batches[d] for d in FALLBACK_CHAINS]
        out[role] = (args, batches, _oracle(orc, batches[0], args))
    return out


@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("role", ["forward", "backward"])
def test_fallback_columns_on_a_checkpoint_and_inside_a_segment(role, K, fallback_sets, orc, monkeypatch):
    """The unregularised table: forward columns that fall back to uniform (k_post takes 1 for their fscale, and the column
    behind one is scaled from the uniform column's sum), backward columns that are all zero (bsum = 0 at the column, the next
    one scaled from 1).  The scale of a flagged checkpoint is the chain's entry, that of a flagged column inside a segment the
    segment's: both occur in chain 0 (C = 260, mid = 130) — the oracle's output says so for the forward role."""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    args, batches, ref0 = fallback_sets[role]
    if role == "forward" and K == 64:
        kept = np.flatnonzero(_oracle(orc, synthetic_panel(430, 64, 20, seed=6), default_table_args()).kept)
        mid = _n_columns(role, 0) // 2
        for c in (mid - 1 - S, mid - 1 + S, mid - 1 - S + 7, mid - 1 + S + 7):   # checkpoints of phase 1 and 2; inside their segments
            assert _forward_column_fell_back(orc, args, kept, c), c
    got = _three_ways(batches, args, monkeypatch)
    for d, r in zip(FALLBACK_CHAINS, got):
        assert r.n_columns == _n_columns(role, d)
    assert_parity(batches[0], got[0], ref0)
