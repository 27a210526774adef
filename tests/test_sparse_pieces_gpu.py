"""Phase 1 of sparse lean chains in pieces (pg_job::n_pieces; pg_device.h: pg_sparse_piece): a job whose chains are all sparse lean
chains runs phase 1 as one launch per piece of PG_PIECE_CHUNKS partner chunks, the farthest piece first, and refills the partner
columns of every piece but piece 0 on the second stream beside the pieces that follow.  A piece resumes from the checkpoint the
piece before it stored — from all-zero states where that checkpoint fell back to uniform, as the single launch went on in
registers — and ends with the zero test of its last column: the results carry the bits of PG_KERNELS=nopieces (one launch, every
refill in phase 2) and of PG_KERNELS=nosparse, and match the oracle at the bar of every parity test.

Kept columns per chain are set exactly, as in tests/test_sparse_phase2_gpu.py.  Chunks of 64 and 128 columns with one and two chunks
per piece put a piece boundary on every checkpoint (64 x 1), on every second one (64 x 2, 128 x 1) and on every fourth (128 x 2).
"""
import numpy as np
import pytest

from pangenie_amd import hmm
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts
from tests.parity_util import assert_parity
from tests.test_sparse_phase2_gpu import PARAMS, S, _oracle, _same_bits, _with_columns

pytestmark = pytest.mark.gpu

KG = [(64, 1), (64, 2), (128, 1), (128, 2)]   # (PG_CHUNK_COLS, PG_PIECE_CHUNKS)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _n_pieces(batches, K, G):
    """what pg_job_new makes of the job's longest chain: chunks over half its variants, G of them per piece"""
    half = max(b.n_variants for b in batches) // 2 + 1
    K = min(K, half)
    n_chunks = (half + K - 1) // K
    return (n_chunks + G - 1) // G


def _run(batches, args, n_pieces):
    """n_pieces: what the plan must say (1: a single phase-1 launch, no word of pieces)"""
    job = hmm.Job(batches, hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS))
    plan = job.plan()
    lines = [ln for ln in plan.splitlines() if "k_sweep_lean<1>" in ln]
    assert lines, plan
    for ln in lines:
        assert (f"in {n_pieces} pieces" in ln) == (n_pieces > 1), plan
        assert ("pieces" in ln) == (n_pieces > 1), plan
    job.run()
    first = job.fetch_all()
    job.run()   # (a resident job: the second run's pieces and refills follow the first run's k_post on the two streams)
    again = job.fetch_all()
    job.close()
    for r, r2 in zip(first, again):
        _same_bits(r, r2)
    return first


def _three_ways(batches, args, K, G, monkeypatch, pieces=True):
    """in pieces, PG_KERNELS=nopieces and PG_KERNELS=nosparse: the same bits; returns the results of the run in pieces"""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    monkeypatch.setenv("PG_PIECE_CHUNKS", str(G))
    monkeypatch.delenv("PG_KERNELS", raising=False)
    n_pieces = _n_pieces(batches, K, G) if pieces else 1
    got = _run(batches, args, n_pieces)
    monkeypatch.setenv("PG_KERNELS", "nopieces")
    single = _run(batches, args, 1)
    monkeypatch.setenv("PG_KERNELS", "nosparse")
    dense = _run(batches, args, 1)
    monkeypatch.delenv("PG_KERNELS", raising=False)
    for r, s1, d in zip(got, single, dense):
        _same_bits(r, s1)
        _same_bits(r, d)
    return got, n_pieces


# columns per chain: one, two, three (empty halves, a one-column piece); halves of 63 / 64 (no checkpoint but the boundary one: one
# piece), 64 / 64 and 64 / 65 (a farthest piece of one column, at 64 x 1: the column the recursion starts at is a piece of its own),
# 127 / 127 and 337 / 338: whole pieces and a ragged farthest one, which holds the chain's leading columns
COLUMNS = (1, 2, 3, 127, 128, 129, 254, 675)


@pytest.fixture(scope="module")
def panels(orc):
    """the chains of COLUMNS and their oracle results, made once for every chunk and piece size"""
    args = default_table_args()
    batches = [_with_columns(orc, synthetic_panel(n + 30, 64, 20, seed=1100 + i), args, n) for i, n in enumerate(COLUMNS)]
    return batches, [_oracle(orc, b, args) for b in batches]


@pytest.mark.parametrize("K,G", KG)
def test_pieces_same_bits_as_single_launch_and_oracle(K, G, panels, monkeypatch):
    batches, refs = panels
    got, n_pieces = _three_ways(batches, default_table_args(), K, G, monkeypatch)
    assert n_pieces == {(64, 1): 6, (64, 2): 3, (128, 1): 3, (128, 2): 2}[(K, G)]
    for n, b, r, ref in zip(COLUMNS, batches, got, refs):
        assert r.n_columns == n
        assert_parity(b, r, ref)


@pytest.fixture(scope="module")
def unequal(orc):
    args = default_table_args()
    batches = [synthetic_panel(v, 64, 20, seed=1200 + i) for i, v in enumerate((1400, 150, 517))]
    return batches, [_oracle(orc, b, args) for b in batches]


@pytest.mark.parametrize("K,G", KG)
def test_three_chains_of_unequal_length(K, G, unequal, monkeypatch):
    """The short chains have no columns in the early pieces: those launches and the refills behind them walk chains without columns."""
    batches, refs = unequal
    got, n_pieces = _three_ways(batches, default_table_args(), K, G, monkeypatch)
    assert n_pieces == {(64, 1): 11, (64, 2): 6, (128, 1): 6, (128, 2): 3}[(K, G)]
    for b, r, ref in zip(batches, got, refs):
        assert_parity(b, r, ref)


# ---- fall-back columns ------------------------------------------------------------------------------------------------------
FB_VARIANTS = 700          # the panel of the construction below (its kept variants: the chains' columns)
FB_CHAINS = (0, 1, 31)     # d: a chain of 520 + 2 d columns, mid = 260 + d
FB_DISTS = (S, 2 * S, 4 * S)   # checkpoints of phase 1, in columns from the phase boundary: a piece boundary at every (K, G) of KG is among them


def _fb_panel():
    b = synthetic_panel(FB_VARIANTS, 64, 20, seed=6)
    b.kmer_count[::3] = 0
    b.kmer_count[1::17] = 6000
    return b


def _fb_columns(role, d):
    return 520 + 2 * d if role == "forward" else 520 + 2 * max(FB_CHAINS) - 2 * d


def _forward_column_fell_back(orc, args, kept, c):
    """tests/test_sparse_phase2_gpu.py's witness on this panel: in the chain cut off behind column c the bins of c are its forward
    column added up by genotype — for the uniform column exactly (n0^2, 2 n0 n1, n1^2) / 4096."""
    b = _with_columns(orc, _fb_panel(), args, c + 1, kept=kept)
    ref = _oracle(orc, b, args)
    v = int(np.flatnonzero(ref.kept)[c])
    bins = np.asarray(ref.lik[int(ref.geno_off[v]):int(ref.geno_off[v + 1])], dtype=np.float64)
    n1 = int((b.path_allele.reshape(b.n_variants, b.n_paths)[v] != 0).sum())
    n0 = 64 - n1
    return bins.size == 3 and np.array_equal(bins, np.array([n0 * n0, 2 * n0 * n1, n1 * n1]) / 4096.0)


@pytest.fixture(scope="module")
def fallback_sets(orc):
    """The unregularised table, as tests/test_sparse_phase2_gpu.py's _fallback_chains makes it, on a panel long enough for four
    checkpoints in either phase-1 half (mid >= 260): forward columns that fall back to uniform, backward columns that are all zero.
    Forward columns depend on the columns in front of them only: kept variants are dropped at the END; backward columns on those
    behind them: dropped at the FRONT.  The witnesses (forward role, from the oracle's output): chain 0's forward columns
    mid - 1 - 64, mid - 1 - 128 and mid - 1 - 256 — checkpoints of phase 1 — fall back."""
    args = (6, 108, 54, 0.0)
    kept = np.flatnonzero(_oracle(orc, synthetic_panel(FB_VARIANTS, 64, 20, seed=6), default_table_args()).kept)
    out = {}
    for role in ("forward", "backward"):
        batches = []
        for d in FB_CHAINS:
            n = _fb_columns(role, d)
            batches.append(_with_columns(orc, _fb_panel(), args, n, kept=kept) if role == "forward"
                           else _with_columns(orc, _fb_panel(), args, n, front=2 * d, kept=kept))
        out[role] = (args, batches, _oracle(orc, batches[0], args))
    mid = _fb_columns("forward", 0) // 2
    out["witness"] = {dist: _forward_column_fell_back(orc, args, kept, mid - 1 - dist) for dist in FB_DISTS}
    return out


@pytest.mark.parametrize("K,G", KG)
@pytest.mark.parametrize("role", ["forward", "backward"])
def test_fallback_columns_on_piece_boundaries_and_inner_checkpoints(role, K, G, fallback_sets, monkeypatch):
    """A flagged checkpoint that is the last column of a piece: the next piece must go on from all-zero states — the single launch
    did, in registers — and not from the stored uniform column, as a chunk launch of phase 2 would.  A flagged checkpoint inside a
    piece: the chain goes on in registers as ever, and the refill segment behind either kind does what it did.  Both must occur, or
    the test says nothing about either: the oracle's output says that the forward columns 64, 128 and 256 behind mid - 1 of chain 0
    fall back — at 64 x 1 all three are piece boundaries (no checkpoint is an inner one there), at 64 x 2 and 128 x 1 the second and
    third, at 128 x 2 the third.  The backward role resumes by the stored sum of the column wherever the checkpoint lies, and the
    oracle's output does not single its all-zero columns out: that half is held to the same bits and to parity alone."""
    args, batches, ref0 = fallback_sets[role]
    if role == "forward":
        witness = fallback_sets["witness"]
        print(f"K={K} G={G}: forward column of chain 0 fell back, by columns behind mid - 1: {witness}")
        on_boundary = [d for d, hit in witness.items() if hit and d % (K * G) == 0]
        on_inner = [d for d, hit in witness.items() if hit and d % (K * G) != 0]
        assert on_boundary, witness
        if K * G > S:
            assert on_inner, witness
    got, n_pieces = _three_ways(batches, args, K, G, monkeypatch)
    assert n_pieces >= 260 // (K * G)
    for d, r in zip(FB_CHAINS, got):
        assert r.n_columns == _fb_columns(role, d)
    assert_parity(batches[0], got[0], ref0)


# ---- resident jobs, and jobs that keep the single launch ------------------------------------------------------------------------
def test_second_run_on_other_counts_gives_the_bits_of_a_fresh_job(orc, monkeypatch):
    """A resident job's next run puts its zeroing and its first piece behind the last k_post of the run before, and its refills
    behind piece events of this run: nothing of the first run's columns, flags or scalars may show."""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    monkeypatch.setenv("PG_PIECE_CHUNKS", "2")
    monkeypatch.delenv("PG_KERNELS", raising=False)
    args = default_table_args()
    batches = [synthetic_panel(700, 64, 20, seed=31), synthetic_panel(300, 64, 20, seed=32)]
    table, params = hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS)
    job = hmm.Job(batches, table, params)
    assert "in 3 pieces" in job.plan()
    job.run()
    first = job.fetch_all()
    for i, b in enumerate(batches):   # (in place: the job re-uploads from the arrays it was made with)
        kc, cov = synthetic_sample_counts(b, seed=77 + i)
        b.kmer_count[:] = kc
        b.coverage[:] = cov
    job.upload()
    job.run()      # (the plain path: phase 1 in pieces)
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


def test_chunk_size_that_is_no_multiple_of_64_keeps_the_single_launch(orc, monkeypatch):
    args = default_table_args()
    b = synthetic_panel(600, 64, 20, seed=41)
    (got,), n_pieces = _three_ways([b], args, 96, 1, monkeypatch, pieces=False)
    assert n_pieces == 1
    assert_parity(b, got, _oracle(orc, b, args))


def test_job_with_a_multiallelic_chain_keeps_the_single_launch(orc, monkeypatch):
    """A chain that is no sparse lean chain runs its phase 1 on another kernel, in one launch: the whole job keeps the single launch
    (and the dense chunk sweeps of phase 2)."""
    args = default_table_args()
    mixed = [synthetic_panel(400, 64, 20, seed=1), synthetic_panel(300, 64, 20, seed=2, multiallelic_frac=0.2)]
    got, n_pieces = _three_ways(mixed, args, 64, 1, monkeypatch, pieces=False)
    assert n_pieces == 1
    for bb, rr in zip(mixed, got):
        assert_parity(bb, rr, _oracle(orc, bb, args))


def test_run_on_a_callers_stream_same_bits(panels, monkeypatch):
    """Job.run(stream=...): pg_job_run takes phase 1 in pieces only on the job's OWN stream; on a caller's stream phase 1 is the
    single launch and phase 2 refills every chunk.  One resident job, run on its own stream, on a caller's and on its own again:
    the same bits each time — chunked (the job is planned in pieces), with PG_SWEEP_MODE unset (two chains: the planner's own
    choice is the chunked job again) and fused, the one schedule that has no second stream."""
    import torch
    all_batches, all_refs = panels
    pick = [COLUMNS.index(129), COLUMNS.index(254)]
    batches, refs = [all_batches[i] for i in pick], [all_refs[i] for i in pick]
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    monkeypatch.setenv("PG_PIECE_CHUNKS", "1")
    monkeypatch.delenv("PG_KERNELS", raising=False)
    theirs = torch.cuda.Stream()
    for mode in ("chunked", None, "fused"):
        if mode:
            monkeypatch.setenv("PG_SWEEP_MODE", mode)
        else:
            monkeypatch.delenv("PG_SWEEP_MODE", raising=False)
        job = hmm.Job(batches, hmm.ProbabilityTable(*default_table_args()), hmm.make_params(*PARAMS))
        assert job.plan().startswith("fused job" if mode == "fused" else "chunked job"), job.plan()
        assert ("in 3 pieces" in job.plan()) == (mode != "fused"), job.plan()
        job.run()
        own = job.fetch_all()
        job.run(stream=theirs.cuda_stream)
        callers = job.fetch_all()
        job.run()
        own_again = job.fetch_all()
        job.close()
        for b, r, r2, r3, ref in zip(batches, own, callers, own_again, refs):
            _same_bits(r, r2)
            _same_bits(r, r3)
            assert_parity(b, r, ref)
