"""Sparse phase 2 of chunked jobs whose chains are all lean chains (DevContig::sparse2): a chunk sweep stores only every 64th
column, counted on from the phase boundary, into an area of the chain's own; k_refill_lean forms the chunk's columns from those
checkpoints into the scratch buffer behind the sweep, and k_post reads them as ever.  The sweeps no longer wait for k_post.  A
refilled column comes from the same instructions as a stored one, so the results carry the same bits as with PG_KERNELS=nosparse2
(dense chunk sweeps) and PG_KERNELS=nosparse (dense phase 1 too) — and match the oracle at the bar of every parity test.

Kept columns per chain are set exactly, as in tests/test_sparse_phase1_gpu.py: with mid = C / 2 the forward role's phase-2 half
has C - mid columns, the backward role's mid.
"""
import numpy as np
import pytest

from pangenie_amd import hmm
from pangenie_amd.panel import default_table_args, synthetic_panel
from tests.parity_util import assert_parity

pytestmark = pytest.mark.gpu

S = 64
PARAMS = (1.26, False, 1e-5)
SPARSE2 = "chunks (sparse: every 64th column stored) + k_refill_lean (both halves) + k_post"
SPARSE1 = "chunks + k_refill_lean + k_post"


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


def _lean_lines(plan):
    return [ln for ln in plan.splitlines() if "k_sweep_lean<3>" in ln]


def _run(batches, args, form):
    """form: "sparse2" (both phases sparse), "sparse1" (dense chunk sweeps), "dense" (no k_refill_lean at all) — what the plan must say"""
    job = hmm.Job(batches, hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS))
    plan = job.plan()
    lines = _lean_lines(plan)
    assert lines, plan
    for ln in lines:
        assert (SPARSE2 in ln) == (form == "sparse2"), plan
        assert (SPARSE1 in ln) == (form == "sparse1"), plan
        assert ("k_refill_lean" in ln) == (form != "dense"), plan
    for ln in plan.splitlines():
        if ln not in lines:
            assert "k_refill_lean" not in ln, plan
    job.run()
    first = job.fetch_all()
    job.run()   # (a resident job: the second run fills the same checkpoint area and scratch buffers again)
    again = job.fetch_all()
    job.close()
    for r, r2 in zip(first, again):
        _same_bits(r, r2)
    return first


def _same_bits(a, b):
    assert a.n_columns == b.n_columns
    assert np.array_equal(a.kept, b.kept)
    assert np.array_equal(a.lik_exp, b.lik_exp)
    assert np.array_equal(a.lik, b.lik), f"{int((a.lik != b.lik).sum())} of {a.lik.size} bins differ"


def _three_ways(batches, args, monkeypatch, default_form="sparse2"):
    """the default plan, PG_KERNELS=nosparse2 and PG_KERNELS=nosparse: the same bits; returns the default plan's results"""
    monkeypatch.delenv("PG_KERNELS", raising=False)
    got = _run(batches, args, default_form)
    monkeypatch.setenv("PG_KERNELS", "nosparse2")
    dense2 = _run(batches, args, "sparse1" if default_form != "dense" else "dense")
    monkeypatch.setenv("PG_KERNELS", "nosparse")
    dense = _run(batches, args, "dense")
    monkeypatch.delenv("PG_KERNELS", raising=False)
    for r, d2, d in zip(got, dense2, dense):
        _same_bits(r, d2)
        _same_bits(r, d)
    return got


# columns per chain (S = 64, the checkpoint spacing): one, two, three columns (empty and one-column phase-2 halves); halves below S
# (a ragged piece and nothing else); of exactly S (a chunk that is one segment), S + 1 (a ragged piece of one column) and 2 S - 1
# (one of 63) in either half; several chunks; odd C (the halves differ)
COLUMNS = (1, 2, 3, 80, 2 * S - 1, 2 * S, 2 * S + 1, 2 * S + 2, 2 * S + 3, 4 * S - 3, 4 * S - 2, 4 * S - 1, 6 * S + 2, 10 * S + 34, 10 * S + 35)


@pytest.fixture(scope="module")
def panels(orc):
    """the chains of COLUMNS and their oracle results, made once for both chunk sizes"""
    args = default_table_args()
    batches = [_with_columns(orc, synthetic_panel(n + 30, 64, 20, seed=500 + i), args, n) for i, n in enumerate(COLUMNS)]
    return batches, [_oracle(orc, b, args) for b in batches]


@pytest.mark.parametrize("K", [64, 128])
def test_sparse_phase2_same_bits_as_dense_and_oracle(K, panels, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    args = default_table_args()
    batches, refs = panels
    got = _three_ways(batches, args, monkeypatch)
    for n, b, r, ref in zip(COLUMNS, batches, got, refs):
        assert r.n_columns == n
        assert_parity(b, r, ref)


def test_three_chains_of_unequal_length(orc, monkeypatch):
    """The short chains run out of columns chunks before the long one: its late sweep, refill and k_post launches walk chains
    without columns.  22 chunks: the sweeps, which nothing ties to the second stream any more, run well ahead of it."""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    args = default_table_args()
    batches = [synthetic_panel(v, 64, 20, seed=700 + i) for i, v in enumerate((1400, 150, 517))]
    got = _three_ways(batches, args, monkeypatch)
    for b, r in zip(batches, got):
        assert_parity(b, r, _oracle(orc, b, args))


# ---- fall-back columns ------------------------------------------------------------------------------------------------------
N_FULL = 386   # columns of the longest chain of the construction below: mid = 130 .. 193 over its 64 chains


def _fallback_chains(orc, role):
    """The unregularised table: forward columns that fall back to uniform, backward columns that are all zero.  Where they lie hangs
    on the panel; where the checkpoints lie on mid alone.  64 chains over ONE panel whose mid takes 64 consecutive values.  Forward
    columns depend on the columns in front of them only, so kept variants are dropped at the END (C = 260 + 2 d, mid = 130 + d: a
    column at a fixed place is 64 different distances from mid - 1); backward columns on those behind them, so they are dropped at
    the FRONT (two per chain).  mid >= 130 puts two checkpoints into either phase-2 half: at 128 columns per chunk an inner one
    and a chunk's last column."""
    args = (6, 108, 54, 0.0)
    kept = np.flatnonzero(_oracle(orc, synthetic_panel(430, 64, 20, seed=6), default_table_args()).kept)
    batches = []
    for d in range(64):
        b = synthetic_panel(430, 64, 20, seed=6)
        b.kmer_count[::3] = 0
        b.kmer_count[1::17] = 6000
        if role == "forward":
            batches.append(_with_columns(orc, b, args, N_FULL - 2 * (63 - d), kept=kept))
        else:
            batches.append(_with_columns(orc, b, args, N_FULL - 2 * d, front=2 * d, kept=kept))
    return args, batches


def _n_columns(role, d):
    return N_FULL - 2 * (63 - d) if role == "forward" else N_FULL - 2 * d


def _forward_column_fell_back(orc, args, kept, c):
    """Does forward column c of the construction's panel fall back to the uniform column?  Read from the oracle's output: in the
    chain cut off behind column c the backward column of c is all ones, so the bins of c are its forward column added up by
    genotype — for the uniform column exactly (n0^2, 2 n0 n1, n1^2) / 4096 with n0, n1 the paths on either allele, which a
    forward column that carries its emission does not give."""
    b = synthetic_panel(430, 64, 20, seed=6)
    b.kmer_count[::3] = 0
    b.kmer_count[1::17] = 6000
    b = _with_columns(orc, b, args, c + 1, kept=kept)
    ref = _oracle(orc, b, args)
    v = int(np.flatnonzero(ref.kept)[c])
    bins = np.asarray(ref.lik[int(ref.geno_off[v]):int(ref.geno_off[v + 1])], dtype=np.float64)
    n1 = int((b.path_allele.reshape(b.n_variants, b.n_paths)[v] != 0).sum())
    n0 = 64 - n1
    return bins.size == 3 and np.array_equal(bins, np.array([n0 * n0, 2 * n0 * n1, n1 * n1]) / 4096.0)


@pytest.fixture(scope="module")
def fallback_sets(orc):
    out = {}
    for role in ("forward", "backward"):
        args, batches = _fallback_chains(orc, role)
        ends = (0, 63)   # the two chains that are compared with the oracle (the oracle takes a second per chain on this table)
        out[role] = (args, batches, {d: _oracle(orc, batches[d], args) for d in ends})
    # witnesses for the forward role: a chain d and a flagged forward column 64 / 128 steps behind its phase-1 checkpoint mid - 1
    args = out["forward"][0]
    kept = np.flatnonzero(_oracle(orc, synthetic_panel(430, 64, 20, seed=6), default_table_args()).kept)
    witness = {}
    for dist in (S, 2 * S):
        for d in range(64):
            n = _n_columns("forward", d)
            f = n // 2 - 1 + dist
            if f < n and _forward_column_fell_back(orc, args, kept, f):
                witness[dist] = (d, f)
                break
    out["witness"] = witness
    return out


@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("role", ["forward", "backward"])
def test_fallback_columns_on_chunk_boundary_and_inner_checkpoints(role, K, fallback_sets, monkeypatch):
    """A flagged checkpoint inside a chunk: the chain went on in registers from all-zero states, and so does the segment behind it.
    A flagged checkpoint that is a chunk's last column: the next chunk launch resumed from the stored uniform column, and so does
    the segment.  Both must occur in this construction, or the test says nothing about either: the oracle's output names a chain
    with a flagged forward column on its first phase-2 checkpoint (a chunk's last column at 64 columns per chunk, an inner
    checkpoint at 128) and one with such a column on its second (a chunk's last column at either size).  The backward role's
    resume takes one path wherever the checkpoint lies (the stored sum of the column says whether it is all zero), and the
    oracle's output does not single its all-zero columns out: that half of the construction is held to the same bits alone."""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    args, batches, refs = fallback_sets[role]
    if role == "forward":
        witness = fallback_sets["witness"]
        print(f"K={K}: (chain, flagged forward column) by steps behind mid - 1: {witness}")
        on_boundary = [w for dist, w in witness.items() if dist % K == 0]
        on_inner = [w for dist, w in witness.items() if dist % K != 0]
        assert on_boundary, witness
        if K > S:
            assert on_inner, witness
        for dist, (d, f) in witness.items():   # (the witness is a checkpoint of a phase-2 half of the chain that is run below)
            n = _n_columns(role, d)
            assert n // 2 <= f < n and (f - (n // 2 - 1)) == dist
    got = _three_ways(batches, args, monkeypatch)
    for d, (b, r) in enumerate(zip(batches, got)):
        assert r.n_columns == _n_columns(role, d)
        if d in refs:
            assert_parity(b, r, refs[d])


def test_chunk_size_that_is_no_multiple_of_64_keeps_the_dense_phase2(orc, monkeypatch):
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "96")
    args = default_table_args()
    b = synthetic_panel(600, 64, 20, seed=41)
    (r,) = _three_ways([b], args, monkeypatch, default_form="dense")
    assert_parity(b, r, _oracle(orc, b, args))


def test_job_with_a_multiallelic_chain_keeps_the_dense_phase2(orc, monkeypatch):
    """A chain that is no sparse lean chain stores its chunk columns into the scratch buffers from the sweep's stream: the whole job
    keeps the buffer rotation with its waits for k_post, and dense chunk sweeps."""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", "64")
    args = default_table_args()
    mixed = [synthetic_panel(400, 64, 20, seed=1), synthetic_panel(300, 64, 20, seed=2, multiallelic_frac=0.2)]
    got = _three_ways(mixed, args, monkeypatch, default_form="sparse1")
    for bb, rr in zip(mixed, got):
        assert_parity(bb, rr, _oracle(orc, bb, args))
