"""Block upkeep of the sparse lean sweeps at fixed steps of the 64-column group (pg_device.h: pg_lean_ring_*; pg_kernels.hip:
lean_ring_open, lean_ring_upkeep).  A sparse launch numbers its column records from the grid of its groups: the first step of a
launch takes a number between 0 and 63, a launch whose first number lies behind the parking step opens with two blocks, the steps
of a group park and expand the next block at two fixed places and carry no test, and the forward role reads its column sums in
front of the next record.  None of it touches a floating-point operation: the results carry the bits of PG_KERNELS=nosparse (every
step tested, numbered from 0) and of PG_KERNELS=nopieces, twice in a row, and match the oracle at the bar of every parity test.

Chains of 64 consecutive lengths put the phase boundary, the leading piece of either role and every launch start on every residue
of the group grid; 640 columns and more wrap the two-block ring twice in a phase-1 half and in a chunk of 128.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from pangenie_amd import hmm
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts
from tests.parity_util import assert_parity
from tests.test_sparse_phase2_gpu import PARAMS, S, _oracle, _same_bits, _with_columns
from tests.test_sparse_pieces_gpu import FB_DISTS, KG, _fb_columns, _fb_panel, _forward_column_fell_back, _three_ways

pytestmark = pytest.mark.gpu

# one, two, three columns (launches without a step); halves around one and two groups; 383 .. 389: the leading piece of a role
# has 63, 0, 1, 2, 3 steps — the first numbers 1, 0, 63, 62, 61, the last three behind the parking step; 675: ragged pieces
COLUMNS = (1, 2, 3, 127, 128, 129, 254, 255, 257, 383, 384, 385, 386, 387, 388, 389, 675)
GRID_FROM, GRID_CHAINS = 640, 64


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _oracles(orc, batches, args):
    with ThreadPoolExecutor(8) as pool:   # (the oracle is C behind ctypes)
        return list(pool.map(lambda b: _oracle(orc, b, args), batches))


@pytest.fixture(scope="module")
def panels(orc):
    args = default_table_args()
    batches = [_with_columns(orc, synthetic_panel(n + 30, 64, 20, seed=1800 + i), args, n) for i, n in enumerate(COLUMNS)]
    return batches, _oracles(orc, batches, args)


@pytest.fixture(scope="module")
def grid(orc):
    """64 chains over ONE panel, 640 .. 703 columns"""
    args = default_table_args()
    kept = np.flatnonzero(_oracle(orc, synthetic_panel(760, 64, 20, seed=1900), args).kept)
    assert kept.size >= GRID_FROM + GRID_CHAINS - 1
    batches = [_with_columns(orc, synthetic_panel(760, 64, 20, seed=1900), args, GRID_FROM + i, kept=kept) for i in range(GRID_CHAINS)]
    return batches, _oracles(orc, batches, args)


@pytest.fixture(scope="module")
def unequal(orc):
    args = default_table_args()
    batches = [synthetic_panel(v, 64, 20, seed=2000 + i) for i, v in enumerate((1400, 150, 517))]
    return batches, _oracles(orc, batches, args)


def _resident(batches, args, orc, K, G, monkeypatch):
    """a resident job run on the counts it was made with, re-uploaded with others and run again: the bits of a fresh job on those"""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    monkeypatch.setenv("PG_PIECE_CHUNKS", str(G))
    monkeypatch.delenv("PG_KERNELS", raising=False)
    table, params = hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS)
    saved = [(b.kmer_count.copy(), b.coverage.copy()) for b in batches]
    try:
        job = hmm.Job(batches, table, params)
        job.run()
        first = job.fetch_all()
        for i, b in enumerate(batches):   # (in place: the job re-uploads from the arrays it was made with)
            kc, cov = synthetic_sample_counts(b, seed=177 + i)
            b.kmer_count[:] = kc
            b.coverage[:] = cov
        job.upload()
        job.run()
        second = job.fetch_all()
        job.close()
        fresh_job = hmm.Job(batches, table, params)
        fresh_job.run()
        fresh = fresh_job.fetch_all()
        fresh_job.close()
        changed = False
        for a, r, f in zip(first, second, fresh):
            changed = changed or not np.array_equal(a.lik, r.lik)
            _same_bits(r, f)
        assert changed   # (the counts did change the posteriors)
    finally:
        for b, (kc, cov) in zip(batches, saved):
            b.kmer_count[:] = kc
            b.coverage[:] = cov


@pytest.mark.parametrize("K,G", KG)
def test_chains_around_the_group_sizes(K, G, panels, orc, monkeypatch):
    batches, refs = panels
    got, _ = _three_ways(batches, default_table_args(), K, G, monkeypatch)
    for n, b, r, ref in zip(COLUMNS, batches, got, refs):
        assert r.n_columns == n
        assert_parity(b, r, ref)
    _resident(batches, default_table_args(), orc, K, G, monkeypatch)


@pytest.mark.parametrize("K,G", KG)
def test_every_residue_of_the_group_grid(K, G, grid, orc, monkeypatch):
    batches, refs = grid
    got, _ = _three_ways(batches, default_table_args(), K, G, monkeypatch)
    for i, (b, r, ref) in enumerate(zip(batches, got, refs)):
        assert r.n_columns == GRID_FROM + i
        assert_parity(b, r, ref)
    _resident(batches, default_table_args(), orc, K, G, monkeypatch)


@pytest.mark.parametrize("K,G", KG)
def test_three_chains_of_unequal_length(K, G, unequal, orc, monkeypatch):
    batches, refs = unequal
    got, _ = _three_ways(batches, default_table_args(), K, G, monkeypatch)
    for b, r, ref in zip(batches, got, refs):
        assert_parity(b, r, ref)
    _resident(batches, default_table_args(), orc, K, G, monkeypatch)


# ---- zero-sum columns ---------------------------------------------------------------------------------------------------------
# chain d has 520 + 2 d columns (mid = 260 + d).  The forward columns that fall back lie where the panel puts them (195, 131, 3: the
# witnesses below), so chain d meets column 195 at step (195 - mid) mod 64 = 63 - d of a group: d = 0 .. 5 puts it on the storing
# step, the plain step behind the upkeep, the expanding step, the parking step and two steps in front of them; d = 31 in mid-group
ZERO_CHAINS = (0, 1, 2, 3, 4, 5, 31)


@pytest.fixture(scope="module")
def zero_sets(orc):
    """tests/test_sparse_pieces_gpu.py's construction (the unregularised table: forward columns that fall back to uniform, backward
    columns that are all zero; kept variants dropped at the end / at the front move the phase boundary, not the columns)"""
    args = (6, 108, 54, 0.0)
    kept = np.flatnonzero(_oracle(orc, synthetic_panel(700, 64, 20, seed=6), default_table_args()).kept)
    out = {}
    for role in ("forward", "backward"):
        batches = [_with_columns(orc, _fb_panel(), args, _fb_columns(role, d), kept=kept) if role == "forward"
                   else _with_columns(orc, _fb_panel(), args, _fb_columns(role, d), front=2 * d, kept=kept) for d in ZERO_CHAINS]
        out[role] = (args, batches, _oracles(orc, batches, args))
    mid = _fb_columns("forward", 0) // 2
    out["witness"] = {dist: _forward_column_fell_back(orc, args, kept, mid - 1 - dist) for dist in FB_DISTS}
    return out


@pytest.mark.parametrize("K,G", [(64, 1), (128, 2)])
@pytest.mark.parametrize("role", ["forward", "backward"])
def test_zero_sum_columns_on_every_step_of_the_upkeep(role, K, G, zero_sets, monkeypatch):
    args, batches, refs = zero_sets[role]
    if role == "forward":
        assert zero_sets["witness"][S], zero_sets["witness"]   # (column 195 of the panel falls back: the comment above stands on it)
    got, _ = _three_ways(batches, args, K, G, monkeypatch)
    for d, b, r, ref in zip(ZERO_CHAINS, batches, got, refs):
        assert r.n_columns == _fb_columns(role, d)
        assert_parity(b, r, ref)
