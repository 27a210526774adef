"""The state block of the lean column step (pg_kernels.hip: lean_states; lean_forward / lean_backward).  A row pair forms both
states' sums in front of their products, and the partial sum starts as the first product (the resume prologues mirror it); the A/B
build that also formed the eight emission addresses of the next column ahead of the column's total was measured slower and is in
history (profiles/r21_lean_pairs.txt).  No floating-point operation changes its operands or its order:
the results carry the bits of the commit before (tests/golden/lean_pairs_parent.npz, written by tools/lean_pairs_golden.py at that
commit), of PG_KERNELS=nosparse and nopieces, twice in a row, and match the oracle at the bar of every parity test.

Chains of 1, 2, 3 columns are launches without a step; 127 .. 129 halves around one group; 383 .. 389 put the leading piece of a
role at 63, 0, 1, 2, 3 steps; 675 has ragged pieces.  The pair panel gives every wave's eight row pairs all four allele
combinations in every column, every pair another one than its neighbours and than the pair four places on (the same byte of the
other register): a wrong byte select fetches another entry of the table.  The zero-sum columns of tests/test_lean_upkeep_gpu.py's
construction refetch a column's emissions behind the state block, where an address formed ahead of it could go stale.
"""
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd import hmm
from pangenie_amd.panel import default_table_args, synthetic_panel
from tests.parity_util import assert_parity
from tests.test_sparse_phase2_gpu import PARAMS, S, _oracle, _with_columns
from tests.test_sparse_pieces_gpu import FB_DISTS, KG, _fb_columns, _fb_panel, _forward_column_fell_back, _three_ways

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "lean_pairs_parent.npz"
COLUMNS = (1, 2, 3, 127, 128, 129, 383, 384, 385, 386, 387, 388, 389, 675)
SEED_CHAINS, SEED_UNEQUAL, SEED_PAIRS = 2100, 2200, 2300
UNFLOORED = (6, 108, 54, 0.0)   # the unregularised table of tests/test_sparse_pieces_gpu.py's fall-back construction
# the allele combination (row 2p, row 2p + 1) of pair p in column v of wave w is PAIR_SEQ[(p + v + 3 w) % 8]: neighbours differ,
# places p and p + 4 differ, and the sequence has no period below 8 (any two places differ in some column)
PAIR_SEQ = (0, 1, 2, 3, 1, 3, 0, 2)
PAIR_COLUMNS = 389
# chain d of the zero-sum construction meets its zero-sum column on step 63 - d of a group: the storing step, the plain step
# behind the upkeep, the expanding step, the parking step (tests/test_lean_upkeep_gpu.py), and one in mid-group
ZERO_CHAINS = (0, 1, 2, 3, 31)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _oracles(orc, batches, args):
    with ThreadPoolExecutor(8) as pool:   # (the oracle is C behind ctypes)
        return list(pool.map(lambda b: _oracle(orc, b, args), batches))


def pair_panel(orc, n_cols=PAIR_COLUMNS, seed=SEED_PAIRS):
    """a 64-path biallelic panel whose path alleles follow PAIR_SEQ, cut to n_cols kept columns; the property is checked here"""
    b = synthetic_panel(n_cols + 40, 64, 20, seed=seed, undefined_frac=0.0)
    V = b.n_variants
    pa = b.path_allele.reshape(V, 64)
    v, w, p = np.meshgrid(np.arange(V), np.arange(4), np.arange(8), indexing="ij")
    comb = np.asarray(PAIR_SEQ)[(p + v + 3 * w) % 8]
    pa[:, :] = np.stack([comb & 1, comb >> 1], axis=-1).reshape(V, 64).astype(pa.dtype)
    b._c = None
    b = _with_columns(orc, b, default_table_args(), n_cols)
    pa = b.path_allele.reshape(V, 64)
    cols = pa[pa.any(axis=1)]
    assert cols.shape[0] == n_cols
    combs = (cols[:, 0::2] + 2 * cols[:, 1::2]).reshape(n_cols, 4, 8)   # [column, wave, pair]
    assert all(set(combs[c, wv]) == {0, 1, 2, 3} for c in range(n_cols) for wv in range(4))
    assert (combs != np.roll(combs, 1, axis=2)).all() and (combs != np.roll(combs, 4, axis=2)).all()
    for d in range(1, 8):   # any two places of a wave hold different combinations in some column
        assert (combs != np.roll(combs, d, axis=2)).any(axis=0).all()
    return b


def _zero_chain(orc, role, d, kept):
    if role == "forward":
        return _with_columns(orc, _fb_panel(), UNFLOORED, _fb_columns(role, d), kept=kept)
    return _with_columns(orc, _fb_panel(), UNFLOORED, _fb_columns(role, d), front=2 * d, kept=kept)


def _zero_kept(orc):
    return np.flatnonzero(_oracle(orc, synthetic_panel(700, 64, 20, seed=6), default_table_args()).kept)


def golden_chains(orc):
    """the six chains of tests/golden/lean_pairs_parent.npz as (name, table arguments, batch): a launch without a step, a half of one
    group and a column, the leading pieces behind the parking step, the pair panel, a zero-sum column on the expanding step of
    the forward role and on the parking step of the backward role"""
    args, kept = default_table_args(), _zero_kept(orc)
    out = [(f"c{n}", args, _with_columns(orc, synthetic_panel(n + 30, 64, 20, seed=SEED_CHAINS + COLUMNS.index(n)), args, n)) for n in (3, 129, 386)]
    out.append(("pairs", args, pair_panel(orc)))
    out.append(("zero_forward", UNFLOORED, _zero_chain(orc, "forward", 2, kept)))
    out.append(("zero_backward", UNFLOORED, _zero_chain(orc, "backward", 3, kept)))
    return out


def run_golden(chains, K, G, setenv):
    """name -> result of each golden chain, run as a job of its own at chunks of K columns, G chunks a piece"""
    setenv("PG_SWEEP_MODE", "chunked")
    setenv("PG_CHUNK_COLS", str(K))
    setenv("PG_PIECE_CHUNKS", str(G))
    out = {}
    for name, args, b in chains:
        job = hmm.Job([b], hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS))
        job.run()
        out[name] = job.fetch_all()[0]
        job.close()
    return out


@pytest.fixture(scope="module")
def panels(orc):
    args = default_table_args()
    batches = [_with_columns(orc, synthetic_panel(n + 30, 64, 20, seed=SEED_CHAINS + i), args, n) for i, n in enumerate(COLUMNS)]
    return batches, _oracles(orc, batches, args)


@pytest.fixture(scope="module")
def unequal(orc):
    args = default_table_args()
    batches = [synthetic_panel(v, 64, 20, seed=SEED_UNEQUAL + i) for i, v in enumerate((1400, 150, 517))]
    return batches, _oracles(orc, batches, args)


@pytest.fixture(scope="module")
def pairs(orc):
    b = pair_panel(orc)
    return b, _oracle(orc, b, default_table_args())


@pytest.fixture(scope="module")
def zero_sets(orc):
    kept = _zero_kept(orc)
    out = {}
    for role in ("forward", "backward"):
        batches = [_zero_chain(orc, role, d, kept) for d in ZERO_CHAINS]
        out[role] = (batches, _oracles(orc, batches, UNFLOORED))
    mid = _fb_columns("forward", 0) // 2
    out["witness"] = {dist: _forward_column_fell_back(orc, UNFLOORED, kept, mid - 1 - dist) for dist in FB_DISTS}
    return out


@pytest.fixture(scope="module")
def parent_bits(orc):
    return golden_chains(orc), np.load(GOLDEN)


@pytest.mark.parametrize("K,G", KG)
def test_chains_around_the_group_sizes(K, G, panels, monkeypatch):
    batches, refs = panels
    got, _ = _three_ways(batches, default_table_args(), K, G, monkeypatch)
    for n, b, r, ref in zip(COLUMNS, batches, got, refs):
        assert r.n_columns == n
        assert_parity(b, r, ref)


@pytest.mark.parametrize("K,G", KG)
def test_three_chains_of_unequal_length(K, G, unequal, monkeypatch):
    batches, refs = unequal
    got, _ = _three_ways(batches, default_table_args(), K, G, monkeypatch)
    for b, r, ref in zip(batches, got, refs):
        assert_parity(b, r, ref)


@pytest.mark.parametrize("K,G", KG)
def test_every_pair_byte_selects_its_own_table_entry(K, G, pairs, monkeypatch):
    b, ref = pairs
    got, _ = _three_ways([b], default_table_args(), K, G, monkeypatch)
    assert got[0].n_columns == PAIR_COLUMNS
    assert_parity(b, got[0], ref)


@pytest.mark.parametrize("K,G", [(64, 1), (128, 2)])
@pytest.mark.parametrize("role", ["forward", "backward"])
def test_zero_sum_columns_on_every_kind_of_step(role, K, G, zero_sets, monkeypatch):
    batches, refs = zero_sets[role]
    if role == "forward":
        assert zero_sets["witness"][S], zero_sets["witness"]   # (column 195 of the panel falls back: ZERO_CHAINS stands on it)
    got, _ = _three_ways(batches, UNFLOORED, K, G, monkeypatch)
    for d, b, r, ref in zip(ZERO_CHAINS, batches, got, refs):
        assert r.n_columns == _fb_columns(role, d)
        assert_parity(b, r, ref)


@pytest.mark.parametrize("K,G", KG)
def test_same_bytes_as_the_commit_before(K, G, parent_bits, monkeypatch):
    chains, want = parent_bits
    got = run_golden(chains, K, G, monkeypatch.setenv)
    assert sorted(want["names"]) == sorted(got)
    for name, r in got.items():
        assert np.array_equal(r.kept, want[name + ".kept"]), name
        assert np.array_equal(r.lik_exp, want[name + ".lik_exp"]), name
        assert r.lik.tobytes() == want[name + ".lik"].tobytes(), name
