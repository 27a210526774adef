"""The preparation beside phase 1 (pg_job::prep_beside; pg_shim_run.cpp: prepare_in_parts; pg_device.h: pg_prep_middle): a job that
runs phase 1 in pieces and whose chains are all-biallelic prepares only the ENDS of its chains — what the first E pieces read — ahead
of phase 1 (k_prep_bi_part, k_records_part on the job's stream) and their MIDDLE on the second stream beside those pieces; the job's
stream waits for the middle in front of piece n_pieces - E - 1.  Which variants are prepared where and when changes no value: the
results carry the bits of PG_KERNELS=prepahead (the whole preparation ahead), of nopieces and of nosparse, and match the oracle at
the bar of every parity test.  PG_PREP_EARLY_PIECES = E puts the wait behind the first piece (1), at the default (2) and directly
in front of piece 0 (n_pieces - 1).

The chains are those of tests/test_sparse_pieces_gpu.py: at 64 columns a chunk and one chunk a piece the 675-column chain has six
pieces and, at E = 2, ends of 81 and 82 columns, and every shorter chain is all middle (tests/test_prep_parts.py)."""
import numpy as np
import pytest

from pangenie_amd import hmm
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts
from tests.parity_util import assert_parity
from tests.test_sparse_phase2_gpu import PARAMS, _oracle, _same_bits, _with_columns
from tests.test_sparse_pieces_gpu import COLUMNS, _n_pieces

pytestmark = pytest.mark.gpu

K = 64
AHEAD = "prep ahead of the sweeps"


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _beside(E, n_pieces):
    return f"prep in parts: the ends of the chains ahead of the sweeps, their middle beside the first {E} of {n_pieces} pieces"


def _run(batches, args, says):
    """one job, run twice (a resident job: the second run's part 2 follows the first run's k_post): the same bits; `says`: what the plan's first line must say"""
    job = hmm.Job(batches, hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS))
    head = job.plan().splitlines()[0]
    assert says in head, job.plan()
    assert ("prep in parts" in head) == (says != AHEAD), job.plan()
    job.run()
    first = job.fetch_all()
    job.run()
    again = job.fetch_all()
    job.close()
    for r, r2 in zip(first, again):
        _same_bits(r, r2)
    return first


_others = {}   # (set, G) -> the results under prepahead, nopieces and nosparse: they do not hang on E


def _other_ways(name, batches, args, G, monkeypatch):
    if (name, G) not in _others:
        monkeypatch.delenv("PG_PREP_EARLY_PIECES", raising=False)
        ways = []
        for tok in ("prepahead", "nopieces", "nosparse"):
            monkeypatch.setenv("PG_KERNELS", tok)
            ways.append(_run(batches, args, AHEAD))
        monkeypatch.delenv("PG_KERNELS", raising=False)
        _others[(name, G)] = ways
    return _others[(name, G)]


def _check(name, batches, refs, G, early, monkeypatch):
    args = default_table_args()
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    monkeypatch.setenv("PG_PIECE_CHUNKS", str(G))
    n_pieces = _n_pieces(batches, K, G)
    E = n_pieces - 1 if early == "last" else early
    ways = _other_ways(name, batches, args, G, monkeypatch)
    monkeypatch.delenv("PG_KERNELS", raising=False)
    monkeypatch.setenv("PG_PREP_EARLY_PIECES", str(E))
    got = _run(batches, args, _beside(E, n_pieces))
    for way in ways:
        for r, w in zip(got, way):
            _same_bits(r, w)
    for b, r, ref in zip(batches, got, refs):
        assert_parity(b, r, ref)
    return got, n_pieces


@pytest.fixture(scope="module")
def panels(orc):
    args = default_table_args()
    batches = [_with_columns(orc, synthetic_panel(n + 30, 64, 20, seed=1100 + i), args, n) for i, n in enumerate(COLUMNS)]
    return batches, [_oracle(orc, b, args) for b in batches]


@pytest.fixture(scope="module")
def unequal(orc):
    """one chain with ends, two without (at E = 2: chunks of 64 columns, one or two a piece)"""
    args = default_table_args()
    batches = [synthetic_panel(v, 64, 20, seed=1200 + i) for i, v in enumerate((1400, 150, 517))]
    return batches, [_oracle(orc, b, args) for b in batches]


CASES = [(1, 1), (1, 2), (1, "last"), (2, 1), (2, 2)]   # (PG_PIECE_CHUNKS, PG_PREP_EARLY_PIECES); at G = 2 there are 3 pieces: "last" is 2


@pytest.mark.parametrize("G,early", CASES)
def test_same_bits_as_the_preparation_ahead_and_oracle(G, early, panels, monkeypatch):
    batches, refs = panels
    got, n_pieces = _check("columns", batches, refs, G, early, monkeypatch)
    assert n_pieces == {1: 6, 2: 3}[G]
    for n, r in zip(COLUMNS, got):
        assert r.n_columns == n


@pytest.mark.parametrize("G,early", CASES)
def test_three_chains_of_unequal_length(G, early, unequal, monkeypatch):
    batches, refs = unequal
    got, n_pieces = _check("unequal", batches, refs, G, early, monkeypatch)
    assert n_pieces == {1: 11, 2: 6}[G]
    if early == 2:   # one chain has ends, two have none
        W = (n_pieces - 2) * G * K
        halves = [r.n_columns // 2 for r in got]
        assert halves[0] > W and halves[1] < W and halves[2] < W, (halves, W)


def test_second_run_on_other_counts_gives_the_bits_of_a_fresh_job(orc, monkeypatch):
    """A resident job run on counts A, its counts replaced by B, run again: the bits of a fresh job on B.  A record of the middle
    left over from A — part 2 not waited for, or not run — would show here."""
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    monkeypatch.setenv("PG_PIECE_CHUNKS", "1")
    monkeypatch.delenv("PG_KERNELS", raising=False)
    monkeypatch.delenv("PG_PREP_EARLY_PIECES", raising=False)
    args = default_table_args()
    batches = [synthetic_panel(700, 64, 20, seed=31), synthetic_panel(300, 64, 20, seed=32)]
    table, params = hmm.ProbabilityTable(*args), hmm.make_params(*PARAMS)
    job = hmm.Job(batches, table, params)
    assert _beside(2, 6) in job.plan(), job.plan()
    job.run()
    first = job.fetch_all()
    assert first[0].n_columns // 2 > 4 * K   # (the long chain has ends)
    for i, b in enumerate(batches):   # (in place: the job re-uploads from the arrays it was made with)
        kc, cov = synthetic_sample_counts(b, seed=77 + i)
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
    for b, a, r, f in zip(batches, first, second, fresh):
        assert not np.array_equal(a.lik, r.lik)   # (the counts did change the posteriors)
        _same_bits(r, f)
        assert_parity(b, r, _oracle(orc, b, args))


def test_jobs_that_keep_the_preparation_ahead_say_so(orc, monkeypatch):
    """No pieces (a chunk size that is no multiple of 64), a chain that is not k_prep_bi's alone, and fewer than E + 1 pieces."""
    args = default_table_args()
    monkeypatch.setenv("PG_SWEEP_MODE", "chunked")
    monkeypatch.setenv("PG_PIECE_CHUNKS", "1")
    monkeypatch.delenv("PG_KERNELS", raising=False)
    monkeypatch.delenv("PG_PREP_EARLY_PIECES", raising=False)
    b = synthetic_panel(600, 64, 20, seed=41)
    monkeypatch.setenv("PG_CHUNK_COLS", "96")
    (got,) = _run([b], args, AHEAD)
    ref = _oracle(orc, b, args)
    assert_parity(b, got, ref)
    monkeypatch.setenv("PG_CHUNK_COLS", str(K))
    mixed = [synthetic_panel(400, 64, 20, seed=1), synthetic_panel(300, 64, 20, seed=2, multiallelic_frac=0.2)]
    for bb, rr in zip(mixed, _run(mixed, args, AHEAD)):
        assert_parity(bb, rr, _oracle(orc, bb, args))
    n_pieces = _n_pieces([b], K, 1)
    assert n_pieces == 5
    monkeypatch.setenv("PG_PREP_EARLY_PIECES", str(n_pieces))      # n_pieces < E + 1
    (kept_ahead,) = _run([b], args, AHEAD)
    monkeypatch.setenv("PG_PREP_EARLY_PIECES", str(n_pieces - 1))
    (beside,) = _run([b], args, _beside(n_pieces - 1, n_pieces))
    _same_bits(kept_ahead, beside)
    assert_parity(b, beside, ref)
