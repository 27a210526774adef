"""Phase 1 of sparse lean chains in pieces (pangenie_amd/csrc/pg_device.h: pg_sparse_piece; include/pangenie_hmm.h:
pg_sparse_piece_range), on the host.  Piece g of a role holds its phase-1 columns whose partner chunk of phase 2 lies in
[g G, (g + 1) G); pg_job_run launches the pieces from the farthest down to piece 0 and, behind every piece but piece 0, the refills
of that piece's chunks on the second stream; phase 2 refills piece 0's chunks as ever.  For every column count, chunk size and G:
the pieces partition the role's phase-1 half, every boundary between two pieces is a column the chain stores (what the next piece
resumes from), every refill segment resumes from a checkpoint inside a piece that has run when the refill is launched, and the
refills of phase 1 and of phase 2 together write every column the chain does not store exactly once.  No device involved."""
import ctypes as C
import functools

import numpy as np
import pytest

from pangenie_amd import _lib, build

S = 64


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_hip()


@functools.lru_cache(maxsize=8)
def _stored(lib, n, role):
    return np.array([lib.pg_sparse_stored_by_chain(n, role, c) for c in range(n)], dtype=bool)


def _pieces(lib, n, K, G, role, n_pieces):
    out = (C.c_uint32 * 2)()
    got = {}
    for g in range(n_pieces + 1):   # (one more than the job has: it must be empty)
        rc = lib.pg_sparse_piece_range(n, K, G, g, role, out)
        assert rc in (0, 1)
        if rc:
            got[g] = (int(out[0]), int(out[1]))
    return got


def _check(lib, n, K, G):
    mid = n // 2
    q = K // S
    n_chunks = (n // 2 + 1 + K - 1) // K             # what a job of this one chain has (the longer half has at most n / 2 + 1 columns)
    n_pieces = (n_chunks + G - 1) // G
    seg = (C.c_uint32 * 3)()
    for role in (0, 1):
        lo_h, hi_h = (0, mid - 1) if role == 0 else (mid, n - 1)   # the role's phase-1 half
        stored = _stored(lib, n, role)
        pieces = _pieces(lib, n, K, G, role, n_pieces)
        # ---- the pieces partition the half: piece 0 at the phase boundary, each next one adjacent and farther away
        assert n_pieces not in pieces
        if hi_h < lo_h:
            assert not pieces
            continue
        assert sorted(pieces) == list(range(len(pieces))), (n, K, G, role)
        piece_of = np.full(n, -1, dtype=np.int64)
        edge = hi_h + 1 if role == 0 else lo_h - 1    # the column next to the phase boundary's side of the piece
        for g in sorted(pieces):
            lo, hi = pieces[g]
            assert lo <= hi
            assert (hi == edge - 1) if role == 0 else (lo == edge + 1), (n, K, G, role, g)
            edge = lo if role == 0 else hi
            assert (piece_of[lo:hi + 1] == -1).all()
            piece_of[lo:hi + 1] = g
            last = g == len(pieces) - 1
            assert hi - lo + 1 == G * K or (last and hi - lo + 1 < G * K)   # (whole pieces are even: the step's two record variables)
            # the partner chunk of every column of the piece lies in [g G, (g + 1) G)
            for c in (lo, hi):
                chunk = (mid - 1 - c) // K if role == 0 else (c - mid) // K
                assert g * G <= chunk < (g + 1) * G
            if not last:   # an interior boundary: the farther piece ends on a column the chain stores, which this one resumes from
                ck = lo - 1 if role == 0 else hi + 1
                assert lo_h <= ck <= hi_h and stored[ck], (n, K, G, role, g)
                assert lib.pg_sparse_stored_by_chain(n, role, ck) == 1
        assert (piece_of[lo_h:hi_h + 1] >= 0).all() and (np.delete(piece_of, np.s_[lo_h:hi_h + 1]) == -1).all()
        # ---- pg_job_run's order: piece g, then (g > 0) the refills of its chunks; piece 0's chunks in phase 2
        written = np.zeros(n, dtype=np.int32)
        ran = set()

        def refill(chunk, g_launched):
            for j in range(q):
                rc = lib.pg_sparse_segment(n, K, chunk, role, j, seg)
                assert rc in (0, 1)
                if rc == 0:
                    continue
                ck, lo, hi = int(seg[0]), int(seg[1]), int(seg[2])
                assert stored[ck] and piece_of[ck] >= g_launched and piece_of[ck] in ran, (n, K, G, role, chunk, j)
                assert (piece_of[lo:hi + 1] == g_launched).all()   # (it writes columns of the piece it is launched behind)
                written[lo:hi + 1] += 1

        in_phase1 = set()
        for g in range(n_pieces - 1, -1, -1):
            ran.add(g)
            if g == 0:
                break
            for chunk in range(min((g + 1) * G, n_chunks) - 1, g * G - 1, -1):
                refill(chunk, g)
                in_phase1.add(chunk)
        for chunk in range(n_chunks):
            if chunk < G:
                assert chunk not in in_phase1
                refill(chunk, 0)
            else:
                assert chunk in in_phase1
        cover = written + stored.astype(np.int32)
        assert (cover[lo_h:hi_h + 1] == 1).all(), (n, K, G, role)
        assert written[:lo_h].sum() == 0 and written[hi_h + 1:].sum() == 0


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("K", [64, 128, 8192])
def test_pieces_partition_the_half_and_refills_follow_their_checkpoints(lib, K, G):
    for n in list(range(1, 701)) + [1023, 1024, 1025, 16385, 49153]:
        _check(lib, n, K, G)


@pytest.mark.parametrize("K", [64, 8192])
def test_whole_chromosome(lib, K):
    for G in (1, 2, 4):
        _check(lib, 397000, K, G)
        _check(lib, 397001, K, G)


def test_arguments_outside_the_scheme(lib):
    out = (C.c_uint32 * 2)()
    assert lib.pg_sparse_piece_range(1000, 96, 1, 0, 0, out) == -1     # chunk size no multiple of 64: one phase-1 launch
    assert lib.pg_sparse_piece_range(1000, 0, 1, 0, 0, out) == -1
    assert lib.pg_sparse_piece_range(1000, 64, 0, 0, 0, out) == -1
    assert lib.pg_sparse_piece_range(1000, 64, 1, 0, 2, out) == -1
    assert lib.pg_sparse_piece_range(1000, 1 << 31, 2, 0, 0, out) == -1    # a piece wider than 32 bits hold
    assert lib.pg_sparse_piece_range(1000, 64, 1, 0, 0, None) == 1
    assert lib.pg_sparse_piece_range(0, 64, 1, 0, 0, out) == 0 and lib.pg_sparse_piece_range(0, 64, 1, 0, 1, out) == 0
    assert lib.pg_sparse_piece_range(1, 64, 1, 0, 0, out) == 0             # a single column is the backward role's
    assert lib.pg_sparse_piece_range(1, 64, 1, 0, 1, out) == 1 and (int(out[0]), int(out[1])) == (0, 0)
    # a long chain: the arithmetic stays inside 32 bits' reach
    assert lib.pg_sparse_piece_range(0xFFFFFFFF, 8192, 4, 0xFFFF, 1, out) == 1
    assert (int(out[0]), int(out[1])) == (0x7FFFFFFF + 0xFFFF * 32768, 0x7FFFFFFF + 0x10000 * 32768 - 1)
    assert lib.pg_sparse_piece_range(0xFFFFFFFF, 8192, 4, 0x10000, 1, out) == 0   # behind the last column
