"""Who writes the per-column scalars of a sparse lean chain (pangenie_amd/csrc/pg_kernels.hip: lean_forward / lean_backward), on
the host.  The rule: fscale[c] / bscale[c] is written by whoever writes column c — the chain at the columns it stores (its
store-free step parks no scalar), a refill segment (k_refill_lean) at the columns it forms, except the closing checkpoint of a
phase-2 segment, which the chain stored.  bsum is written by the chain alone, at the columns it stores.

With the arithmetic the kernels use (pg_device.h: pg_sparse_* / pg_sparse2_*, through the hooks of tests/test_sparse_segments.py
and tests/test_sparse2_segments.py), for every column count, either role and every chunk size:
  * every entry of fscale and of bscale has exactly one writer among the chain's stored columns, the phase-1 segments and the
    phase-2 segments — also where only phase 1 is sparse (dense chunk sweeps: a job with another kind of chain in it);
  * every column a chunk launch or a segment resumes from is one the chain stored, so its bsum exists.
A chunk size that is no multiple of 64 keeps the dense sweeps: no segment exists and the chain writes every entry.  No device
involved."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib, build

S = 64


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_hip()


def _halves(n, role):
    """(phase-1 half, phase-2 half) of a role as boolean masks: forward 0 .. mid-1 then mid .. n-1, backward the other way round"""
    mid = n // 2
    first = np.zeros(n, dtype=bool)
    if role == 0:
        first[:mid] = True
    else:
        first[mid:] = True
    return first, ~first


def _writers(lib, n, K, role, sparse2):
    """writers per entry of the role's scale array (fscale: role 0, bscale: role 1), the columns whose bsum-style hand-over the chain
    writes, and the columns that launches and segments resume from"""
    mid = n // 2
    out = (C.c_uint32 * 3)()
    half1, half2 = _halves(n, role)
    writers = np.zeros(n, dtype=np.int32)
    chain = np.zeros(n, dtype=bool)
    resumes = []
    if K % S:
        # dense sweeps: the hooks know no segment, the chain stores and scales every column
        assert lib.pg_sparse_segment(n, K, 0, role, 0, out) == -1 and lib.pg_sparse_chunk_segment(n, K, 0, role, 0, out) == -1
        chain[:] = True
        writers += 1
        top = mid - 1
        while role == 1 and top >= 0:   # the chunk launches of the backward role's phase 2: Sy = bsum[top + 1]
            resumes.append(top + 1)
            top -= K
        return writers, chain, resumes
    q = K // S
    n_chunks = (max(mid, n - mid) + K - 1) // K + 1
    # phase 1: the chain at the columns it stores (the leading piece and the checkpoints), the partner segments at the rest
    for c in np.flatnonzero(half1):
        if lib.pg_sparse_stored_by_chain(n, role, int(c)):
            chain[c] = True
    for chunk in range(n_chunks):
        for j in range(q):
            rc = lib.pg_sparse_segment(n, K, chunk, role, j, out)
            assert rc in (0, 1)
            if rc:
                ck, lo, hi = int(out[0]), int(out[1]), int(out[2])
                writers[lo:hi + 1] += 1
                resumes.append(ck)
    # phase 2: a chain of a single column keeps the dense store of the recursion's initial column (sweep_lean_body)
    if not sparse2 or n < 2:
        chain |= half2
    else:
        for c in np.flatnonzero(half2):
            if lib.pg_sparse_chunk_stored_by_chain(n, role, int(c)):
                chain[c] = True
        for chunk in range(n_chunks):
            for j in range(q):
                rc = lib.pg_sparse_chunk_segment(n, K, chunk, role, j, out)
                assert rc in (0, 1)
                if rc:
                    ck, lo, hi = int(out[0]), int(out[1]), int(out[2])
                    writers[lo:hi + 1] += 1
                    last = hi if role == 0 else lo   # the closing checkpoint, if the chain stored it: the chain's entry
                    if lib.pg_sparse_chunk_stored_by_chain(n, role, last):
                        writers[last] -= 1
                    resumes.append(ck)
    # the chunk launches of phase 2 resume from the column in front of the chunk (in the role's direction)
    for chunk in range(n_chunks):
        if role == 0 and mid >= 1 and mid + chunk * K < n:
            resumes.append(mid + chunk * K - 1)
        if role == 1 and mid - 1 - chunk * K >= 0:
            resumes.append(mid - chunk * K)
    writers += chain.astype(np.int32)
    return writers, chain, resumes


def _check(lib, n, K):
    for role in (0, 1):
        for sparse2 in (True, False):
            writers, chain, resumes = _writers(lib, n, K, role, sparse2)
            assert (writers == 1).all(), (n, K, role, sparse2, np.flatnonzero(writers != 1)[:8].tolist())
            for c in resumes:
                assert 0 <= c < n and chain[c], (n, K, role, sparse2, c)   # the chain wrote this column — and, backward, its bsum


@pytest.mark.parametrize("K", [64, 96, 128, 8192])
def test_every_scale_entry_has_one_writer_and_every_resume_a_stored_column(lib, K):
    for n in list(range(1, 701)) + [1023, 1024, 1025, 16383, 16384, 16385, 16511, 16513]:
        _check(lib, n, K)


def test_the_whole_genome_chunk_size_over_several_chunks(lib):
    for n in (16383, 16384, 16385, 20001, 49153):
        _check(lib, n, 8192)
