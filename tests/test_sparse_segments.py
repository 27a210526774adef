"""The arithmetic of the sparse phase 1 (pangenie_amd/csrc/pg_device.h: pg_sparse_*; include/pangenie_hmm.h: pg_sparse_segment),
on the host: which columns a lean chain stores itself, which segment of which chunk re-runs the others.  For every column count
and chunk size: a column of a role's phase-1 half is either stored by the chain or written by exactly one refill segment, the
segment lies in the partner range of the chunk that k_post reads it in, it resumes from a column the chain stored, and it runs
63 columns in the role's own direction.  No device involved."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib, build

S = 64


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_hip()


def _stored(lib, n, role):
    return np.array([lib.pg_sparse_stored_by_chain(n, role, c) for c in range(n)], dtype=bool)


def _check(lib, n, K):
    mid = n // 2
    q = K // S
    out = (C.c_uint32 * 3)()
    n_chunks = (max(mid, n - mid) + K - 1) // K + 1   # (one more than any half needs: it must be empty)
    for role in (0, 1):
        half = np.zeros(n, dtype=bool)
        if role == 0:
            half[:mid] = True
        else:
            half[mid:] = True
        stored = _stored(lib, n, role)
        # the column phase 2 resumes from, the column the recursion starts at, and every 64th from the phase boundary
        if role == 0 and mid:
            assert stored[mid - 1] and stored[0]
            want = {mid - 1 - m * S for m in range(mid) if mid - 1 - m * S >= 0}
        elif role == 1 and n:
            assert stored[mid] and stored[n - 1]
            want = {mid + m * S for m in range(n) if mid + m * S < n}
        else:
            want = set()
        assert all(stored[c] for c in want)
        written = np.zeros(n, dtype=np.int32)
        for chunk in range(n_chunks):
            # the partner range of this chunk: what k_post(chunk) reads of this role's phase-1 columns
            if role == 0:
                top = mid - 1 - chunk * K
                lo_r, hi_r = max(top - K + 1, 0), top
            else:
                lo_r, hi_r = mid + chunk * K, min(mid + (chunk + 1) * K, n) - 1
            for j in range(q):
                rc = lib.pg_sparse_segment(n, K, chunk, role, j, out)
                assert rc in (0, 1)
                if rc == 0:
                    continue
                ck, lo, hi = int(out[0]), int(out[1]), int(out[2])
                assert hi - lo + 1 == S - 1
                assert lo_r <= lo and hi <= hi_r, (n, K, role, chunk, j)
                assert ck == (lo - 1 if role == 0 else hi + 1) and ck in want
                assert half[lo:hi + 1].all() and not stored[lo:hi + 1].any()
                written[lo:hi + 1] += 1
        cover = written + stored.astype(np.int32)
        assert (cover[half] == 1).all(), (n, K, role)
        assert (written[~half] == 0).all()
        # the chain's own columns besides the checkpoints: only the leading piece, shorter than a segment
        extra = stored & half
        extra[list(want)] = False
        assert extra.sum() < S
        if extra.any():
            idx = np.flatnonzero(extra)
            assert (np.diff(idx) == 1).all() and (idx[0] == 0 if role == 0 else idx[-1] == n - 1)


@pytest.mark.parametrize("K", [64, 128, 8192])
def test_every_column_is_stored_or_refilled_exactly_once(lib, K):
    for n in list(range(0, 700)) + [1000, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 4095, 4096, 4097, 16383, 16384, 16385, 16511, 16513, 20001]:
        _check(lib, n, K)


def test_arguments_outside_the_scheme(lib):
    out = (C.c_uint32 * 3)()
    assert lib.pg_sparse_segment(1000, 96, 0, 0, 0, out) == -1    # chunk size no multiple of 64: such jobs keep the dense phase 1
    assert lib.pg_sparse_segment(1000, 0, 0, 0, 0, out) == -1
    assert lib.pg_sparse_segment(1000, 64, 0, 2, 0, out) == -1
    assert lib.pg_sparse_segment(1000, 128, 0, 0, 2, out) == -1   # two segments per chunk and role at 128 columns
    assert lib.pg_sparse_segment(1000, 64, 0, 0, 0, None) == 1
    assert lib.pg_sparse_stored_by_chain(10, 0, 10) == 0 and lib.pg_sparse_stored_by_chain(10, 2, 1) == 0
