"""The arithmetic of the sparse phase 2 (pangenie_amd/csrc/pg_device.h: pg_sparse2_*; include/pangenie_hmm.h:
pg_sparse_chunk_segment), on the host: which columns of its phase-2 half a lean chain stores itself (the checkpoints, into an area
of its own), and which segment of which chunk forms the columns k_post reads from the scratch buffers.  For every column count and
chunk size: every phase-2 column of either role is written by exactly one segment of exactly one chunk — the chunk k_post reads it
in — or, in a chain of a single column, stored by the chain; a segment resumes from the checkpoint directly in front of it (in the
role's own direction), which the chain stored or which is phase 1's last column; it runs at most 64 columns and ends on the next
checkpoint unless the half ends first; every chunk's last column is a checkpoint unless the half ends there.  No device involved."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib, build

S = 64


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_hip()


def _check(lib, n, K):
    mid = n // 2
    q = K // S
    out = (C.c_uint32 * 3)()
    n_chunks = (max(mid, n - mid) + K - 1) // K + 1   # (one more than any half needs: it must be empty)
    for role in (0, 1):
        half = np.zeros(n, dtype=bool)
        if role == 0:
            half[mid:] = True
        else:
            half[:mid] = True
        stored = np.array([lib.pg_sparse_chunk_stored_by_chain(n, role, c) for c in range(n)], dtype=bool)
        assert not stored[~half].any()
        # every 64th column from the phase boundary on, and no other
        if n < 2:
            want = set()
        elif role == 0:
            want = {mid - 1 + m * S for m in range(1, n) if mid - 1 + m * S < n}
        else:
            want = {mid - m * S for m in range(1, n) if mid - m * S >= 0}
        assert set(np.flatnonzero(stored).tolist()) == want, (n, role)
        first_ck = (mid - 1 if role == 0 else mid) if n >= 2 else None   # phase 1's last column: stored by phase 1
        written = np.zeros(n, dtype=np.int32)
        for chunk in range(n_chunks):
            # the columns of this chunk: what k_post(chunk) reads from the scratch buffer
            if role == 0:
                lo_c, hi_c = mid + chunk * K, min(mid + (chunk + 1) * K, n) - 1
            else:
                hi_c = mid - 1 - chunk * K
                lo_c = max(hi_c - K + 1, 0)
            if lo_c <= hi_c and hi_c - lo_c + 1 == K:
                assert stored[hi_c if role == 0 else lo_c], (n, K, role, chunk)   # the next chunk launch resumes from it
            for j in range(q):
                rc = lib.pg_sparse_chunk_segment(n, K, chunk, role, j, out)
                assert rc in (0, 1)
                if rc == 0:
                    continue
                ck, lo, hi = int(out[0]), int(out[1]), int(out[2])
                assert 1 <= hi - lo + 1 <= S
                assert lo_c <= lo and hi <= hi_c, (n, K, role, chunk, j)
                assert ck == (lo - 1 if role == 0 else hi + 1)        # the checkpoint precedes the segment ...
                assert ck == first_ck or stored[ck]                   # ... and is a column that was stored
                assert half[lo:hi + 1].all()
                last = hi if role == 0 else lo
                if hi - lo + 1 == S:
                    assert stored[last]                               # it delivers its closing checkpoint
                else:
                    assert last == (n - 1 if role == 0 else 0)        # the ragged piece at the end of the half
                assert not stored[lo:hi + 1].any() or np.flatnonzero(stored[lo:hi + 1]).tolist() == [last - lo]
                written[lo:hi + 1] += 1
        if n == 1 and role == 0:
            assert written.sum() == 0   # (the single column is the recursion's initial one: the chain stores it as ever)
        else:
            assert (written[half] == 1).all(), (n, K, role)
        assert (written[~half] == 0).all()


@pytest.mark.parametrize("K", [64, 128, 192])
def test_every_phase2_column_is_written_by_exactly_one_segment(lib, K):
    for n in list(range(0, 420)) + [1000, 1023, 1024, 1025, 16383, 16384, 16385, 16511, 16513]:
        _check(lib, n, K)


def test_whole_genome_chunk_size(lib):
    for n in (1, 2, 8191, 16384, 16385, 16511, 16513, 20001, 49153):
        _check(lib, n, 8192)


def test_arguments_outside_the_scheme(lib):
    out = (C.c_uint32 * 3)()
    assert lib.pg_sparse_chunk_segment(1000, 96, 0, 0, 0, out) == -1    # chunk size no multiple of 64: such jobs keep the dense phase 2
    assert lib.pg_sparse_chunk_segment(1000, 0, 0, 0, 0, out) == -1
    assert lib.pg_sparse_chunk_segment(1000, 64, 0, 2, 0, out) == -1
    assert lib.pg_sparse_chunk_segment(1000, 128, 0, 0, 2, out) == -1   # two segments per chunk and role at 128 columns
    assert lib.pg_sparse_chunk_segment(1000, 64, 0, 0, 0, None) == 1
    assert lib.pg_sparse_chunk_segment(1, 64, 0, 0, 0, out) == 0 and lib.pg_sparse_chunk_segment(0, 64, 0, 1, 0, out) == 0
    assert lib.pg_sparse_chunk_stored_by_chain(10, 0, 10) == 0 and lib.pg_sparse_chunk_stored_by_chain(10, 2, 1) == 0
    # a long chain: the arithmetic stays inside 32 bits' reach
    assert lib.pg_sparse_chunk_segment(0xFFFFFFFF, 8192, 0x3FFFF, 0, 127, out) == 1   # checkpoint mid - 1 + 64 (2^25 - 1)
    assert (int(out[0]), int(out[1]), int(out[2])) == (0xFFFFFFBE, 0xFFFFFFBF, 0xFFFFFFFE)
    assert lib.pg_sparse_chunk_segment(0xFFFFFFFF, 8192, 0x40000, 0, 0, out) == 0      # behind the last column
