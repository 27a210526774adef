"""The preparation in parts of a job that runs phase 1 in pieces (pangenie_amd/csrc/pg_device.h: pg_prep_middle,
pg_prep_middle_variants, pg_prep_part_item; include/pangenie_hmm.h: pg_prep_parts, pg_prep_part_member), on the host.  The MIDDLE of a
chain is one band of W = (n_pieces - E) piece_cols columns to either side of the phase boundary, the ENDS are the rest; the ends are
prepared ahead of phase 1, the middle on the second stream beside the first E pieces.  For every column count, chunk size, G and E:
ends and middle partition the columns, every column of the pieces >= n_pieces - E of either role lies in the ends and every column of
a lower piece in the middle, the variant rule puts every variant into exactly one part — that of its column, or of the next column
below it —, and the kernels' mapping of their threads onto a part reaches every item of the part exactly once.  No device involved."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib, build

S = 64
EXHAUSTIVE = {1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 130, 254, 255, 256, 257, 385, 675, 700}   # column counts whose parts are enumerated item by item


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_hip()


def _n_pieces(n, K, G):
    n_chunks = (n // 2 + 1 + K - 1) // K     # what a job of this one chain has (tests/test_sparse_pieces.py)
    return (n_chunks + G - 1) // G


def _column_list(n, rng):
    """n kept variants among V, ascending: variants that are no column in front of the first column, between columns and behind the last"""
    V = n + n // 3 + 5
    colv = np.sort(rng.choice(V, size=n, replace=False)).astype(np.uint32)
    return V, colv


def _members(lib, part, lo, hi, n):
    out = []
    for u in range(n + 2):
        m = lib.pg_prep_part_member(part, lo, hi, n, u)
        if m == n:
            assert all(lib.pg_prep_part_member(part, lo, hi, n, w) == n for w in (u + 1, n, n + 1, 0xFFFFFFFF))   # (no item behind the part's last)
            break
        out.append(m)
    return out


def _check(lib, n, K, G, rng, exhaustive):
    n_pieces = _n_pieces(n, K, G)
    mid = n // 2
    cols, var = (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
    piece = (C.c_uint32 * 2)()
    V, colv = _column_list(n, rng)
    colv_p = colv.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.pg_prep_parts(n, K, G, n_pieces, n_pieces, colv_p, V, cols, var) == 0      # no piece left behind the early ones
    assert lib.pg_prep_parts(n, K, G, n_pieces, n_pieces + 1, colv_p, V, cols, var) == 0
    pieces = []   # (role, g, lowest, highest column): they do not hang on E
    for role in (0, 1):
        for g in range(n_pieces):
            rc = lib.pg_sparse_piece_range(n, K, G, g, role, piece)
            assert rc in (0, 1)
            if rc:
                pieces.append((role, g, int(piece[0]), int(piece[1])))
    seen = np.zeros(n, dtype=np.int32)
    for (_, _, plo, phi) in pieces:
        seen[plo:phi + 1] += 1
    assert (seen == 1).all()   # (the pieces of the two roles are all the columns: ends and middle partition them)
    col_of_variant = np.maximum(np.searchsorted(colv, np.arange(V), side="right") - 1, 0)
    # every E; a whole chromosome in 64-column chunks has thousands of pieces: the E next to either end and some between
    early = range(1, n_pieces) if n_pieces <= 64 else sorted({1, 2, 3, n_pieces // 3, n_pieces // 2, n_pieces - 3, n_pieces - 2, n_pieces - 1})
    for E in early:
        assert lib.pg_prep_parts(n, K, G, n_pieces, E, colv_p, V, cols, var) == 1
        lo, hi = int(cols[0]), int(cols[1])
        W = (n_pieces - E) * G * K
        assert (lo, hi) == (mid - min(mid, W), mid + min(n - mid, W))
        assert 0 <= lo <= mid <= hi <= n
        in_middle = np.zeros(n, dtype=bool)
        in_middle[lo:hi] = True
        # ---- every column of a piece >= n_pieces - E lies in the ends, every column of a lower piece in the middle
        for (role, g, plo, phi) in pieces:
            if g >= n_pieces - E:
                assert not in_middle[plo:phi + 1].any(), (n, K, G, E, role, g)
            else:
                assert in_middle[plo:phi + 1].all(), (n, K, G, E, role, g)
        # ---- the variant rule: a variant goes with its column, one that is no column with the next column below it (column 0 at the least)
        vlo, vhi = int(var[0]), int(var[1])
        assert 0 <= vlo <= vhi <= V
        want = in_middle[col_of_variant]
        got = np.zeros(V, dtype=bool)
        got[vlo:vhi] = True
        assert np.array_equal(got, want), (n, K, G, E)
        assert np.array_equal(got[colv], in_middle)   # (a column's variant is in the column's part)
        # ---- the kernels' mapping: items 0 .. of a part, each exactly once, below the middle first
        for (a, b, N) in ((lo, hi, n), (vlo, vhi, V)):
            n1, n2 = N - (b - a), b - a
            if exhaustive:
                assert _members(lib, 2, a, b, N) == list(range(a, b))
                assert _members(lib, 1, a, b, N) == list(range(0, a)) + list(range(b, N))
            else:
                for u, m in ((0, a if n2 else N), (n2 - 1, b - 1 if n2 else N), (n2, N), (0xFFFFFFFF, N)):
                    assert lib.pg_prep_part_member(2, a, b, N, u & 0xFFFFFFFF) == m
                first1 = (0 if a else b) if n1 else N
                for u, m in ((0, first1), (a - 1, a - 1 if a else N), (a, b if b < N else N), (n1 - 1, (N - 1 if b < N else a - 1) if n1 else N), (n1, N)):
                    assert lib.pg_prep_part_member(1, a, b, N, u & 0xFFFFFFFF) == m, (N, a, b, u)
    # (without a column list: the columns alone)
    if n_pieces > 1:
        assert lib.pg_prep_parts(n, K, G, n_pieces, 1, None, V, cols, None) == 1


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("K", [64, 128, 8192])
def test_ends_and_middle_partition_columns_and_variants(lib, K, G):
    rng = np.random.default_rng(1000 * K + G)
    for n in list(range(1, 701)) + [1023, 1024, 1025, 16385, 49153, 397000, 397001]:
        _check(lib, n, K, G, rng, exhaustive=n in EXHAUSTIVE)


def test_the_675_column_chain_at_64_by_1(lib):
    """What tests/test_prep_beside_gpu.py relies on: six pieces; at the default E = 2 the ends are 81 and 82 columns (roles 0 and 1),
    and every shorter chain of that job is all middle."""
    cols = (C.c_uint32 * 2)()
    assert _n_pieces(675, 64, 1) == 6
    assert lib.pg_prep_parts(675, 64, 1, 6, 2, None, 675, cols, None) == 1
    assert (int(cols[0]), 675 - int(cols[1])) == (81, 82)
    for n in (1, 2, 3, 127, 128, 129, 254):
        assert lib.pg_prep_parts(n, 64, 1, 6, 2, None, n, cols, None) == 1
        assert (int(cols[0]), int(cols[1])) == (0, n)


def test_a_chain_without_columns_is_all_middle(lib):
    cols, var = (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
    assert lib.pg_prep_parts(0, 64, 1, 6, 2, None, 17, cols, var) == 1
    assert (int(cols[0]), int(cols[1]), int(var[0]), int(var[1])) == (0, 0, 0, 17)


def test_arguments_outside_the_scheme(lib):
    cols, var = (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
    colv = np.arange(1000, dtype=np.uint32)
    p = colv.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.pg_prep_parts(1000, 96, 1, 6, 2, p, 1000, cols, var) == -1     # chunk size no multiple of 64: no pieces
    assert lib.pg_prep_parts(1000, 0, 1, 6, 2, p, 1000, cols, var) == -1
    assert lib.pg_prep_parts(1000, 64, 0, 6, 2, p, 1000, cols, var) == -1
    assert lib.pg_prep_parts(1000, 1 << 31, 2, 6, 2, p, 1000, cols, var) == -1   # a piece wider than 32 bits hold
    assert lib.pg_prep_parts(1000, 64, 1, 6, 0, p, 1000, cols, var) == -1      # no early piece
    assert lib.pg_prep_parts(1000, 64, 1, 0, 1, p, 1000, cols, var) == -1
    assert lib.pg_prep_parts(1000, 64, 1, 6, 2, p, 999, cols, var) == -1       # more columns than variants
    assert lib.pg_prep_parts(1000, 64, 1, 6, 2, None, 1000, cols, var) == -1   # variants asked for without a column list
    assert lib.pg_prep_parts(1000, 64, 1, 6, 2, None, 1000, None, None) == 1
    assert lib.pg_prep_parts(1000, 64, 1, 2, 2, p, 1000, cols, var) == 0
    # a band wider than 32 bits hold: the whole chain is middle
    assert lib.pg_prep_parts(0xFFFFFFFF, 1 << 30, 2, 3, 1, None, 0xFFFFFFFF, cols, None) == 1
    assert (int(cols[0]), int(cols[1])) == (0, 0xFFFFFFFF)
    # a long chain: the arithmetic stays inside 32 bits' reach
    assert lib.pg_prep_parts(0xFFFFFFFF, 8192, 4, 0x10000, 1, None, 0xFFFFFFFF, cols, None) == 1
    assert (int(cols[0]), int(cols[1])) == (32767, 0xFFFFFFFF - 32768)
    assert lib.pg_prep_parts(0xFFFFFFFF, 8192, 4, 0x10000, 0xFFFF, None, 0xFFFFFFFF, cols, None) == 1
    assert (int(cols[0]), int(cols[1])) == (0x7FFFFFFF - 32768, 0x7FFFFFFF + 32768)
    assert lib.pg_prep_part_member(0, 2, 5, 9, 0) == 9 and lib.pg_prep_part_member(3, 2, 5, 9, 0) == 9
    assert lib.pg_prep_part_member(1, 5, 2, 9, 0) == 9 and lib.pg_prep_part_member(1, 2, 10, 9, 0) == 9
