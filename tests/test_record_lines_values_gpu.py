"""The record lines through the unit entry point (pg_record_lines_from_text; k_rlines_* of pangenie_amd/csrc/pg_record_lines.hip):
arbitrary bytes in, the packed lines out, compared byte for byte with the plain Python join
    prefix[r] + b"".join(b"\\t" + text_s[r] for s) + b"\\n"          (nothing, if a text_s[r] is empty).
The shapes are the kernels' seams: 1, 255, 256, 257 and 1025 records (a block of the scan is 256 lines) times 1, 2, 3, 64, 65
and 130 members (the lines a wave takes go 64, 64, 32, 2, 2, 1, and a step takes 64 pieces); every residue mod 16 of a block's
first byte; empty prefixes; a prefix and pieces longer than the 8 KB stage; a line of 1500 short pieces; empty pieces at the
first, a middle and the last record of a block and member.  The join has no arithmetic: no tolerance anywhere."""
import numpy as np
import pytest

from pangenie_amd import _lib, calls

pytestmark = pytest.mark.gpu
SEED = 9400
GUARD = 64


def pieces(rng, R, lo, hi):
    """R random byte strings of lo .. hi bytes as (off, bytes): every byte value occurs, tabs and newlines included"""
    lens = rng.integers(lo, hi + 1, R)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return off, rng.integers(0, 256, int(off[-1]), dtype=np.uint8)


def of_lengths(rng, lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return off, rng.integers(0, 256, int(off[-1]), dtype=np.uint8)


def piece(p, r):
    return p[1][int(p[0][r]):int(p[0][r + 1])].tobytes()


def expected(texts, prefix):
    R = len(prefix[0]) - 1
    lines = []
    for r in range(R):
        ts = [piece(t, r) for t in texts]
        lines.append(b"" if any(len(t) == 0 for t in ts) else piece(prefix, r) + b"".join(b"\t" + t for t in ts) + b"\n")
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.uint64)
    return off, b"".join(lines)


def run_guarded(texts, prefix):
    """the entry point with a guard behind the bound: (off, the whole buffer, the bound)"""
    lib = _lib.load_hip()
    import ctypes as C
    R, S = len(prefix[0]) - 1, len(texts)
    cap = calls.record_lines_bound(R, S, int(prefix[0][-1]), sum(int(t[0][-1]) for t in texts))
    op = (C.c_void_p * S)(*[t[0].ctypes.data for t in texts])
    tp = (C.c_void_p * S)(*[t[1].ctypes.data if len(t[1]) else None for t in texts])
    off = np.zeros(R + 1, np.uint64)
    out = np.full(cap + GUARD, 0xA5, np.uint8)
    rc = lib.pg_record_lines_from_text(0, R, S, op, tp, prefix[0].ctypes.data, prefix[1].ctypes.data if len(prefix[1]) else None, off.ctypes.data,
                                       out.ctypes.data, cap)
    assert rc == 0, rc
    return off, out, cap


def check(texts, prefix, what):
    want_off, want = expected(texts, prefix)
    off, out, cap = run_guarded(texts, prefix)
    assert off.tolist() == want_off.tolist(), what
    n = int(off[-1])
    assert out[:n].tobytes() == want, what
    assert (out[n:] == 0xA5).all(), what                       # nothing behind off[R], in the buffer or in the guard
    hosts = int((np.diff(want_off.astype(np.int64)) == 0).sum())
    assert (n == cap) == (hosts == 0), what                    # the bound is reached exactly when no line is the host's
    return hosts


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 130])
def test_the_lines_are_the_join(S):
    for R in (1, 255, 256, 257, 1025):
        rng = np.random.default_rng(SEED + 1000 * S + R)
        texts = [pieces(rng, R, 1, 40) for _ in range(S)]
        assert check(texts, pieces(rng, R, 1, 40), (R, S)) == 0


def test_every_block_starts_at_every_residue():
    """16 runs, run k with a first line 1 + k bytes longer: the second and third block of the scan begin at every residue mod 16
    (the stage is laid out at it), whatever the other lengths add up to"""
    rng = np.random.default_rng(SEED + 1)
    R = 600
    lens = [rng.integers(1, 40, R) for _ in range(3)]
    plens = rng.integers(1, 40, R)
    seen = [set(), set()]
    for k in range(16):
        plens[0] = 1 + k
        texts = [of_lengths(rng, l) for l in lens[:2]]
        prefix = of_lengths(rng, plens)
        check(texts, prefix, ("residue", k))
        off = expected(texts, prefix)[0]
        seen[0].add(int(off[256]) % 16)
        seen[1].add(int(off[512]) % 16)
    assert seen[0] == set(range(16)) and seen[1] == set(range(16))


def test_empty_prefixes_begin_with_a_tab():
    rng = np.random.default_rng(SEED + 2)
    R = 300
    plens = rng.integers(0, 3, R)
    plens[[0, 1, 255, 256, 299]] = 0
    for S in (1, 3):
        texts = [pieces(rng, R, 1, 40) for _ in range(S)]
        prefix = of_lengths(rng, plens)
        check(texts, prefix, ("empty prefix", S))
        off, out, _ = run_guarded(texts, prefix)
        assert all(out[int(off[r])] == 9 for r in (0, 1, 255, 256, 299))
    empty = (np.zeros(R + 1, np.uint64), np.zeros(0, np.uint8))   # no prefix byte at all
    check([pieces(rng, R, 1, 40)], empty, "no prefix bytes")


def test_a_prefix_longer_than_the_stage():
    rng = np.random.default_rng(SEED + 3)
    for at in (0, 100, 299):
        plens = rng.integers(1, 40, 300)
        plens[at] = 70_000
        for S in (1, 3):
            check([pieces(rng, 300, 1, 40) for _ in range(S)], of_lengths(rng, plens), ("long prefix", at, S))


def test_pieces_longer_than_the_stage_cross_windows():
    rng = np.random.default_rng(SEED + 4)
    R = 5
    texts = [of_lengths(rng, np.full(R, 20_000) + rng.integers(0, 17, R)) for _ in range(3)]
    check(texts, pieces(rng, R, 1, 40), "20 000-byte pieces")


def test_a_line_of_1500_pieces():
    rng = np.random.default_rng(SEED + 5)
    R = 3
    texts = [of_lengths(rng, np.full(R, 30)) for _ in range(1500)]
    check(texts, pieces(rng, R, 1, 40), "1500 members")


@pytest.mark.parametrize("S", [1, 3, 65])
def test_an_empty_piece_leaves_the_line_to_the_host_and_nothing_else_changes(S):
    rng = np.random.default_rng(SEED + 6 + S)
    R = 600
    records = [0, 130, 255, 256, 400, 511, 512, 599]       # the first, a middle and the last record of a block
    members = sorted({0, S // 2, S - 1})                      # the first, a middle and the last member
    lens = [rng.integers(1, 40, R) for _ in range(S)]
    plens = rng.integers(1, 40, R)
    full = [of_lengths(np.random.default_rng(SEED + 50 + s), lens[s]) for s in range(S)]
    prefix = of_lengths(np.random.default_rng(SEED + 49), plens)
    assert check(full, prefix, ("full", S)) == 0
    full_off, full_bytes = expected(full, prefix)
    for i, r in enumerate(records):
        lens[members[i % len(members)]][r] = 0
    # the same bytes everywhere else: a member's bytes are drawn piece by piece from the full ones
    holed = []
    for s in range(S):
        data = b"".join(piece(full[s], r)[:int(lens[s][r])] for r in range(R))
        holed.append((np.concatenate([[0], np.cumsum(lens[s])]).astype(np.uint64), np.frombuffer(data, np.uint8)))
    assert check(holed, prefix, ("holed", S)) == len(records)
    off, out, _ = run_guarded(holed, prefix)
    for r in range(R):
        got = out[int(off[r]):int(off[r + 1])].tobytes()
        assert got == (b"" if r in records else full_bytes[int(full_off[r]):int(full_off[r + 1])]), r
