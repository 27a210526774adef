"""The record lines over a slotted prefix through the unit entry point (pg_record_lines_from_text_slotted; the SLOT instantiation
of k_rlines_* of pangenie_amd/csrc/pg_record_lines.hip): arbitrary bytes in, the packed lines out, compared byte for byte with the plain
Python join
    prefix[r][:slot[r]] + str(uk[r]) + prefix[r][slot[r]:] + b"".join(b"\\t" + text_s[r] for s) + b"\\n"
(nothing, if a text_s[r] is empty).  The shapes are the kernels' seams: 1, 255, 256, 257 and 1025 records (a block of the scan
is 256 lines) times 1, 2 and 65 members (a wave takes 64, 64 and 4 lines; a step takes 64 pieces); UK at every number of
digits and at both ends of each; slots at 0, at the prefix's end and inside; empty prefixes; every residue mod 16 of a block's
first byte; a 70 000-byte prefix whose slot lies near its middle and at the last byte of a window of the 8 KB stage; 20 000-byte
member pieces; empty member pieces at the first, a middle and the last record of a block.  Without slots the bytes and offsets
are pg_record_lines_from_text's.  The join has no arithmetic: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib, calls
from pangenie_amd.hmm import PanGenieError

pytestmark = pytest.mark.gpu
SEED = 9800
GUARD = 64
STAGE = 8192
UK_EDGES = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]


def pieces(rng, R, lo, hi):
    """R random byte strings of lo .. hi bytes as (off, bytes): every byte value occurs, tabs, newlines and digits included"""
    return of_lengths(rng, rng.integers(lo, hi + 1, R))


def of_lengths(rng, lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return off, rng.integers(0, 256, int(off[-1]), dtype=np.uint8)


def piece(p, r):
    return p[1][int(p[0][r]):int(p[0][r + 1])].tobytes()


def lengths(p):
    return np.diff(p[0].astype(np.int64))


def uk_values(rng, R):
    """the edges of every number of digits first, random 16-bit values behind them, shuffled unless R is too small to hold all"""
    uk = np.concatenate([UK_EDGES, rng.integers(0, 65536, max(R, len(UK_EDGES)))])[:max(R, len(UK_EDGES))].astype(np.uint16)
    rng.shuffle(uk)
    return uk[:R].copy()


def slots_of(rng, prefix):
    """a third of the slots at 0, a third at the prefix's end, the others inside (or at an end of a prefix too short for it)"""
    plen = lengths(prefix)
    kind = rng.integers(0, 3, len(plen))
    inside = (rng.random(len(plen)) * (plen + 1)).astype(np.int64)
    return np.where(kind == 0, 0, np.where(kind == 1, plen, inside)).astype(np.uint32)


def expected(texts, prefix, slot, uk):
    R = len(prefix[0]) - 1
    lines = []
    for r in range(R):
        ts = [piece(t, r) for t in texts]
        p = piece(prefix, r)
        if slot is not None:
            p = p[:int(slot[r])] + str(int(uk[r])).encode() + p[int(slot[r]):]
        lines.append(b"" if any(len(t) == 0 for t in ts) else p + b"".join(b"\t" + t for t in ts) + b"\n")
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.uint64)
    return off, b"".join(lines)


def bound_of(texts, prefix, slot):
    R, S = len(prefix[0]) - 1, len(texts)
    f = calls.record_lines_bound if slot is None else calls.record_lines_bound_slotted
    return f(R, S, int(prefix[0][-1]), sum(int(t[0][-1]) for t in texts))


def raw(texts, prefix, slot, uk, out_off, out, cap):
    lib = _lib.load_hip()
    R, S = len(prefix[0]) - 1, len(texts)
    op = (C.c_void_p * S)(*[t[0].ctypes.data for t in texts])
    tp = (C.c_void_p * S)(*[t[1].ctypes.data if len(t[1]) else None for t in texts])
    return lib.pg_record_lines_from_text_slotted(0, R, S, op, tp, prefix[0].ctypes.data, prefix[1].ctypes.data if len(prefix[1]) else None,
                                                 None if slot is None else slot.ctypes.data, None if uk is None else uk.ctypes.data,
                                                 None if out_off is None else out_off.ctypes.data, out.ctypes.data, cap)


def run_guarded(texts, prefix, slot, uk):
    """the entry point with a guard behind the bound and behind the offsets: (off, the whole buffer, the bound)"""
    R = len(prefix[0]) - 1
    cap = bound_of(texts, prefix, slot)
    off = np.full(R + 1 + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
    out = np.full(cap + GUARD, 0xA5, np.uint8)
    assert raw(texts, prefix, slot, uk, off, out, cap) == 0
    assert (off[R + 1:] == 0xA5A5A5A5A5A5A5A5).all()           # nothing behind off[R]
    return off[:R + 1], out, cap


def check(texts, prefix, slot, uk, what):
    want_off, want = expected(texts, prefix, slot, uk)
    off, out, cap = run_guarded(texts, prefix, slot, uk)
    assert off.tolist() == want_off.tolist(), what
    n = int(off[-1])
    assert out[:n].tobytes() == want, what
    assert (out[n:] == 0xA5).all(), what                       # nothing behind the bytes, in the buffer or in the guard
    assert n <= cap, what
    return int((np.diff(want_off.astype(np.int64)) == 0).sum())


@pytest.mark.parametrize("S", [1, 2, 65])
def test_the_lines_are_the_join_with_the_number_at_the_slot(S):
    for R in (1, 255, 256, 257, 1025):
        rng = np.random.default_rng(SEED + 1000 * S + R)
        texts = [pieces(rng, R, 1, 40) for _ in range(S)]
        prefix = pieces(rng, R, 0, 40)
        assert check(texts, prefix, slots_of(rng, prefix), uk_values(rng, R), (R, S)) == 0


def test_every_number_of_digits_at_every_kind_of_slot():
    """one record per (UK edge, slot at 0 / inside / at the end), and a prefix of no bytes at all with the slot at 0"""
    rng = np.random.default_rng(SEED + 1)
    uk = np.repeat(np.array(UK_EDGES, np.uint16), 3)
    R = len(uk)
    prefix = of_lengths(rng, np.full(R, 11))
    slot = np.tile(np.array([0, 5, 11], np.uint32), len(UK_EDGES))
    texts =[pieces(np.random.default_rng(SEED + 2), R, 1, 9)]
    assert check(texts, prefix, slot, uk, "digits") == 0
    off, out, _ = run_guarded(texts, prefix, slot, uk)
    for r in range(R):   # the digits stand where the rule says, in plain sight
        digits = str(int(uk[r])).encode()
        at = int(off[r]) + int(slot[r])
        assert out[at:at + len(digits)].tobytes() == digits, r
    empty = (np.zeros(R + 1, np.uint64), np.zeros(0, np.uint8))
    assert check(texts, empty, np.zeros(R, np.uint32), uk, "no prefix bytes") == 0
    off, out, _ = run_guarded(texts, empty, np.zeros(R, np.uint32), uk)
    for r in range(R):   # the number, then the first member's tab
        digits = str(int(uk[r])).encode()
        assert out[int(off[r]):int(off[r]) + len(digits) + 1].tobytes() == digits + b"\t", r


def test_empty_prefixes_among_others():
    rng = np.random.default_rng(SEED + 3)
    R = 300
    plens = rng.integers(0, 3, R)
    plens[[0, 1, 255, 256, 299]] = 0
    for S in (1, 2):
        prefix = of_lengths(rng, plens)
        check([pieces(rng, R, 1, 40) for _ in range(S)], prefix, slots_of(rng, prefix), uk_values(rng, R), ("empty prefix", S))


def test_every_block_starts_at_every_residue():
    """16 runs, run k with a first line 1 + k bytes longer: the second and third block of the scan begin at every residue mod 16
    (the stage is laid out at it), whatever the other lengths add up to"""
    rng = np.random.default_rng(SEED + 4)
    R = 600
    lens = [rng.integers(1, 40, R) for _ in range(2)]
    plens = rng.integers(1, 40, R)
    uk = uk_values(rng, R)
    seen = [set(), set()]
    for k in range(16):
        plens[0] = 1 + k
        texts = [of_lengths(rng, l) for l in lens]
        prefix = of_lengths(rng, plens)
        slot = slots_of(rng, prefix)
        check(texts, prefix, slot, uk, ("residue", k))
        off = expected(texts, prefix, slot, uk)[0]
        seen[0].add(int(off[256]) % 16)
        seen[1].add(int(off[512]) % 16)
    assert seen[0] == set(range(16)) and seen[1] == set(range(16))


def test_a_prefix_longer_than_the_stage_with_the_slot_in_its_middle_and_at_a_windows_last_byte():
    """The long prefix is record 0: its line begins at byte 0 of the output, so the stage's windows end at the multiples of
    8192.  A slot at 5 * 8192 - 1 puts the first digit on a window's last byte, one at 5 * 8192 - 3 lets a 5-digit number
    straddle the seam, one at 5 * 8192 begins the next window with it; then the same with the long prefix elsewhere."""
    rng = np.random.default_rng(SEED + 5)
    R = 300
    for S in (1, 2):
        texts = [pieces(rng, R, 1, 40) for _ in range(S)]
        plens = rng.integers(1, 40, R)
        plens[0] = 70_000
        prefix = of_lengths(rng, plens)
        for at in (35_000, 5 * STAGE - 1, 5 * STAGE - 3, 5 * STAGE, 0, 70_000):
            slot = slots_of(rng, prefix)
            slot[0] = at
            uk = uk_values(rng, R)
            uk[0] = 54321
            check(texts, prefix, slot, uk, ("long prefix", S, at))
    for at in (100, 299):
        plens = rng.integers(1, 40, R)
        plens[at] = 70_000
        prefix = of_lengths(rng, plens)
        slot = slots_of(rng, prefix)
        slot[at] = 35_000
        check([pieces(rng, R, 1, 40)], prefix, slot, uk_values(rng, R), ("long prefix at", at))


def test_member_pieces_longer_than_the_stage_cross_windows():
    rng = np.random.default_rng(SEED + 6)
    R = 5
    texts = [of_lengths(rng, np.full(R, 20_000) + rng.integers(0, 17, R)) for _ in range(3)]
    prefix = pieces(rng, R, 1, 40)
    check(texts, prefix, slots_of(rng, prefix), uk_values(rng, R), "20 000-byte pieces")


@pytest.mark.parametrize("S", [1, 2, 65])
def test_an_empty_piece_leaves_the_line_to_the_host_and_nothing_else_changes(S):
    rng = np.random.default_rng(SEED + 7 + S)
    R = 600
    records = [0, 130, 255, 256, 400, 511, 512, 599]       # the first, a middle and the last record of a block
    members = sorted({0, S // 2, S - 1})                      # the first, a middle and the last member
    lens = [rng.integers(1, 40, R) for _ in range(S)]
    full = [of_lengths(np.random.default_rng(SEED + 50 + s), lens[s]) for s in range(S)]
    prefix = pieces(rng, R, 1, 40)
    slot, uk = slots_of(rng, prefix), uk_values(rng, R)
    assert check(full, prefix, slot, uk, ("full", S)) == 0
    full_off, full_bytes = expected(full, prefix, slot, uk)
    for i, r in enumerate(records):
        lens[members[i % len(members)]][r] = 0
    holed = []   # the same bytes everywhere else: a member's bytes are drawn piece by piece from the full ones
    for s in range(S):
        data = b"".join(piece(full[s], r)[:int(lens[s][r])] for r in range(R))
        holed.append((np.concatenate([[0], np.cumsum(lens[s])]).astype(np.uint64), np.frombuffer(data, np.uint8)))
    assert check(holed, prefix, slot, uk, ("holed", S)) == len(records)
    off, out, _ = run_guarded(holed, prefix, slot, uk)
    for r in range(R):
        got = out[int(off[r]):int(off[r + 1])].tobytes()
        assert got == (b"" if r in records else full_bytes[int(full_off[r]):int(full_off[r + 1])]), r


@pytest.mark.parametrize("S", [1, 2, 65])
def test_without_slots_the_lines_are_those_of_the_plain_kernels(S):
    for R in (1, 257, 1025):
        rng = np.random.default_rng(SEED + 100 * S + R)
        texts = [pieces(rng, R, 0 if R > 1 else 1, 40) for _ in range(S)]
        prefix = pieces(rng, R, 0, 40)
        want_off, want = calls.record_lines_from_text(texts, prefix)
        got_off, got = calls.record_lines_from_text_slotted(texts, prefix)
        assert got_off.tolist() == want_off.tolist() and got == want
        assert check(texts, prefix, None, None, ("plain", R, S)) == int((np.diff(want_off.astype(np.int64)) == 0).sum())
        off, out, cap = run_guarded(texts, prefix, None, None)
        assert cap == calls.record_lines_bound(R, S, int(prefix[0][-1]), sum(int(t[0][-1]) for t in texts))
    long_prefix = of_lengths(rng, np.array([3, 70_000, 5]))
    texts = [pieces(rng, 3, 1, 40) for _ in range(S)]
    assert calls.record_lines_from_text_slotted(texts, long_prefix)[1] == calls.record_lines_from_text(texts, long_prefix)[1]


def test_the_wrapper_gives_the_same_lines():
    rng = np.random.default_rng(SEED + 8)
    R = 300
    texts = [pieces(rng, R, 1, 40) for _ in range(2)]
    prefix = pieces(rng, R, 0, 40)
    slot, uk = slots_of(rng, prefix), uk_values(rng, R)
    want_off, want = expected(texts, prefix, slot, uk)
    off, got = calls.record_lines_from_text_slotted(texts, prefix, slot, uk)
    assert off.tolist() == want_off.tolist() and got == want


def test_the_refusals():
    rng = np.random.default_rng(SEED + 9)
    R = 4
    texts = [pieces(rng, R, 1, 9) for _ in range(2)]
    prefix = of_lengths(rng, np.array([3, 0, 5, 2]))
    slot, uk = np.array([3, 0, 2, 1], np.uint32), np.array([7, 65535, 0, 10], np.uint16)
    cap = bound_of(texts, prefix, slot)
    assert cap == calls.record_lines_bound(R, 2, 10, sum(int(t[0][-1]) for t in texts)) + 5 * R
    off, out = np.zeros(R + 1, np.uint64), np.full(cap + GUARD, 0xA5, np.uint8)
    INV = _lib.PG_ERR_INVALID
    assert raw(texts, prefix, slot, uk, off, out, cap) == 0
    for r in range(R):   # a slot beyond its prefix, by one and by far
        for beyond in (1, 1 << 31):
            bad = slot.copy()
            bad[r] = int(lengths(prefix)[r]) + beyond
            assert raw(texts, prefix, bad, uk, off, out, cap) == INV
    assert raw(texts, prefix, slot, None, off, out, cap) == INV                       # slots without UK values
    assert raw(texts, prefix, slot, uk, off, out, cap - 1) == INV                     # below the slotted bound ...
    assert raw(texts, prefix, slot, uk, off, out, cap - 5 * R) == INV                 # ... the plain bound is not enough
    assert raw(texts, prefix, None, None, off, out, cap - 5 * R) == 0                 # ... unless there are no slots
    assert raw(texts, prefix, None, None, off, out, cap - 5 * R - 1) == INV
    assert raw(texts, prefix, slot, uk, None, out, cap) == INV
    shrinking = (np.array([0, 3, 2, 8, 10], np.uint64), prefix[1])
    assert raw(texts, shrinking, np.zeros(R, np.uint32), uk, off, out, cap) == INV
    not_at_0 = (prefix[0] + np.uint64(1), np.concatenate([prefix[1], prefix[1][:1]]))
    assert raw(texts, not_at_0, slot, uk, off, out, cap) == INV
    bad_text = [(texts[0][0][::-1].copy(), texts[0][1]), texts[1]]
    assert raw(bad_text, prefix, slot, uk, off, out, cap) == INV
    lib = _lib.load_hip()
    assert lib.pg_record_lines_from_text_slotted(0, R, 0, None, None, prefix[0].ctypes.data, prefix[1].ctypes.data, slot.ctypes.data, uk.ctypes.data,
                                                 off.ctypes.data, out.ctypes.data, cap) == INV
    with pytest.raises(ValueError):
        calls.record_lines_from_text_slotted(texts, prefix, slot)                     # the wrapper: slots without UK values
    with pytest.raises(ValueError):
        calls.record_lines_from_text_slotted(texts, prefix, slot[:-1], uk)
    bad = slot.copy()
    bad[2] = 6
    with pytest.raises(PanGenieError) as e:
        calls.record_lines_from_text_slotted(texts, prefix, bad, uk)
    assert e.value.code == INV
