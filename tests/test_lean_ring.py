"""The record ring of the sparse lean launches (pangenie_amd/csrc/pg_device.h: pg_lean_ring_first, pg_lean_ring_lead,
pg_lean_ring_launch; include/pangenie_hmm.h: pg_lean_ring_schedule), on the host.  A launch reads its column records out of an
LDS ring of two blocks of 64; step number n reads records n + 1 and n + 2 (the forward role n + 2 alone), a block is parked four
records ahead of its first read and expanded a step later.  A sparse launch numbers its steps from the grid of its 64-step
groups, so that a group parks and expands at two fixed steps and its other steps carry no upkeep at all; the steps in front of the
first group and behind the last one test their number, as every step of a dense launch and of a refill segment does.

The test walks every launch form through the exported schedule and keeps the ring's books step by step: what is read was parked
and expanded at earlier steps, nothing is overwritten while a step still reads it, and the fixed steps are where the tested rule
would put them, in every group."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib

S = 64            # PG_LEAN_SPARSE == PG_LEAN_BLOCK
SMALL = list(range(1, 701)) + [1023, 1024, 1025, 16385]
LARGE = [397000, 397001]
CHUNKS = (64, 128, 8192)
PIECE_CHUNKS = (1, 2, 4)


@pytest.fixture(scope="module")
def lib():
    return _lib.load_hip()


def _schedule(lib, n, K, G, role, form, arg):
    out = (C.c_uint32 * 6)()
    rc = lib.pg_lean_ring_schedule(n, K, G, role, form, arg, out)
    assert rc in (0, 1), (n, K, G, role, form, arg, rc)
    return tuple(int(x) for x in out) if rc else None


def _launches(lib, n, K, role):
    """every sparse launch of a chain of n columns at chunk size K: (what, schedule)"""
    s = _schedule(lib, n, K, 1, role, 0, 0)
    if s:
        yield "single", s
    for G in PIECE_CHUNKS:     # (piece g lies g G K columns from the phase boundary: none that far out has a step)
        for g in range(n // (G * K) + 1):
            s = _schedule(lib, n, K, G, role, 1, g)
            if s:
                yield f"piece {g} of {G}", s
    for q in range(n // K + 1):
        s = _schedule(lib, n, K, 1, role, 2, q)
        if s:
            yield f"chunk {q}", s


def _kinds(steps, lead, s0, park, expand):
    """per step: 0 none, 1 park, 2 expand — the leading steps and the tail by their number, the groups by their place"""
    i = np.arange(steps, dtype=np.int64)
    n = s0 + i
    tested = np.where((n + 4) % S == 0, 1, np.where((n + 3) % S == 0, 2, 0))
    groups = (steps - lead) // S if steps > lead else 0
    in_group = (i >= lead) & (i < lead + groups * S)
    j = (i - lead) % S
    fixed = np.where(j == park, 1, np.where(j == expand, 2, 0))
    return n, np.where(in_group, fixed, tested), in_group, tested


def _check_arithmetic(what, sched):
    """the whole launch at once: the groups begin on the grid, the fixed steps are the tested rule's, and every block from the
    first one the launch does not open with is parked at number 64 b - 4 and expanded at 64 b - 3"""
    c0, steps, lead, s0, park, expand = sched
    assert steps >= 1 and lead < S and s0 < S and (s0 + lead) % S == 0, (what, sched)
    assert (park, expand) == (S - 4, S - 3), (what, sched)
    n, kind, in_group, tested = _kinds(steps, lead, s0, park, expand)
    assert np.array_equal(kind, tested), (what, sched)               # the same positions in every group, and the rule's own
    assert np.all(n[in_group][::S] % S == 0)
    last = s0 + steps - 1
    want_park = np.arange(1, (last + 4) // S + 1) * S - 4       # (a first number behind 60: block 1 is the opening's, see _walk)
    want_expand = np.arange(1, (last + 3) // S + 1) * S - 3
    assert np.array_equal(n[kind == 1], want_park[want_park >= s0]), (what, sched)
    assert np.array_equal(n[kind == 2], want_expand[want_expand >= s0]), (what, sched)


def _walk(what, sched, role):
    """the ring's books, step by step.  A slot holds (block, number of the step that parked it, ... that expanded it); the launch
    opens with block 0 — and block 1 where its first number lies behind the parking step — parked and expanded ahead of every step"""
    c0, steps, lead, s0, park, expand = sched
    n_arr, kind, _, _ = _kinds(steps, lead, s0, park, expand)
    OPEN = -1
    slot = {0: (0, OPEN - 1, OPEN), 1: (1, OPEN - 1, OPEN) if s0 > park else None}

    def read(rel, at):
        b = rel // S
        held = slot[b & 1]
        assert held is not None and held[0] == b, (what, sched, "record", rel, "read at", at, "slot holds", held)
        assert held[1] < held[2] < at, (what, sched, "record", rel, "read at", at, "parked / expanded at", held[1:])

    for rel in (s0, s0 + 1):          # the launch's first column and the first step's emissions, behind the opening barrier
        read(rel, s0 - 0.5)
    for n, k in zip(n_arr.tolist(), kind.tolist()):
        # (the backward role does its upkeep in front of the step's barrier and reads behind it; the forward role reads and does
        #  its upkeep behind the barrier of the step before: either way a write of step n meets the reads of step n - 1 at most)
        if k == 1:
            b = (n + 4) // S
            old = slot[b & 1]
            assert old is None or old[0] < n // S, (what, sched, "block", b, "parked at", n, "over", old)
            slot[b & 1] = (b, n, None)
        elif k == 2:
            b = (n + 3) // S
            held = slot[b & 1]
            assert held is not None and held[0] == b and held[1] < n, (what, sched, "block", b, "expanded at", n, "slot holds", held)
            if held[2] is None:       # (a launch that opens with block 1 expanded may expand it once more at its first step: the same bytes)
                slot[b & 1] = (b, held[1], n)
        if role == 1:
            read(n + 1, n)
        read(n + 2, n)


def test_consecutive_records_lie_256_bytes_apart_modulo_the_ring(lib):
    """one 256-byte image per record, 128 of them: block b of 64 records fills half b & 1 of the ring in record order, and the
    images of two records of different blocks that are live together never coincide"""
    IMAGE, RING = 256, 2 * S * 256
    for rel in list(range(0, 5 * S)) + [2 ** 31 - 2, 2 ** 32 - 2]:
        a, b = lib.pg_lean_ring_image_offset(rel), lib.pg_lean_ring_image_offset((rel + 1) & 0xFFFFFFFF)
        assert a % IMAGE == 0 and a < RING
        assert b == (a + IMAGE) % RING
        assert a == (((rel // S) & 1) * S + rel % S) * IMAGE      # where LeanRecs::park puts the record


@pytest.mark.parametrize("role", [0, 1])
@pytest.mark.parametrize("K", CHUNKS)
def test_every_launch_form_small_chains(lib, K, role):
    seen = set()
    for n in SMALL:
        for what, sched in _launches(lib, n, K, role):
            key = sched[1:]           # (the books depend on steps, lead and first number alone)
            _check_arithmetic((n, K, role, what), sched)
            if key not in seen:
                seen.add(key)
                _walk((n, K, role, what), sched, role)
    assert len(seen) > 50 or K == 8192


@pytest.mark.parametrize("role", [0, 1])
@pytest.mark.parametrize("K", CHUNKS)
@pytest.mark.parametrize("n", LARGE)
def test_every_launch_form_genome_sized_chain(lib, n, K, role):
    seen = set()
    count = 0
    for what, sched in _launches(lib, n, K, role):
        count += 1
        if sched[1:] in seen:
            continue
        seen.add(sched[1:])
        _check_arithmetic((n, K, role, what), sched)
        if sched[1] <= 40000:
            _walk((n, K, role, what), sched, role)
    assert count >= 1 + 3 + 1


def test_every_first_number_a_launch_can_take(lib):
    """the leading piece of a single launch meets every residue: 64 consecutive chain lengths, both roles — and the first numbers
    behind the parking step (61, 62, 63: a leading piece of three, two, one steps) open with two blocks"""
    for role in (0, 1):
        firsts = set()
        for n in range(640, 640 + 2 * S):
            sched = _schedule(lib, n, 64, 1, role, 0, 0)
            firsts.add(sched[3])
            assert sched[3] == (S - sched[2]) % S
        assert firsts == set(range(S)), (role, sorted(firsts))


def test_tested_launches_number_from_zero():
    """a refill segment (63 or 64 steps) and every dense launch keep the tested step and number their steps from 0"""
    for role in (0, 1):
        for steps in (1, 2, 62, 63, 64, 65, 127, 128, 129, 700):
            _walk(("tested", steps), (0, steps, 0, 0, S - 4, S - 3), role)


def test_arguments_outside_the_scheme(lib):
    out = (C.c_uint32 * 6)()
    assert lib.pg_lean_ring_schedule(1000, 96, 1, 0, 0, 0, out) == -1
    assert lib.pg_lean_ring_schedule(1000, 0, 1, 0, 0, 0, out) == -1
    assert lib.pg_lean_ring_schedule(1000, 64, 1, 2, 0, 0, out) == -1
    assert lib.pg_lean_ring_schedule(1000, 64, 1, 0, 3, 0, out) == -1
    assert lib.pg_lean_ring_schedule(1000, 64, 0, 0, 1, 0, out) == -1
    assert lib.pg_lean_ring_schedule(1000, 64, 1, 0, 0, 0, None) == 1
    assert lib.pg_lean_ring_schedule(0, 64, 1, 0, 0, 0, out) == 0 and lib.pg_lean_ring_schedule(0, 64, 1, 1, 0, 0, out) == 0
    assert lib.pg_lean_ring_schedule(1, 64, 1, 0, 0, 0, out) == 0 and lib.pg_lean_ring_schedule(1, 64, 1, 1, 0, 0, out) == 0
