"""The device k-mer counter (pangenie_amd/csrc/pg_kmers.hip) on the paths that random texts of test size do not reach, each
against the restatements of tests/test_kmers_gpu.py (dict_counts, numpy_counts), exactly:

  A  probe runs that are CONSTRUCTED: the table's hash is restated here in Python integers, codes are searched for chosen home
     slots, so that a run wraps round the end of the table, one run is 250 slots long, and the smallest table is full at its end;
  B  the histogram above KK_HIST_LDS = 1024 (global atomics), the `count > max_count` cut and the LDS flush above a small max_count;
  C  the seams between staging buffers (8 MiB pieces that overlap by k - 1 bytes) with text ends and non-letters on them;
  D  every byte value at every position of a 16-byte chunk."""
from collections import Counter

import numpy as np
import pytest

from pangenie_amd import _lib, kmers
from tests.test_counts_gpu import assert_same, contig_of, restated_fill
from tests.test_kmers_gpu import check_all, dict_counts, numpy_counts, rc

pytestmark = pytest.mark.gpu

NONE = kmers.NOT_REGISTERED
ACGT = np.frombuffer(b"ACGT", np.uint8)
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ A. constructed collisions
def mix64(x: int) -> int:
    """the splitmix64 finaliser of pg_kmers.hip / kmer_counts.cpp in Python integers"""
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    x ^= x >> 31
    return x


def home(code: int, cap: int) -> int:
    return (mix64(code) * cap) >> 64


def capacity(n: int) -> int:
    return max(16, 2 * n + 1)


def search(rng, k, cap, homes, n, taken):
    """n random canonical k-mers (code, string) whose home slot is in `homes` (None: any), none of them in `taken`"""
    found = []
    while len(found) < n:
        strings = [row.tobytes() for row in rng.choice(ACGT, (20000, k))]
        for s, code in zip(strings, kmers.canonical_codes(strings, k).tolist()):
            if code in taken or (homes is not None and home(code, cap) not in homes):
                continue
            taken.add(code)
            found.append((code, s))
            if len(found) == n:
                break
    return found


def occupied_slots(codes, cap):
    """the slots linear probing fills (the set does not depend on the order of the insertions)"""
    full = set()
    for code in codes:
        at = home(code, cap)
        while at in full:
            at = (at + 1) % cap
        full.add(at)
    return full


def reads_of_kmers(rng, items):
    """a text of the k-mers themselves: (string, times) -> that many lines, every other one the reverse complement, shuffled"""
    lines = [s if i % 2 == 0 else rc(s) for s, times in items for i in range(times)]
    order = rng.permutation(len(lines))
    return b"\n".join(lines[i] for i in order) + b"\n"


def displacements(table, cap):
    """the open-addressing invariant on a snapshot: walking from every key's home slot, with wrap, reaches the key before any
    empty slot.  Returns {key: (home, slot)}."""
    keys = table[:, 0].tolist()
    where = {}
    for slot, key in enumerate(keys):
        if key == NONE:
            continue
        assert key not in where, ("a key in two slots", key, where[key], slot)
        at = h = home(key, cap)
        while at != slot:
            assert keys[at] != NONE, ("an empty slot between a key's home and the key", key, h, slot, at)
            at = (at + 1) % cap
        where[key] = (h, slot)
    return where


def constructed_case(k, rng, members, foreign):
    """`members` (code, string) are registered in one add_codes; `foreign` are not, and their home slots are occupied.
    Returns {key: (home, slot)} of the table for the caller's condition on the input."""
    cap = capacity(len(members))
    codes = [c for c, _ in members]
    assert len(set(codes)) == len(codes) and not set(codes) & {c for c, _ in foreign}
    full = occupied_slots(codes, cap)
    assert all(home(c, cap) in full for c, _ in foreign)   # (every foreign probe walks at least one slot)
    registered = Counter(dict.fromkeys(codes, 1))
    with kmers.KmerCounter(k) as counter:
        counter.add_codes(np.array(codes, np.uint64))
        table = counter.table()
        assert table.shape[0] == cap, (table.shape, cap)   # the sizing rule this construction rests on
        where = displacements(table, cap)
        assert set(where) == set(codes) and {slot for _, slot in where.values()} == full
        # Which key settled where depends on the order the insertions arrived in, so the reads are made now: 0, 1, 2 or 7 of
        # every k-mer, but at least one of every key that lies behind the wrap (a probe that misses slot 0 must miss a read),
        # and 3000 of the key farthest from its home slot.
        times = [(0, 1, 2, 7)[i % 4] for i in range(len(members))]
        for i, c in enumerate(codes):
            if where[c][1] < where[c][0] and times[i] == 0:
                times[i] = 1
        times[max(range(len(codes)), key=lambda i: (where[codes[i]][1] - where[codes[i]][0]) % cap)] = 3000
        items = [(s, t) for (_, s), t in zip(members, times)] + [(s, 1 + i % 3) for i, (_, s) in enumerate(foreign)]
        text = reads_of_kmers(rng, items)
        want = dict_counts(text, k)
        assert all(want.get(c, 0) == t for c, t in zip(codes, times)) and all(want[c] == 1 + i % 3 for i, (c, _) in enumerate(foreign))
        seen = {c: want.get(c, 0) for c in codes}   # what a plan may see: the counts of registered codes only
        counter.count(text)
        check_all(counter, registered, want, sum(want.values()))
        displaced = displacements(counter.table(), cap)
        assert displaced == where   # counting moves no key
        if foreign:
            assert (counter.lookup_codes(np.array([c for c, _ in foreign], np.uint64)) == np.uint64(NONE)).all()
        # the count plan over the same runs: kk_plan_resolve walks them too
        pool = np.array(codes, np.uint64)
        contigs = [contig_of(rng, pool, 60, 5, 12, n_rate=0.05), contig_of(rng, pool, 33, 3, 40, n_rate=0.05)]
        with kmers.CountPlan(counter, contigs) as plan:
            assert plan.stats().unresolved == 0
            for coverage in (0, 1, 3, 30, 20000):
                got, expect = plan.fill(coverage), restated_fill(contigs, seen, coverage)
                assert_same(got[0], expect[0], f"kmer_count at {coverage}")
                assert_same(got[1], expect[1], f"coverage at {coverage}")
        if foreign:
            strangers = np.array([c for c, _ in foreign], np.uint64)
            lenient = [contig_of(rng, np.concatenate([pool, strangers]), 60, 5, 12, n_rate=0.05)]
            asked = np.concatenate([lenient[0].kmer_code, lenient[0].flank_code])
            unresolved = int(np.isin(asked, strangers).sum())
            assert unresolved > 0
            with pytest.raises(kmers.KmerCounterError) as e:
                kmers.CountPlan(counter, lenient)
            assert e.value.code == _lib.PG_ERR_INVALID
            with kmers.CountPlan(counter, lenient, lenient=True) as plan:
                assert plan.stats().unresolved == unresolved
                for coverage in (1, 3):
                    got, expect = plan.fill(coverage), restated_fill(lenient, seen, coverage)
                    assert_same(got[0], expect[0], f"lenient kmer_count at {coverage}")
                    assert_same(got[1], expect[1], f"lenient coverage at {coverage}")
    return where


@pytest.mark.parametrize("k", [31, 32])
def test_a_probe_run_that_wraps_round_the_end_of_the_table(k):
    """300 codes, 601 slots: 120 codes at home in the last slot and 120 in the ten slots before it fill slots 590 ... 600 and
    229 slots from slot 0 on; unregistered k-mers at home inside that run walk it to its end"""
    rng = np.random.default_rng(600 + k)
    n = 300
    cap = capacity(n)
    assert cap == 601
    taken = set()
    members = search(rng, k, cap, {cap - 1}, 120, taken) + search(rng, k, cap, set(range(cap - 11, cap - 1)), 120, taken) + search(rng, k, cap, None, 60, taken)
    foreign = search(rng, k, cap, {cap - 11, cap - 2, cap - 1, 0, 1, 100, 228}, 40, taken)
    order = rng.permutation(n)
    where = constructed_case(k, rng, [members[i] for i in order], foreign)
    below = [key for key, (h, slot) in where.items() if slot < h]
    assert len(below) >= 229, len(below)             # the wrap happened: keys in slots below their home
    assert all(s in {slot for _, slot in where.values()} for s in list(range(cap - 11, cap)) + list(range(229)))


@pytest.mark.parametrize("k", [31, 32])
def test_one_long_probe_run(k):
    """250 codes with the same home slot in the middle of the table: the last one inserted lies 249 slots from home, and a
    window of kk_count goes through up to 250 rounds while its neighbours are done after the first"""
    rng = np.random.default_rng(700 + k)
    n = 250
    cap = capacity(n)
    at = cap // 2
    taken = set()
    members = search(rng, k, cap, {at}, n, taken)
    foreign = search(rng, k, cap, {at, at + 1, at + 125, at + 249}, 20, taken)
    where = constructed_case(k, rng, members, foreign)
    assert sorted(slot for _, slot in where.values()) == list(range(at, at + n))
    assert all(h == at for h, _ in where.values())


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("k", [31, 32])
def test_the_smallest_table_with_every_home_in_its_last_slot(k, n):
    rng = np.random.default_rng(800 + 10 * k + n)
    cap = capacity(n)
    assert cap == 16
    taken = set()
    members = search(rng, k, cap, {cap - 1}, n, taken)
    foreign = search(rng, k, cap, {cap - 1} | set(range(n - 1)), 6, taken)
    where = constructed_case(k, rng, members, foreign)
    assert sorted(slot for _, slot in where.values()) == sorted([cap - 1] + list(range(n - 1)))
    assert sum(slot < h for h, slot in where.values()) == n - 1   # all but one key wrapped


# ------------------------------------------------------------------------------------------------------------ B. histogram
def test_histogram_on_both_sides_of_the_lds_bins():
    """counts below 1024 meet in LDS, counts from 1024 on go to hist[count] with global atomics, counts above max_count are cut"""
    k = 15
    rng = np.random.default_rng(1024)
    planned = [0, 1, 2, 1022, 1023, 1024, 1025, 4096] * 3 + [70000, 300000]
    strings = [row.tobytes() for row in rng.choice(ACGT, (len(planned), k))]
    codes = kmers.canonical_codes(strings, k)
    assert len(set(codes.tolist())) == len(planned)
    rows = np.frombuffer(b"".join(s + b"\n" + rc(s) + b"\n" for s in strings), np.uint8).reshape(2 * len(planned), k + 1)
    idx = np.concatenate([np.repeat(np.array([2 * i, 2 * i + 1]), [c - c // 2, c // 2]) for i, c in enumerate(planned)])
    rng.shuffle(idx)
    registered = Counter(dict.fromkeys(codes.tolist(), 1))
    limits = [0, 1, 2, 1022, 1023, 1024, 1025, 4095, 4096, 69999, 70000, 300000, 1 << 20]

    def histogram_of(expected, max_count):
        hist = np.bincount(expected, minlength=max_count + 1)[:max_count + 1].astype(np.uint64)
        hist[0] = 0   # (the kernel leaves unseen codes out)
        return hist

    with kmers.KmerCounter(k) as counter:
        counter.add_codes(codes)
        for lines, expected in ((idx, np.array(planned, np.int64)), (idx[::3], None)):
            text = rows[lines].tobytes()
            want = numpy_counts(text, k)
            by_code = np.array([want.get(c, 0) for c in codes.tolist()], np.int64)
            if expected is None:   # the second sample: every third line
                expected = by_code
                assert expected.max() > 70000 and (expected == 0).sum() >= 3
            assert np.array_equal(by_code, expected)
            counter.reset_counts()
            counter.count(text)
            check_all(counter, registered, want, lines.size)
            for max_count in limits if lines is idx else [1025]:
                got = counter.histogram(max_count)
                assert got.shape == (max_count + 1,) and np.array_equal(got, histogram_of(expected, max_count)), max_count
        with pytest.raises(kmers.KmerCounterError) as e:
            counter.histogram(1 << 28)
        assert e.value.code == _lib.PG_ERR_UNSUPPORTED


# -------------------------------------------------------------------------------------------------------- C. staging seams
STAGE = 8 << 20   # KK_STAGE_BYTES of pg_kmers.hip: a text longer than this goes to the device in pieces that overlap by k - 1 bytes


def seam_lengths(k):
    S = STAGE
    return [S - 1, S, S + 1, S + k - 2, S + k - 1, S + k, 2 * S - (k - 1), 2 * S - (k - 1) + 1, 2 * S + 5]   # (the last three: two seams)


def seam_offsets(k):
    """round the end of the first piece (S) and of the second (it starts at S - (k - 1) and ends at 2 S - (k - 1)).  All seven
    offsets at k = 31; at k = 4 and 32 three of them: with all seven at every k the test took 31.6 s on an MI355X machine, where
    test_a_million_targets_ten_million_windows takes 3.8 s."""
    around = (-k, -k + 1, -2, -1, 0, 1, k - 2) if k == 31 else (-k + 1, -1, 0)
    return [end + d for end in (STAGE, 2 * STAGE - (k - 1)) for d in around]


def counts_of_prefixes(text, lengths, k):
    """numpy_counts of text[:n] for every n, each from the one before: the windows of text[:n] that are not windows of
    text[:done] are the windows of text[done - (k - 1):n]"""
    out, have, done = {}, Counter(), 0
    for n in sorted(lengths):
        have = have + numpy_counts(text[max(0, done - (k - 1)):n], k)
        out[n], done = have, n
    return out


def counts_after_a_change(counts, before, after, at, n, k):
    """numpy_counts of `after`, which differs from `before` in bytes [at, at + n) only: the windows that touch those bytes are
    the windows of [at - (k - 1), at + n + (k - 1)), all others are the same windows"""
    lo, hi = max(0, at - (k - 1)), min(len(before), at + n + (k - 1))
    c = Counter(counts)
    c.subtract(numpy_counts(before[lo:hi], k))
    c.update(numpy_counts(after[lo:hi], k))
    assert all(v >= 0 for v in c.values())
    return +c


@pytest.mark.parametrize("k", [4, 31, 32])
def test_text_ends_and_non_letters_on_the_seams_between_staging_buffers(k):
    rng = np.random.default_rng(8 + k)
    genome = rng.choice(ACGT, 200000).tobytes()
    longest = 2 * STAGE + 5
    text = (genome * (longest // len(genome) + 1))[:longest]
    registered = numpy_counts(genome, k)   # (the windows across the joints of the repeated genome are not registered)
    by_length = counts_of_prefixes(text, seam_lengths(k), k)
    whole = by_length[longest]
    assert whole == numpy_counts(text, k)   # the stepwise reference is the direct one
    if k == 31:
        assert dict_counts(text[:1000000], k) == numpy_counts(text[:1000000], k)

    def cases():
        for n in seam_lengths(k):
            yield f"length {n}", text[:n], by_length[n]
        for at in seam_offsets(k):
            for mark in (b"\n", b"N", b"\r\n", text[at:at + 1].lower()):
                changed = bytearray(text)
                changed[at:at + len(mark)] = mark
                changed = bytes(changed)
                want = counts_after_a_change(whole, text, changed, at, len(mark), k)
                if mark == b"N" and at == STAGE - 1:
                    assert want == numpy_counts(changed, k)   # ... and so is the reference of a changed text
                if mark.islower():
                    assert want == whole
                yield f"{mark!r} at {at}", changed, want

    done = 0
    with kmers.KmerCounter(k) as counter:
        counter.add_text(genome)
        for name, t, want in cases():
            counter.reset_counts()
            counter.count(t)
            try:
                check_all(counter, registered, want, sum(want.values()))
            except AssertionError as e:
                raise AssertionError(f"count, k = {k}, {name}: {e}") from e
            with kmers.KmerCounter(k) as fresh:   # the same text as the source of the targets: registered in pieces too
                assert fresh.add_text(t) == sum(want.values()), (k, name)
                assert fresh.stats().targets == len(want), (k, name)
            done += 1
    assert done == 9 + (14 if k == 31 else 6) * 4


# -------------------------------------------------------------------------------- D. every byte at every chunk position
@pytest.mark.parametrize("k", [1, 5, 16])
def test_every_byte_value_at_every_position_of_a_chunk(k):
    """dict_counts' CODE table is the specification: exactly ACGTacgt are letters.  Each byte value stands at each position
    modulo 16 between two runs of letters of lengths k - 1, k and k + 3 (the newlines in front only align it)."""
    rng = np.random.default_rng(160 + k)
    out, at = [], 0
    for before, after in ((k - 1, k), (k, k + 3), (k + 3, k - 1)):
        for value in range(256):
            for position in range(16):
                pad = (position - (at + before)) % 16
                piece = b"\n" * pad + rng.choice(ACGT, before).tobytes() + bytes([value]) + rng.choice(ACGT, after).tobytes() + b"\n"
                assert (at + pad + before) % 16 == position
                out.append(piece)
                at += len(piece)
    text = b"".join(out)
    want = dict_counts(text, k)
    with kmers.KmerCounter(k) as counter:
        assert counter.add_text(text) == sum(want.values())
        counter.count(text)
        check_all(counter, want, want, sum(want.values()))
    other = dict_counts(rc(text), k)   # targets from one text, counts from another: the reverse strand, bytes in other positions
    assert other == want
    with kmers.KmerCounter(k) as counter:
        counter.add_codes(np.fromiter(want.keys(), np.uint64, len(want)))
        counter.count(rc(text)[3:])
        shifted = dict_counts(rc(text)[3:], k)
        check_all(counter, want, shifted, sum(shifted.values()))
