"""The device k-mer counter (include/pangenie_kmers.h, pangenie_amd/kmers.py) against counts formed in Python over the
same text: a plain dictionary filled letter by letter for the small cases; for texts of megabytes numpy, which forms every
window's code from its k letters without rolling (the two are checked against each other on the CPU).  Every comparison is exact and
covers every registered k-mer."""
from collections import Counter

import numpy as np
import pytest

from pangenie_amd import _lib, kmers

CODE = {c: i for i, c in enumerate("ACGT")}
CODE.update({c.lower(): i for c, i in list(CODE.items())})
KS = [1, 4, 15, 16, 31, 32]


def dict_counts(text: bytes, k: int) -> Counter:
    """canonical code -> windows, letter by letter (the rule of kmer_counts.hpp, restated in Python integers)"""
    counts = Counter()
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    fwd = rev = filled = 0
    for ch in text.decode("latin-1"):
        b = CODE.get(ch)
        if b is None:
            filled = 0
            continue
        fwd = ((fwd << 2) | b) & mask
        rev = (rev >> 2) | ((3 - b) << top)
        filled += 1
        if filled >= k:
            counts[min(fwd, rev)] += 1
    return counts


_LUT = np.full(256, 4, np.uint8)
for _c, _i in CODE.items():
    _LUT[ord(_c)] = _i


def numpy_counts(text: bytes, k: int) -> Counter:
    a = _LUT[np.frombuffer(text, np.uint8)]
    n = a.size - k + 1
    if n <= 0:
        return Counter()
    bad = np.concatenate(([0], np.cumsum(a > 3)))
    whole = (bad[k:] - bad[:-k]) == 0
    b = (a & 3).astype(np.uint64)
    fwd = np.zeros(n, np.uint64)
    rev = np.zeros(n, np.uint64)
    for i in range(k):
        fwd = (fwd << np.uint64(2)) | b[i:i + n]
        rev = (rev << np.uint64(2)) | (np.uint64(3) - b[k - 1 - i:k - 1 - i + n])
    codes, times = np.unique(np.minimum(fwd, rev)[whole], return_counts=True)
    return Counter(dict(zip(codes.tolist(), times.tolist())))


def messy_text(seed: int, letters: int) -> bytes:
    """reads of all lengths (many shorter than 32), lower case, N, \\r\\n, runs of separators, other bytes"""
    rng = np.random.default_rng(seed)
    out = []
    total = 0
    while total < letters:
        n = int(rng.choice([1, 3, 14, 15, 16, 30, 31, 32, 33, 64, 150, 151, 1000]))
        s = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())
        if rng.random() < 0.3:
            s = bytearray(bytes(s).lower())
        if rng.random() < 0.2:
            s[int(rng.integers(n))] = ord("N")
        if rng.random() < 0.05:
            s[int(rng.integers(n))] = int(rng.integers(128, 256))
        out.append(bytes(s))
        out.append([b"\n", b"\r\n", b"\n\n\n", b"\n>x y\n", b"\x00", b"NNNN"][int(rng.integers(6))])
        total += n
    return b"".join(out)


def rc(text: bytes) -> bytes:
    return text[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def check_all(counter, registered: Counter, want: Counter, windows: int):
    """every registered code has exactly the wanted count; stats and histogram follow from the same dictionary"""
    codes = np.fromiter(registered.keys(), np.uint64, len(registered))
    got = counter.lookup_codes(codes)
    expect = np.array([want.get(int(c), 0) for c in codes.tolist()], np.uint64)
    wrong = np.nonzero(got != expect)[0]
    assert wrong.size == 0, (wrong.size, codes[wrong[:5]], got[wrong[:5]], expect[wrong[:5]])
    st = counter.stats()
    assert st.targets == len(registered) and st.windows == windows
    top = 40
    hist = np.zeros(top + 1, np.uint64)
    for c in expect.tolist():
        if 0 < c <= top:
            hist[c] += 1
    assert np.array_equal(counter.histogram(top), hist)
    table = counter.table()
    filled = table[table[:, 0] != np.uint64(kmers.NOT_REGISTERED)]
    assert filled.shape[0] == len(registered)
    assert dict(zip(filled[:, 0].tolist(), filled[:, 1].tolist())) == {int(c): int(e) for c, e in zip(codes.tolist(), expect.tolist())}


@pytest.mark.parametrize("k", [1, 4, 15, 32])
def test_the_two_references_agree(k):
    text = messy_text(3, 6000) + b"ACGTACGTAC" * 7 + b"acgtnACGT"
    assert dict_counts(text, k) == numpy_counts(text, k)
    assert dict_counts(b"ACGTACGT\nACGNACGTA", 4) == Counter({0b00011011: 3, 0b01101100: 3, 0b10110001: 1})


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_messy_text_every_k(k):
    graph, reads = messy_text(10 + k, 40000), messy_text(100 + k, 150000) + messy_text(10 + k, 40000)[:30000]
    registered, want = dict_counts(graph, k), dict_counts(reads, k)
    with kmers.KmerCounter(k) as c:
        assert c.add_text(graph) == sum(registered.values())
        c.count(reads)
        check_all(c, registered, want, sum(want.values()))
        # never registered: the marker, not a silent 0 (codes of the reads that are not in the graph, if there are any)
        foreign = [code for code in want if code not in registered][:1000]
        if foreign:
            assert (c.lookup_codes(foreign) == np.uint64(kmers.NOT_REGISTERED)).all()
    if k >= 15:
        assert foreign and any(v == 0 for v in (want.get(code, 0) for code in registered))   # registered and unseen answer 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_buffers_that_end_early(k):
    rng = np.random.default_rng(k)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 3 * k + 5).tobytes()
    registered = dict_counts(seq, k)
    for text in (b"", seq[:k - 1], seq[:k], seq[:k + 1], seq[:2 * k - 1] + b"\n" + seq[:k - 1], seq + b"\n" + seq[:k // 2]):
        with kmers.KmerCounter(k) as c:
            c.add_text(seq)
            c.count(text)
            want = dict_counts(text, k)
            check_all(c, registered, want, sum(want.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 31, 32])
def test_tile_edges(k):
    tile = kmers.tile_bytes()
    rng = np.random.default_rng(77 + k)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 3 * tile + 100).tobytes()
    registered = numpy_counts(seq, k)
    texts = [seq[:n] for n in (tile - 1, tile, tile + 1, tile + k - 1, tile + k, 2 * tile, 2 * tile + k - 2)]
    for at in (tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, tile - k, tile - k + 1, tile + k - 1):
        t = bytearray(seq)
        t[at] = ord("\n")
        texts.append(bytes(t))
    t = bytearray(seq)
    t[tile - 2:tile + 2] = b"\r\n\r\n"
    texts.append(bytes(t))
    with kmers.KmerCounter(k) as c:
        c.add_text(seq)
        for text in texts:
            c.reset_counts()
            c.count(text)
            want = numpy_counts(text, k)
            assert want == dict_counts(text, k)
            check_all(c, registered, want, sum(want.values()))


@pytest.mark.gpu
def test_one_sequence_of_several_megabytes():
    """longer than a staging buffer: the pieces overlap by k - 1 letters and every window is counted once"""
    k = 31
    rng = np.random.default_rng(5)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 300000).tobytes()
    seq = (genome * 31)[: 9 * 1024 * 1024 + 12345]   # one sequence, no separator, 9 MB
    registered, want = numpy_counts(genome, k), numpy_counts(seq, k)
    with kmers.KmerCounter(k) as c:
        c.add_text(genome)
        c.count(seq)
        check_all(c, registered, want, sum(want.values()))
    with kmers.KmerCounter(k) as c:   # the same text as the target source: registered in pieces too
        assert c.add_text(seq) == len(seq) - k + 1
        assert c.stats().targets == len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 4, 31, 32])
def test_low_complexity(k):
    for text in (b"A" * 200000, b"AC" * 100000, b"t" * 70001):
        want = dict_counts(text, k)
        assert len(want) <= 2
        with kmers.KmerCounter(k) as c:
            c.add_text(text[:4 * k])
            c.add_text(b"ACGTTGCA" * 8)
            registered = dict_counts(text[:4 * k], k) + dict_counts(b"ACGTTGCA" * 8, k)
            c.count(text)
            check_all(c, registered, want, sum(want.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 15, 32])
def test_both_strands(k):
    graph, reads = messy_text(1, 30000), messy_text(2, 60000) + messy_text(1, 30000)
    registered = dict_counts(graph, k)
    codes = np.fromiter(registered.keys(), np.uint64, len(registered))
    with kmers.KmerCounter(k) as a, kmers.KmerCounter(k) as b:
        a.add_text(graph)
        b.add_text(rc(graph))
        a.count(reads)
        b.count(rc(reads))
        assert a.stats() == b.stats()
        assert np.array_equal(a.lookup_codes(codes), b.lookup_codes(codes))
        want = dict_counts(reads, k)
        check_all(b, registered, want, sum(want.values()))


@pytest.mark.gpu
def test_targets_given_twice_as_codes_and_as_text_count_once():
    k = 15
    graph, reads = messy_text(4, 20000), messy_text(5, 50000) + messy_text(4, 20000)
    registered = dict_counts(graph, k)
    codes = np.fromiter(registered.keys(), np.uint64, len(registered))
    with kmers.KmerCounter(k) as c:
        c.add_codes(codes)
        c.add_text(graph)
        c.add_codes(codes[::-1])
        c.add_text(graph.lower())
        c.count(reads)
        want = dict_counts(reads, k)
        check_all(c, registered, want, sum(want.values()))
    with kmers.KmerCounter(k) as c:   # strings through the numpy helper
        some = ["ACGTACGTACGTACG", "CGTACGTACGTACGT", "AAAAAAAAAAAAAAA", "TTTTTTTTTTTTTTT"]
        c.add_codes(kmers.canonical_codes(some, k))
        c.count(b"ACGTACGTACGTACGT\nAAAAAAAAAAAAAAAAA\n")
        assert c.stats() == (2, 5)   # (the first two are each other's reverse complement, the last two too)
        assert c.lookup(some + ["ACGTACGTACGTACC"]).tolist() == [2, 2, 3, 3, kmers.NOT_REGISTERED]
        with pytest.raises(kmers.KmerCounterError) as e:
            kmers.KmerCounter(4).add_codes([256])
        assert e.value.code == _lib.PG_ERR_INVALID


@pytest.mark.gpu
def test_counts_add_up_reset_gives_zeros_and_a_fresh_start():
    k = 16
    graph, r1, r2 = messy_text(6, 30000), messy_text(7, 80000) + messy_text(6, 30000)[:9000], messy_text(8, 50000) + messy_text(6, 30000)[9000:]
    registered = dict_counts(graph, k)
    w1, w2 = dict_counts(r1, k), dict_counts(r2, k)
    with kmers.KmerCounter(k) as c:
        c.add_text(graph)
        c.count(r1, sync=False)
        c.count(r2, sync=False)
        check_all(c, registered, w1 + w2, sum(w1.values()) + sum(w2.values()))
        c.reset_counts()
        check_all(c, registered, Counter(), 0)
        c.count(r2)
        with kmers.KmerCounter(k) as fresh:
            fresh.add_text(graph)
            fresh.count(r2)
            # (slot by slot the two tables may differ: colliding codes settle in the order their insertions arrive)
            a, b = (t[t[:, 0] != np.uint64(kmers.NOT_REGISTERED)] for t in (fresh.table(), c.table()))
            assert np.array_equal(a[np.argsort(a[:, 0])], b[np.argsort(b[:, 0])])
        check_all(c, registered, w2, sum(w2.values()))


@pytest.mark.gpu
def test_registering_after_the_first_count_is_invalid():
    with kmers.KmerCounter(4) as c:
        c.add_text(b"ACGTACGT")
        c.count(b"ACGTAC")
        for call in (lambda: c.add_text(b"GGGGGG"), lambda: c.add_codes([1, 2])):
            with pytest.raises(kmers.KmerCounterError) as e:
                call()
            assert e.value.code == _lib.PG_ERR_INVALID
        assert c.stats() == (3, 3)


@pytest.mark.gpu
def test_a_million_targets_ten_million_windows():
    """at least 2^20 distinct codes, about ten times as many windows: collisions and long probe runs in a table of millions"""
    k = 31
    rng = np.random.default_rng(2024)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), (1 << 20) + 150000)
    graph = genome.tobytes()
    reads = []
    for r in range(13):   # 13 passes over the genome in reads of 150 (120 windows each), every other pass on the other strand, a few wrong letters
        g = genome.copy()
        hit = rng.integers(0, g.size, g.size // 400)
        g[hit] = rng.choice(np.frombuffer(b"ACGTN", np.uint8), hit.size)
        shift = int(rng.integers(0, 150))
        body = g[shift:shift + (g.size - shift) // 150 * 150].reshape(-1, 150)
        lines = np.concatenate([body, np.full((body.shape[0], 1), 10, np.uint8)], axis=1).tobytes()
        reads.append(rc(lines) if r % 2 else lines)
    text = b"".join(reads)
    registered, want = numpy_counts(graph, k), numpy_counts(text, k)
    assert len(registered) >= 1 << 20 and sum(want.values()) > 9 * len(registered)
    with kmers.KmerCounter(k) as c:
        c.add_text(graph)
        c.count(text)
        check_all(c, registered, want, sum(want.values()))
