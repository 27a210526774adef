"""The count plan on the device (include/pangenie_counts.h) against a NumPy / dictionary restatement of
pangenie::fill_read_kmercounts + windowed_mean: every entry equal, no tolerance.  Tables and reads are made here."""
import numpy as np
import pytest

from pangenie_amd import _lib, hmm, kmers
from pangenie_amd.panel import default_table_args, synthetic_panel

pytestmark = pytest.mark.gpu

NONE = kmers.NOT_REGISTERED
COVERAGES = (0, 1, 3, 30, 20000, 70000)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def genome(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def windows(text: bytes, k: int):
    return [text[i:i + k] for i in range(len(text) - k + 1)]


def reads_of(rng, g: bytes, n: int, length: int = 90) -> bytes:
    out = []
    for r in range(n):
        at = int(rng.integers(0, len(g) - length))
        piece = bytearray(g[at:at + int(rng.integers(length // 2, length))])
        if r % 2:
            piece = bytearray(bytes(piece).translate(COMP)[::-1])
        if r % 11 == 0:
            piece[int(rng.integers(0, len(piece)))] = ord("N")
        if r % 5 == 0:
            piece = bytearray(bytes(piece).lower())
        out.append(bytes(piece))
    return b"\n".join(out) + b"\n"


def dictionary_counts(text: bytes, k: int) -> dict:
    """canonical code -> occurrences over every window of k letters of ACGTacgt in the text"""
    seen = {}
    for line in text.split(b"\n"):
        if len(line) < k:
            continue
        codes = kmers.canonical_codes(windows(line, k), k)
        for c, n in zip(*np.unique(codes[codes != np.uint64(NONE)], return_counts=True)):
            seen[int(c)] = seen.get(int(c), 0) + int(n)
    return seen


def windowed_mean(counts, expected: int) -> int:
    lowest, highest = expected // 4, (expected * 4) & (2 ** 64 - 1)
    inside = [c for c in counts if lowest <= c <= highest]
    return (sum(inside) // len(inside) if inside and sum(inside) else expected) & 0xFFFF


def restated_fill(contigs, seen: dict, kmer_coverage: int):
    """fill_read_kmercounts in plain Python: a code that is not in the dictionary (never seen, never registered, or a k-mer
    with an N) counts 0"""
    count = lambda code: 0 if int(code) == NONE else seen.get(int(code), 0)
    kc, cv = [], []
    for c in contigs:
        kc.append(np.array([count(x) & 0xFFFF for x in c.kmer_code], np.uint16))
        cv.append(np.array([windowed_mean([count(x) for x in c.flank_code[int(c.flank_off[v]):int(c.flank_off[v + 1])]], kmer_coverage)
                            for v in range(c.n_variants)], np.uint16))
    return kc, cv


def contig_of(rng, pool, n_variants, max_kmers, max_flanks, n_rate=0.02):
    """a contig whose variants ask about random members of `pool` (codes), now and then about a k-mer with an N"""
    nk = rng.integers(0, max_kmers + 1, n_variants) if max_kmers else np.zeros(n_variants, np.int64)
    nf = rng.integers(0, max_flanks + 1, n_variants) if max_flanks else np.zeros(n_variants, np.int64)
    def draw(n):
        codes = pool[rng.integers(0, len(pool), n)].copy()
        codes[rng.random(n) < n_rate] = np.uint64(NONE)
        return codes
    return kmers.CountContig(np.concatenate([[0], np.cumsum(nk)]).astype(np.uint32), draw(int(nk.sum())),
                             np.concatenate([[0], np.cumsum(nf)]).astype(np.uint64), draw(int(nf.sum())))


def empty_contig():
    return kmers.CountContig(np.zeros(1, np.uint32), np.zeros(0, np.uint64), np.zeros(1, np.uint64), np.zeros(0, np.uint64))


def assert_same(got, want, what):
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint16 and g.shape == w.shape, (what, c)
        assert np.array_equal(g, w), (what, c, np.flatnonzero(g != w)[:5], g[g != w][:5], w[g != w][:5])


def on_host(tensors):
    return [t.cpu().numpy().view(np.uint16) for t in tensors]


def fill_equals_the_restated_host_loop(k, plan_of):
    """the body of the test of that name; `plan_of(counter, contigs, lenient=False)` makes the plan (tests/test_counts_wide_gpu.py
    runs the same body over plans with 64-bit slot indices)"""
    rng = np.random.default_rng(100 + k)
    g = genome(rng, 4000)
    pool = np.unique(kmers.canonical_codes(windows(g, k), k))
    # several contigs: ragged lists, one without variants, one whose lines all have `nan` flanks, one long (many blocks), one
    # without unique k-mers
    contigs = [contig_of(rng, pool, 37, 6, 30), empty_contig(), contig_of(rng, pool, 20, 9, 0), contig_of(rng, pool, 700, 3, 40),
               contig_of(rng, pool, 50, 0, 5)]
    text = reads_of(rng, g, 500)
    seen = dictionary_counts(text, k)
    with kmers.KmerCounter(k) as counter:
        counter.add_codes(pool)
        counter.count(text)
        with plan_of(counter, contigs) as plan:
            st = plan.stats()
            assert st.n_kmers == sum(c.kmer_code.size for c in contigs) and st.n_flanks == sum(c.flank_code.size for c in contigs)
            assert st.unresolved == 0 and st.device_bytes >= 4 * (st.n_kmers + st.n_flanks)
            assert plan.last_fill_ms() == 0.0
            for coverage in COVERAGES:
                want = restated_fill(contigs, seen, coverage)
                got = plan.fill(coverage)
                assert_same(got[0], want[0], f"fill_host kmer_count at {coverage}")
                assert_same(got[1], want[1], f"fill_host coverage at {coverage}")
                dev = plan.fill_device(coverage)
                assert_same(on_host(dev[0]), want[0], f"fill_device kmer_count at {coverage}")
                assert_same(on_host(dev[1]), want[1], f"fill_device coverage at {coverage}")
            assert plan.last_fill_ms() > 0.0
            # the nan contig gets the given coverage everywhere, the windows were exercised: not every variant fell back
            assert (plan.fill(30)[1][2] == 30).all() and (plan.fill(3)[1][0] != 3).any()
            # host pointers where device arrays are expected are refused on the host
            kc, cv = plan.fill(3)
            import ctypes as C
            n = len(contigs)
            pk = (C.c_void_p * n)(*[a.ctypes.data if a.size else None for a in kc])
            pc = (C.c_void_p * n)(*[a.ctypes.data if a.size else None for a in cv])
            assert kmers._counts().pg_count_plan_fill_device(plan._h, 3, pk, pc) == _lib.PG_ERR_INVALID


@pytest.mark.parametrize("k", [5, 21, 31, 32])
def test_fill_equals_the_restated_host_loop(k):
    fill_equals_the_restated_host_loop(k, kmers.CountPlan)


def named_cases_by_hand(plan_of):
    k = 31
    rng = np.random.default_rng(7)
    many, five, never = (genome(rng, k) for _ in range(3))
    with_n = many[:10] + b"N" + many[11:]
    c_many, c_five, c_never, c_n = kmers.canonical_codes([many, five, never, with_n], k)
    assert c_n == NONE and len({int(c_many), int(c_five), int(c_never)}) == 3
    flanks = [[c_many], [c_never, c_never], [c_five], [c_n, c_five], [c_many, c_five], []]
    contig = kmers.CountContig(np.array([0, 4, 4, 4, 4, 4, 4], np.uint32), np.array([c_many, c_five, c_never, c_n], np.uint64),
                               np.concatenate([[0], np.cumsum([len(f) for f in flanks])]).astype(np.uint64),
                               np.array([x for f in flanks for x in f], np.uint64))
    with kmers.KmerCounter(k) as counter:
        counter.add_codes([c_many, c_five, c_never])
        counter.count((many + b"\n") * 70000 + (five.translate(COMP)[::-1] + b"\n") * 5)
        assert counter.lookup_codes([c_many])[0] == 70000
        with plan_of(counter, [contig]) as plan:
            trunc = 70000 - 65536
            expect = {
                #        many alone  never x2  five alone  N + five    many + five          none
                0:      [0,          0,        0,          0,          0,                   0],      # window [0, 0]: only zeros -> fall-back 0
                1:      [1,          1,        1,          1,          1,                   1],      # [0, 4]: 5 is outside, zeros sum to 0
                3:      [3,          3,        5,          2,          5,                   3],      # [0, 12]: (0 + 5) / 2 = 2
                30:     [30,         30,       30,         30,         30,                  30],     # [7, 120]: all outside
                20000:  [trunc,      20000,    20000,      20000,      trunc,               20000],  # [5000, 80000]: 70000, cast
                70000:  [trunc,      trunc,    trunc,      trunc,      trunc,               trunc],  # [17500, 280000]; the cast of the fall-back
            }
            for coverage, want in expect.items():
                kc, cv = plan.fill(coverage)
                assert kc[0].tolist() == [trunc, 5, 0, 0], coverage
                assert cv[0].tolist() == want, coverage
                kd, cd = plan.fill_device(coverage)
                assert on_host(kd)[0].tolist() == [trunc, 5, 0, 0] and on_host(cd)[0].tolist() == want, coverage


def test_named_cases_by_hand():
    """counts above 65 535 are truncated, not saturated; the window's edges; all flanks outside; all flanks 0; an N"""
    named_cases_by_hand(kmers.CountPlan)


def strict_plan_names_the_first_unregistered_code_and_a_lenient_one_counts_zero(plan_of):
    k = 21
    rng = np.random.default_rng(3)
    g = genome(rng, 600)
    pool = np.unique(kmers.canonical_codes(windows(g, k), k))
    known, unknown = pool[:400], pool[400:]
    a = contig_of(rng, known, 30, 4, 6, n_rate=0.1)
    b = contig_of(rng, known, 40, 4, 6, n_rate=0.1)
    v = int(np.flatnonzero(np.diff(b.flank_off) >= 2)[3])          # a variant with two flanking k-mers or more: its second one
    at = int(b.flank_off[v]) + 1
    b.flank_code[at] = unknown[0]
    later = v + 1 + int(np.flatnonzero(np.diff(b.kmer_off)[v + 1:] > 0)[0])
    b.kmer_code[int(b.kmer_off[later])] = unknown[1]               # a later variant's unique k-mer: not the first
    text = reads_of(rng, g, 200)
    seen = dictionary_counts(text, k)
    for code in unknown:
        seen.pop(int(code), None)                                  # never registered: counts 0 in a lenient plan
    with kmers.KmerCounter(k) as counter:
        counter.add_codes(known)
        counter.count(text)
        with pytest.raises(kmers.KmerCounterError) as e:
            plan_of(counter, [a, b])
        assert e.value.code == _lib.PG_ERR_INVALID
        assert f"contig 1, variant {v}, flanking k-mer {at - int(b.flank_off[v])} (code {int(unknown[0])})" in str(e.value), str(e.value)
        with plan_of(counter, [a, b], lenient=True) as plan:
            assert plan.stats().unresolved == int((b.flank_code == unknown[0]).sum() + (b.kmer_code == unknown[1]).sum()) > 0
            want = restated_fill([a, b], seen, 3)
            got = plan.fill(3)
            assert_same(got[0], want[0], "lenient kmer_count")
            assert_same(got[1], want[1], "lenient coverage")
        # what the host can decide is refused before anything is launched
        for bad in (kmers.CountContig(np.array([0, 2, 1], np.uint32), known[:2], np.zeros(3, np.uint64), known[:0]),
                    kmers.CountContig(np.array([0, 1], np.uint32), np.array([1 << 42], np.uint64), np.zeros(2, np.uint64), known[:0]),
                    kmers.CountContig(np.array([1, 2], np.uint32), known[:2], np.zeros(2, np.uint64), known[:0])):
            with pytest.raises(kmers.KmerCounterError) as e:
                plan_of(counter, [bad], lenient=True)
            assert e.value.code == _lib.PG_ERR_INVALID


def test_strict_plan_names_the_first_unregistered_code_and_a_lenient_one_counts_zero():
    strict_plan_names_the_first_unregistered_code_and_a_lenient_one_counts_zero(kmers.CountPlan)


def test_two_samples_through_one_plan_equal_two_fresh_counters():
    k = 31
    rng = np.random.default_rng(11)
    g = genome(rng, 3000)
    pool = np.unique(kmers.canonical_codes(windows(g, k), k))
    contigs = [contig_of(rng, pool, 120, 5, 24), contig_of(rng, pool, 64, 5, 24)]
    texts = [reads_of(rng, g, 300), reads_of(rng, g[:1500], 400)]
    fresh = []
    for text in texts:
        with kmers.KmerCounter(k) as counter:
            counter.add_codes(pool)
            counter.count(text)
            with kmers.CountPlan(counter, contigs) as plan:
                fresh.append(plan.fill(10))
    assert not np.array_equal(fresh[0][0][0], fresh[1][0][0])
    with kmers.KmerCounter(k) as counter:
        counter.add_codes(pool)
        with kmers.CountPlan(counter, contigs) as plan:
            for text, want in zip(texts, fresh):
                counter.reset_counts()
                counter.count(text, sync=False)   # (a fill waits for everything submitted)
                got = plan.fill(10)
                assert_same(got[0], want[0], "kmer_count of the next sample")
                assert_same(got[1], want[1], "coverage of the next sample")


def test_from_tables_on_the_golden_table():
    """CountPlan.from_tables over the reference's own table and reads: the restated host loop at the fixture's coverage"""
    from pathlib import Path
    golden = Path(__file__).resolve().parent / "golden"
    table = golden / "index_chr1_kmers.tsv.gz"
    contig = kmers.parse_kmer_table(table, 31)
    lines = (golden / "region-reads.fa").read_bytes().split(b"\n")
    text = b"\n".join(lines[1::4]) + b"\n"   # (FASTQ despite its name: the sequence lines)
    seen = dictionary_counts(text, 31)
    with kmers.KmerCounter(31) as counter:
        codes = np.concatenate([contig.kmer_code, contig.flank_code])
        counter.add_codes(codes[codes != np.uint64(NONE)])
        counter.count(text)
        with kmers.CountPlan.from_tables(counter, [table]) as plan:
            assert plan.stats().n_kmers == contig.kmer_code.size and plan.stats().unresolved == 0
            want = restated_fill([contig], seen, 18)
            got = plan.fill(18)
            assert_same(got[0], want[0], "golden kmer_count")
            assert_same(got[1], want[1], "golden coverage")
            assert got[0][0].any()


# ---------------------------------------------------------------------------------------------------------------- cohort job
FIELDS = ("lik", "lik_exp", "kept", "n_kmers", "coverage")


def plan_over(rng, index, pool):
    """a plan with the job's k-mers per variant; which code a k-mer is, and every variant's flanks, are drawn from `pool`"""
    contigs = []
    for b in index:
        V, nf = b.n_variants, rng.integers(0, 25, b.n_variants)
        contigs.append(kmers.CountContig(b.kmer_off.copy(), pool[rng.integers(0, len(pool), int(b.kmer_off[-1]))],
                                         np.concatenate([[0], np.cumsum(nf)]).astype(np.uint64), pool[rng.integers(0, len(pool), int(nf.sum()))]))
    return contigs


def fill_job_equals_an_upload_of_the_host_filled_arrays(paths, plan_of):
    k, S = 21, 3
    rng = np.random.default_rng(paths)
    g = genome(rng, 5000)
    pool = np.unique(kmers.canonical_codes(windows(g, k), k))
    index = [synthetic_panel(V, paths, 12, seed=40 + i, multiallelic_frac=0.1 if i % 2 else 0.0) for i, V in enumerate((150, 90, 260, 40))]
    contigs = plan_over(rng, index, pool)
    table = hmm.ProbabilityTable(*default_table_args())
    params = hmm.make_params(1.26, False, 1e-5)
    zeros = [([np.zeros(b.kmer_count.size, np.uint16) for b in index], [np.full(b.n_variants, 30, np.uint16) for b in index]) for _ in range(S)]
    job = hmm.Job.cohort(index, zeros, table, params)
    with kmers.KmerCounter(k) as counter:
        counter.add_codes(pool)
        with plan_of(counter, contigs) as plan:
            for round_ in range(2):   # the second round: other reads into the same job, after a run
                coverages = [28 + 3 * s + round_ for s in range(S)]
                filled = []
                for s in range(S):
                    counter.reset_counts()
                    counter.count(reads_of(rng, g[1000 * s:1000 * s + 3000], 1500))
                    filled.append(plan.fill(coverages[s]))
                    plan.fill_job(job, s, coverages[s])
                    if s == 0 and round_ == 1:   # the job HAS run: between a fill and the next run a fetch answers an error, not round 0's likelihoods
                        with pytest.raises(hmm.PanGenieError) as e:
                            job.fetch(0)
                        assert "pg_job_run has not been called" in str(e.value)
                assert not np.array_equal(filled[0][0][0], filled[1][0][0])
                want_job = hmm.Job.cohort(index, filled, table, params)
                want_job.run()
                job.run()
                for chain in range(S * len(index)):
                    got, want = job.fetch(chain), want_job.fetch(chain)
                    assert got.n_columns == want.n_columns, chain
                    for f in FIELDS:
                        assert np.array_equal(getattr(got, f), getattr(want, f)), (round_, chain, f)
                    s, c = divmod(chain, len(index))
                    assert np.array_equal(job.fetch_panel(chain).kmer_count, filled[s][0][c]), (round_, chain)
                want_job.close()
            # ---- errors, all decided on the host
            def refused(fill, text):
                with pytest.raises(kmers.KmerCounterError) as e:
                    fill()
                assert e.value.code == _lib.PG_ERR_INVALID and text in str(e.value), str(e.value)
            refused(lambda: plan.fill_job(job, S, 30), f"sample {S} of {S}")
            plain = hmm.Job(index[:1], table, params)
            with plan_of(counter, contigs[:1]) as one:
                refused(lambda: one.fill_job(plain, 0, 30), "not a cohort job")
            plain.close()
            other = [c for c in contigs]
            koff = other[2].kmer_off.copy()
            koff[5] += 1 if koff[5] < koff[6] else -1
            other[2] = other[2]._replace(kmer_off=koff)
            with plan_of(counter, other) as changed:
                refused(lambda: changed.fill_job(job, 0, 30), "contig 2")
            with plan_of(counter, contigs[:3]) as short:
                refused(lambda: short.fill_job(job, 0, 30), "3 contigs")
            job.upload_begin(zeros)
            refused(lambda: plan.fill_job(job, 0, 30), "pg_job_upload_end")
            job.upload_end()
            plan.fill_job(job, 0, 30)
            job.run()
            assert job.fetch(0).n_columns > 0
    job.close()


@pytest.mark.parametrize("paths", [16, 64])
def test_fill_job_equals_an_upload_of_the_host_filled_arrays(paths):
    fill_job_equals_an_upload_of_the_host_filled_arrays(paths, kmers.CountPlan)
