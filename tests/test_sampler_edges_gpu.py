"""The sampler kernels (pangenie_amd/csrc/pg_sampler.hip) on the branches no seeded random panel reaches: the 1024-column
jump and the second stay dword of ks_backtrack_fast, every instantiation of ks_forward_fast / ks_forward, batches of mixed
width, more than KS_MAXPASS passes, allele lists at the 254 / 256 boundaries, the limits of ku_count / ku_write, and the
strict tie rule.  Every panel is built directly as a ContigBatch.  The bar is exact: sampled paths and best scores equal
oracle.pyoracle.sampler_run, reduced panels equal ContigBatch.update_paths field for field.  Every test asserts which
kernel ran (waves per workgroup of the fast kernel, 0 = general) and, ON THE ORACLE'S OUTPUT, the property that makes its
input reach the branch, so that a later change of a helper or a seed cannot quietly lose the reach."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc  # checker only
from pangenie_amd import hmm
from pangenie_amd import panel as pn
from pangenie_amd import sampler as smp
from tests.test_sampled_cohort_gpu import PANEL_FIELDS, PARAMS, TABLE, check_cohort, draw_samples

pytestmark = pytest.mark.gpu

# read counts of an allele's own k-mers by the emission cost they give (present = count >= 3): all present 0, one of two
# -10 log10f(1/2) = 3, none 25; an undefined allele costs 50 whatever its k-mers
COST_KMERS = {0: [10], 3: [10, 0], 25: [0], 50: [10]}
KS_MAXPASS, KS_BT_BLOCK = 64, 32   # pg_sampler.hip


def build(P, pos, cols, extra_kmers=None):
    """cols: per column (alleles, row): alleles = [(allele id, emission cost)] in listed order, row = allele of every
    path.  Each allele gets one or two k-mers of its own (COST_KMERS); extra_kmers[c] more k-mers on no allele."""
    koff, kc, aoff, aid, fl, ako, akm, rows, want = [0], [], [0], [], [], [], [], [], []
    for c, (alleles, row) in enumerate(cols):
        k = 0
        for a, cost in alleles:
            cnt = COST_KMERS[cost]
            aid.append(a); fl.append(int(cost == 50)); ako.append(k); akm.append((1 << len(cnt)) - 1)
            kc += cnt
            k += len(cnt)
            want.append(cost)
        extra = (extra_kmers or {}).get(c, 0)
        kc += [0] * extra
        koff.append(koff[-1] + k + extra)
        aoff.append(aoff[-1] + len(alleles))
        rows.append(np.asarray(row, np.uint16))
    V = len(cols)
    b = pn.ContigBatch(P, np.asarray(pos, np.uint64), np.full(V, 20, np.uint16), koff, kc, aoff, aid, fl, ako, akm,
                       np.concatenate(rows) if rows else np.zeros(0, np.uint16))
    assert orc.sampler_emission_costs(b).tolist() == want     # the costs the construction means, as the oracle forms them
    return b


def random_panel(P, V, seed, a_hi=3):
    """Seeded panel of 2..a_hi alleles per column with costs from 0 / 3 / 25 (2 % undefined), every path a random allele."""
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(V):
        A = int(rng.integers(2, a_hi + 1))
        costs = [50 if rng.random() < 0.02 else int(rng.choice([0, 3, 25])) for _ in range(A)]
        cols.append((list(zip(range(A), costs)), rng.integers(0, A, P)))
    return build(P, 1000 + np.cumsum(rng.integers(1, 3000, V)), cols)


def runs(path):
    """(start, length, path id) of every run of a sampled path"""
    path = np.asarray(path)
    starts = np.concatenate([[0], np.flatnonzero(np.diff(path)) + 1])
    return [(int(s), int(e - s), int(path[s])) for s, e in zip(starts, np.concatenate([starts[1:], [path.size]]))]


def assert_sampler(b, size, o_paths, o_best, kernel, **kw):
    h = smp.HaplotypeSampler(b, size, **kw)
    assert h.kernel == kernel
    assert h.best_scores == o_best.tolist()
    assert np.array_equal(h.sampled, o_paths)


def use_kernel(monkeypatch, kernel):
    if kernel == "general":
        monkeypatch.setenv("PG_SAMPLER_KERNEL", "general")
    else:
        monkeypatch.delenv("PG_SAMPLER_KERNEL", raising=False)


# --------------------------------------------------------------------------- #
#  A. long runs and block edges of the fast backtrace
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def long_run_case(P, hot, leave, join, V, s):
    """Two alleles per column, 1500 bp apart.  Path `hot` carries allele 1 (cost 0) everywhere, `leave` carries it on the
    columns before s, `join` from s on; every other cell carries allele 0 (cost 25; undefined, 50, in the first and the
    last column, so that one column of the cheap allele pays for a recombination).  Pass 0 stays on `hot` for all V
    columns; pass 1 (allele 1 now at 10, `hot` masked) runs on `leave` and switches to `join` at column s exactly.
    (A joining path that merely TIES with the rest before s is traced back along itself: no switch would be recorded.)"""
    rows = np.zeros((V, P), np.uint16)
    rows[:, hot] = 1
    rows[:s, leave] = 1
    rows[s:, join] = 1
    cols = [([(0, 50 if c in (0, V - 1) else 25), (1, 0)], rows[c]) for c in range(V)]
    b = build(P, 1000 + 1500 * np.arange(V), cols)
    return b, orc.sampler_run(b, 3)


def long_run_reach(case, hot, leave, join, V, s):
    _, (o_paths, o_best) = case
    assert runs(o_paths[0]) == [(0, V, hot)] and o_best[0] == 0                 # one run of V >= 1025 columns: the jump
    assert runs(o_paths[1]) == [(0, s, leave), (s, V - s, join)]               # the switch column
    assert max(n for p in o_paths for _, n, _ in runs(p)) >= 1025


LONG_LAYOUTS = [            # P, hot, leave, join: paths per lane, waves and the stay word the long trace reads
    (64, 7, 3, 12),         # PPL = 1
    (100, 70, 90, 5),       # PPL = 2, the high half word
    (256, 70, 130, 200),    # PPL = 4: dword 0 high half; pass 1: dword 1 low half, then dword 1 high half
    (256, 130, 200, 70),
    (256, 200, 70, 130),
    (300, 260, 290, 130),   # NW = 2 (T = 128): ids >= 2T read the second dword
]
LONG_SWITCHES = ([(2100, s, None) for s in (1, 16, 17, 1024, 1025, 1026, 2099)] +
                 [(2097, 2096, None), (2097, 1025, None), (2098, 2097, None), (2098, 1024, None)] +
                 # the edges of the jumps themselves (jump_lo): pass 1 is traced down from V - 1 without a switch until s
                 [(2100, 1089, "edge1"), (2100, 1088, "below1"), (2100, 1073, "below1"), (2100, 65, "edge2"), (2100, 64, "below2"),
                  (2100, 48, "below2"), (2100, 33, "below2"), (2097, 1073, "edge1"), (2097, 1072, "below1"), (2097, 1057, "below1"),
                  (2098, 1089, "edge1"), (2098, 1088, "below1"), (2098, 1073, "below1")])


def jump_lo(cur):
    """The lowest column of the 64 blocks of 16 that one step of ks_backtrack_fast inspects from column cur down: where a
    step that finds no switch ends."""
    blk = (cur - 1) // 16
    return (blk - 63) * 16 + 1 if blk >= 63 else 1


def jump_reach(V, s, where):
    """The switch column against the block arithmetic of the jumps: the trace of pass 1 runs V - 1 - s columns down from
    V - 1 before it meets the switch at s.  edge1 / edge2: s is the last column the first / second step inspects, so the
    switch is found in the lowest bit of its last lane; below1 / below2: s lies in the one / two blocks right below, which
    the step must NOT assign: a `lo` one block too low assigns them unseen and loses the switch (one block too HIGH only
    inspects a block twice and changes no output)."""
    lo1 = jump_lo(V - 1)
    lo2 = jump_lo(lo1 - 1)
    assert lo1 > 1024 and lo2 > 1 and V - 1 - lo1 >= 1008 and lo1 - 1 - lo2 == 1023
    if where == "edge1":
        assert s == lo1 and V - 1 - s == 16 * 63 + (V - 2) % 16
    elif where == "below1":
        assert lo1 - 16 <= s < lo1
    elif where == "edge2":
        assert s == lo2
    elif where == "below2":
        assert lo2 - 32 <= s < lo2


@pytest.mark.parametrize("V,s,where", LONG_SWITCHES)
@pytest.mark.parametrize("P,hot,leave,join", LONG_LAYOUTS)
def test_long_runs_and_block_edges(P, hot, leave, join, V, s, where, monkeypatch):
    """ks_backtrack_fast: the `sw == 0` jump over 1024 columns (blk_cur >= 63 and below), the stay word of every quarter of
    the path ids, a switch at the first / last bit of a block of 16, around column 1024, in the last column with and without
    a partial last block ((V - 1) % 16 = 3, 0, 1), and at the column a jump ends on and in the blocks right below it."""
    use_kernel(monkeypatch, "fast")
    assert V <= 2200 and (2097 - 1) % 16 == 0 and (2098 - 1) % 16 == 1
    case = long_run_case(P, hot, leave, join, V, s)
    long_run_reach(case, hot, leave, join, V, s)
    if where:
        assert runs(case[1][0][1])[1][:2] == (s, V - s)      # the oracle's pass 1 switches at s: the trace comes down V - 1 - s columns
        jump_reach(V, s, where)
    T = 64 * (2 if P > 256 else 1)
    assert P <= 64 or hot >= 64
    assert P < 256 or max(hot, leave, join) >= 2 * T                           # a long trace on an id >= 2T: the second stay dword
    b, (o_paths, o_best) = case
    assert_sampler(b, 3, o_paths, o_best, kernel=2 if P > 256 else 1)


# --------------------------------------------------------------------------- #
#  B. every instantiation
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def top_ids_case(P, V, size):
    """The cheapest paths at the top ids, so that a lost tail shows: allele 1 (cost 0) lies on P-1 and P-2 in alternating
    segments of 16 columns (on P-1 alone below 32 columns), allele 2 (cost 3) on P-3 everywhere and, in a few columns each,
    on a sprinkling of the other paths from id 0 on; the rest is allele 0 (cost 25).  Pass 0 follows allele 1, pass 1 is P-3."""
    rows = np.zeros((V, P), np.uint16)
    for c in range(V):
        rows[c, np.arange(c % 7, P - 3, 7 * V)] = 2
        rows[c, P - 3] = 2
        rows[c, P - 1 if V < 32 or (c // 16) % 2 == 0 else P - 2] = 1
    cols = [([(0, 25), (1, 0), (2, 3)], rows[c]) for c in range(V)]
    b = build(P, 1000 + 1500 * np.arange(V), cols)
    return b, orc.sampler_run(b, size)


def top_ids_reach(case, P, V):
    _, (o_paths, o_best) = case
    want0 = [(s, min(16, V - s), P - 1 if (s // 16) % 2 == 0 else P - 2) for s in range(0, V, 16)] if V >= 32 else [(0, V, P - 1)]
    if V >= 32 and V % 16 == 1:     # one last column of the cheap allele does not pay for a recombination
        want0[-2:] = [(want0[-2][0], 17, want0[-2][2])]
    assert runs(o_paths[0]) == want0
    assert runs(o_paths[1]) == [(0, V, P - 3)] and o_best[1] == 3 * V


@pytest.mark.parametrize("P,V,size,forced,kernel", [
    (2049, 40, 3, None, 16),           # ks_forward_fast<16,4>: block_min reads 16 wave minima from one row
    (4096, 33, 2, None, 16),
    (257, 65, 3, "general", 0),        # ks_forward<1024,1>; three LDS blocks of the backtrace
    (1024, 40, 2, "general", 0),       # ... and the widest panel whose backtrace blocks fit into LDS
    (1025, 40, 3, "general", 0),       # ks_forward<1024,4>; the backtrace reads global memory
    (4096, 35, 2, "general", 0),
    (4097, 20, 3, None, 0),            # ks_forward<1024,16>, chosen by the width
    (16385, 3, 2, None, 0),            # ks_forward<1024,64>
    (65534, 3, 3, None, 0),
])
def test_every_instantiation(P, V, size, forced, kernel, monkeypatch):
    use_kernel(monkeypatch, forced)
    case = top_ids_case(P, V, size)
    top_ids_reach(case, P, V)
    if V == 65:
        assert V > 2 * KS_BT_BLOCK and len(runs(case[1][0][0])) >= 3     # switches in more than one LDS block
    b, (o_paths, o_best) = case
    assert_sampler(b, size, o_paths, o_best, kernel)


# --------------------------------------------------------------------------- #
#  C. mixed widths in one call
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def mixed_index():
    return (random_panel(2, 70, 31), random_panel(5, 130, 32, 4), random_panel(600, 90, 33, 4), random_panel(130, 45, 34, 5),
            random_panel(9, 5, 35).slice(0, 0))


@pytest.mark.parametrize("kernel,code", [("fast", 4), ("general", 0)])
@pytest.mark.parametrize("size,first", [(1, 0), (4, 1)])
def test_mixed_widths_in_one_call(size, first, kernel, code, monkeypatch):
    """T and the paths per lane come from the widest contig (600 paths: NW = 4): the 2-, 5- and 130-path contigs run at
    T = 256 with almost every cost word masked.  One pass over all of them (a 2-path contig has no second one), four
    passes over the rest."""
    use_kernel(monkeypatch, kernel)
    batches = list(mixed_index())[first:]
    assert [b.n_paths for b in mixed_index()] == [2, 5, 600, 130, 9] and batches[-1].n_variants == 0
    sampled, best = smp.sample_contigs(batches, size)
    assert smp.last_ms()[1] == code
    for b, s, bs in zip(batches, sampled, best):
        if b.n_variants == 0:
            assert s.shape == (size, 0)
            continue
        o_paths, o_best = orc.sampler_run(b, size)
        assert len(runs(o_paths[0])) >= 2                       # the oracle's path recombines: more than a column minimum
        assert np.array_equal(s, o_paths) and bs.tolist() == o_best.tolist(), b.n_paths


@pytest.mark.parametrize("kernel,code", [("fast", 4), ("general", 0)])
@pytest.mark.parametrize("size,first", [(1, 0), (4, 1)])
def test_mixed_widths_cohort(size, first, kernel, code, monkeypatch):
    """The same index through sample_cohort with two samples: against sample_then_job alone, the oracle and the host's
    update_paths (check_cohort, unchanged)."""
    use_kernel(monkeypatch, kernel)
    index = list(mixed_index())[first:]
    samples = draw_samples(index, 2, 50 + size)
    job, _, _ = smp.sample_cohort(index, samples, size, hmm.ProbabilityTable(*TABLE), hmm.make_params(*PARAMS), add_reference=True)
    assert smp.last_ms()[1] == code                           # the cohort call's own choice, read before any other call
    job.close()
    check_cohort(index, samples, size, True, hmm.make_params(*PARAMS), oracle=True)


# --------------------------------------------------------------------------- #
#  D. more than KS_MAXPASS passes
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("kernel,code", [("fast", 1), ("general", 0)])
@pytest.mark.parametrize("size,reads_paths", [(64, False), (65, False), (66, True), (70, True)])
def test_more_than_64_passes(size, reads_paths, kernel, code, monkeypatch):
    """The general kernel keeps the picks of KS_MAXPASS passes in LDS and reads the later ones from d.paths: the pass with
    index KS_MAXPASS + 1 (size 66) is the first to read one; 64 and 65 passes are the boundary below."""
    use_kernel(monkeypatch, kernel)
    b = random_panel(72, 20, 41, 4)
    o_paths, o_best = orc.sampler_run(b, size)
    assert (size - 1 > KS_MAXPASS) == reads_paths             # the last pass masks a pick of a pass >= KS_MAXPASS
    assert size >= KS_MAXPASS and all(len(set(o_paths[:, c].tolist())) == size for c in range(20))   # every pick masks a cell
    assert_sampler(b, size, o_paths, o_best, code)


# --------------------------------------------------------------------------- #
#  E. allele-list widths
# --------------------------------------------------------------------------- #
WIDE_P, WIDE_V = 8, 6


@functools.lru_cache(maxsize=None)
def wide_case(A):
    """Every other column lists A alleles, most of them on no path: the paths carry the LAST listed one (the cheapest: 3)
    or allele 1 (25); the columns between have two alleles (25 / 0).  Path 6 is the one that always carries the cheap
    allele; the lower ids carry the expensive one, so an allele that is not found (cost 0) moves the answer."""
    last_on = {0: (5, 6), 2: (6, 7), 4: (3, 6)}
    cols = []
    for c in range(WIDE_V):
        row = np.ones(WIDE_P, np.uint16) if c % 2 == 0 else np.zeros(WIDE_P, np.uint16)
        if c % 2 == 0:
            row[list(last_on[c])] = A - 1
            cols.append(([(a, 3 if a == A - 1 else 25) for a in range(A)], row))
        else:
            row[[2, 6]] = 1
            cols.append(([(0, 25), (1, 0)], row))
    b = build(WIDE_P, 1000 + 1500 * np.arange(WIDE_V), cols)
    return b, orc.sampler_run(b, 3)


def wide_reach(case, A):
    b, (o_paths, o_best) = case
    assert int(np.diff(b.allele_off).max()) == A
    assert runs(o_paths[0]) == [(0, WIDE_V, 6)] and o_best[0] == 9            # 3 per wide column: the last allele's cost counts
    pa = b.path_allele.reshape(WIDE_V, WIDE_P)
    for c in range(0, WIDE_V, 2):                                              # ... and it sits in the last slot of its list
        assert b.allele_id[b.allele_off[c + 1] - 1] == pa[c, 6] == A - 1
    assert len({int(p) for p in o_paths[1:].ravel()} - {6}) >= 2


@pytest.mark.parametrize("A,kernel", [(254, 1), (255, 0), (256, 0), (257, 0), (300, 0)])
def test_allele_list_widths(A, kernel, monkeypatch):
    """ks_slots stops at 254 listed alleles, contig_tcost sends wider columns to the general kernel, whose LDS tables hold
    256 and which reads global memory beyond."""
    use_kernel(monkeypatch, None)
    case = wide_case(A)
    wide_reach(case, A)
    b, (o_paths, o_best) = case
    assert_sampler(b, 3, o_paths, o_best, kernel)
    if A == 254:                                                               # the general kernel on the same panel
        use_kernel(monkeypatch, "general")
        assert_sampler(b, 3, o_paths, o_best, 0)


def test_fast_kernel_refuses_255_alleles(monkeypatch):
    monkeypatch.setenv("PG_SAMPLER_KERNEL", "fast")
    b = wide_case(255)[0]
    with pytest.raises(RuntimeError, match=r"outside the fast kernel's bounds \(error -3\)"):
        smp.HaplotypeSampler(b, 3)
    b, (o_paths, o_best) = wide_case(254)
    assert_sampler(b, 3, o_paths, o_best, 1)


@functools.lru_cache(maxsize=None)
def windows_contig():
    """A variant of 212 k-mers: seven alleles whose windows start 30 k-mers apart and spread four k-mers over all 32
    positions (bits 0, 7, 19, 31), between two plain variants."""
    rng = np.random.default_rng(61)
    P, A, bits = 12, 7, (0, 7, 19, 31)
    K = 30 * (A - 1) + 32
    mask = sum(1 << x for x in bits)
    koff = [0, 2, 2 + K, 4 + K]
    kc = np.concatenate([[10, 0], rng.choice([0, 10], K), [0, 10]])
    aoff = [0, 2, 2 + A, 4 + A]
    aid = [0, 1] + list(range(A)) + [0, 1]
    ako = [0, 1] + [30 * a for a in range(A)] + [0, 1]
    akm = [1, 1] + [mask] * A + [1, 1]
    rows = np.concatenate([rng.integers(0, 2, P), rng.integers(0, A, P), rng.integers(0, 2, P)])
    b = pn.ContigBatch(P, np.array([1000, 2500, 4000], np.uint64), np.full(3, 20, np.uint16), koff, kc, aoff, aid, np.zeros(4 + A, np.uint8),
                       ako, akm, rows)
    assert int(np.diff(b.kmer_off).max()) == 212 > 64 * 3
    return b


def check_then_job(panels, size, add_reference, kernel):
    t, p = hmm.ProbabilityTable(*TABLE), hmm.make_params(*PARAMS)
    job, sampled, best = smp.sample_then_job(panels, size, t, p, add_reference=add_reference)
    assert smp.last_ms()[1] == kernel
    job.run()
    got = job.fetch_all()
    for g, b in enumerate(panels):
        o_paths, o_best = orc.sampler_run(b, size)
        assert np.array_equal(sampled[g], o_paths) and best[g].tolist() == o_best.tolist(), g
        rows = np.vstack([o_paths, np.zeros((1, b.n_variants), np.uint32)]) if add_reference else o_paths
        host, dev = b.update_paths(rows), job.batches[g]
        assert dev.n_paths == host.n_paths == size + int(add_reference)
        for f in PANEL_FIELDS:
            assert np.array_equal(getattr(dev, f), getattr(host, f)), (g, f)
        # the job fetched: the columns the oracle's HMM forms over the host's panel (none where one allele is left)
        ref = orc.genotype_contig(host, orc.OracleTable(*TABLE), orc.make_params(*PARAMS))
        assert got[g].n_columns == ref.n_columns > 0 and np.array_equal(got[g].kept, ref.kept), g
    job.close()


@pytest.mark.parametrize("widths,kernel", [((254,), 1), ((254, 255, 256, 257, 300), 0)])
@pytest.mark.parametrize("add_reference", [False, True])
def test_wide_lists_through_the_panel_reduction(widths, kernel, add_reference, monkeypatch):
    """ku_count / ku_write on variants of more than 64 alleles and more than 64 k-mers (the second and later ballot rounds),
    kept alleles in the last slot, windows of 32: the reduced panel is the host's update_paths, and the job fetches."""
    use_kernel(monkeypatch, None)
    panels = [wide_case(A)[0] for A in widths] + [windows_contig()]
    for A in widths:
        wide_reach(wide_case(A), A)
    w = windows_contig()
    o_paths, _ = orc.sampler_run(w, 3)
    kept = w.update_paths(o_paths)
    assert int(np.diff(kept.kmer_off)[1]) >= 8 and int(kept.allele_kmer_off[kept.allele_off[1]:kept.allele_off[2]].max()) > 0
    check_then_job(panels, 3, add_reference, kernel)


def test_panel_reduction_refusals(monkeypatch):
    """The three PG_ERR_UNSUPPORTED refusals of pg_sampler_then_job, each followed by a valid call."""
    use_kernel(monkeypatch, None)
    t = hmm.ProbabilityTable(*TABLE)
    good = wide_case(254)[0]

    def valid():
        job, sampled, _ = smp.sample_then_job([good], 3, t)
        assert np.array_equal(sampled[0], wide_case(254)[1][0])
        job.run()
        assert job.fetch(0).n_columns == WIDE_V
        job.close()

    def refused(fn, text):
        with pytest.raises(hmm.PanGenieError) as e:
            fn()
        assert e.value.code == -3 and text in str(e.value)
        valid()

    row = np.array([0, 1024, 0, 1], np.uint16)
    many_alleles = build(4, [1000, 2500], [([(a, 25 if a < 1024 else 0) for a in range(1025)], row), ([(0, 25), (1, 0)], row % 2)])
    assert int(np.diff(many_alleles.allele_off).max()) == 1025
    refused(lambda: smp.sample_then_job([good, many_alleles], 2, t), "more than 1024 alleles or 2048 k-mers")
    many_kmers = build(4, [1000, 2500], [([(0, 25), (1, 0)], row % 2)] * 2, extra_kmers={1: 2047})
    assert int(np.diff(many_kmers.kmer_off).max()) == 2049
    refused(lambda: smp.sample_then_job([many_kmers, good], 2, t), "more than 1024 alleles or 2048 k-mers")
    refused(lambda: smp.sample_then_job([good], 1024, t, add_reference=True), "at most 1024 kept paths")
    # one inside each bound passes: 1024 alleles, 2048 k-mers
    ok_alleles = build(4, [1000, 2500], [([(a, 25 if a < 1023 else 0) for a in range(1024)], np.minimum(row, 1023)), ([(0, 25), (1, 0)], row % 2)])
    ok_kmers = build(4, [1000, 2500], [([(0, 25), (1, 0)], row % 2)] * 2, extra_kmers={1: 2046})
    check_then_job([ok_alleles, ok_kmers], 2, True, 0)


# --------------------------------------------------------------------------- #
#  F. exact ties
# --------------------------------------------------------------------------- #
def gap_with_cost(P, cost):
    for gap in range(1, 8000):
        if orc.sampler_transition_cost(1000, 1000 + gap, 1.26, P) == cost:
            return gap
    raise AssertionError(f"no gap with recombination cost {cost} at {P} paths")


@functools.lru_cache(maxsize=None)
def tie_case(P, seed):
    """Every recombination costs exactly 25 and every emission 0 or 25: all values are multiples of 25, so cells whose own
    path costs exactly min + t — where the reference switches: it stays only if same < min + t — are everywhere."""
    rng = np.random.default_rng(seed)
    V, gap = 24, gap_with_cost(P, 25)
    rows = (rng.random((V, P)) < 0.3).astype(np.uint16)
    b = build(P, 1000 + gap * np.arange(V), [([(0, 25), (1, 0)], rows[c]) for c in range(V)])
    return b, orc.sampler_run(b, 3, allele_penalty=25)


def tie_reach(case, P):
    """Pass 0 again in numpy (no masks, no penalties yet), to find on the oracle's path the columns of an exact tie."""
    b, (o_paths, o_best) = case
    V, t = b.n_variants, 25
    assert all(orc.sampler_transition_cost(b.variant_pos[c - 1], b.variant_pos[c], 1.26, P) == t for c in range(1, V))
    assert all(smp.SamplingTransitions(int(b.variant_pos[c - 1]), int(b.variant_pos[c]), 1.26, P).cost == t for c in range(1, V))
    e = np.where(b.path_allele.reshape(V, P) == 1, 0, 25).astype(np.int64)
    val = np.zeros((V, P), np.int64)
    val[0] = e[0]
    for c in range(1, V):
        first = int(np.argmin(val[c - 1]))                                   # the lowest id of the smallest value
        others = np.full(P, val[c - 1, first])
        others[first] = np.delete(val[c - 1], first).min()
        val[c] = np.minimum(val[c - 1], others + t) + e[c]
    p = o_paths[0].astype(np.int64)
    assert val[-1].min() == o_best[0] and int(np.argmin(val[-1])) == p[-1]
    ties = [c for c in range(1, V) if p[c] != p[c - 1] and val[c - 1, p[c]] == val[c - 1].min() + t]
    assert len(ties) >= 2                                                     # the path switches where staying costs exactly min + t
    # at one of them several cells hold the minimum the path switches to, and the one it takes — the lowest id of THOSE — is
    # neither path 0 nor the lowest id of the cells involved: cells that stay level at min + t have lower ids
    def target_among_ties(c):
        level, low = np.flatnonzero(val[c - 1] == val[c - 1].min() + t), np.flatnonzero(val[c - 1] == val[c - 1].min())
        return low.size >= 2 and p[c - 1] == low[0] > 0 and level.min() < p[c - 1]
    assert any(target_among_ties(c) for c in ties)


@pytest.mark.parametrize("kernel", ["fast", "general"])
@pytest.mark.parametrize("P,seed,nw", [(100, 2, 1), (300, 3, 2)])
def test_exact_ties(P, seed, nw, kernel, monkeypatch):
    """`dd < 0` in fast_column and `same < previous_cell` in ks_forward: staying costs exactly min + t."""
    use_kernel(monkeypatch, kernel)
    case = tie_case(P, seed)
    tie_reach(case, P)
    b, (o_paths, o_best) = case
    assert_sampler(b, 3, o_paths, o_best, nw if kernel == "fast" else 0, allele_penalty=25)
