"""Constructed inputs for the Viterbi kernels (pangenie_amd/csrc/pg_viterbi.hip) and a CPU restatement that shows which
kernel condition each of them reaches.  A plain module: tests/test_viterbi_cases.py proves the conditions on the CPU,
tests/test_viterbi_edges_gpu.py runs the same cases on the device.

`restate` is the four-candidate step of tests/test_viterbi_precision.py:viterbi_four_candidates in numpy long double
(the oracle's own arithmetic: emission tables and transition probabilities are the oracle's, columns are divided by
their sum, summed in index order).  Unlike the oracle it returns the STATE path, the backpointers and, per column,
whether the column came out all 0 and how many states had all four products 0.

A case is a `Case`: the batch, the table spec (the format of tests/golden/reference_known_answers.json, applied with
tests/fixtures_util.fill_table) and the regimes (recombrate, effective_N, uniform) it runs in.  Widths mean H paths:
k_viterbi<1> for H <= 16, <2> for H <= 32, <4> for H <= 64.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import pyoracle as orc
from pangenie_amd.panel import (BiallelicUniqueKmers, ContigBatch, MultiallelicUniqueKmers, default_table_args, flatten,
                                synthetic_panel)
from tests.fixtures_util import fill_table

LD = np.longdouble
BC = 32        # columns per staged block (pg_viterbi.hip: VitCfg::BC)
PG_AMAX = 5    # more alleles than this on the paths: a "wide" column (pg_device.h)

# (recombrate, effective_N, uniform): the five regimes of tests/test_viterbi_gpu.py:test_viterbi_vs_oracle
DEFAULT, PRODUCTION, NO_RECOMB, UNIFORM, FIXTURE = ((1.26, 25000.0, False), (1.26, 1e-5, False), (0.0, 25000.0, False),
                                                    (1.26, 25000.0, True), (446.287102628, 0.25, False))
FIVE = (DEFAULT, PRODUCTION, NO_RECOMB, UNIFORM, FIXTURE)
REGIME_NAME = {DEFAULT: "default", PRODUCTION: "production", NO_RECOMB: "q0", UNIFORM: "uniform", FIXTURE: "fixture"}

PANEL_TABLE = {"default": False, "args": list(default_table_args()), "modify": []}


def kernel_k(H):
    """states per lane of the kernel that takes H paths"""
    return 1 if H <= 16 else 2 if H <= 32 else 4


@dataclass
class Case:
    name: str
    batch: ContigBatch
    table: dict = field(default_factory=lambda: PANEL_TABLE)
    regimes: tuple = (PRODUCTION,)
    genotyping: bool = False   # the device also runs it with run_genotyping=True
    want: dict = field(default_factory=dict)   # what tests/test_viterbi_cases.py asserts about it

    @property
    def H(self):
        return self.batch.n_paths


def oracle_table(spec):
    t = orc.OracleTable(default=True) if spec["default"] else orc.OracleTable(*spec["args"])
    return fill_table(t, spec, orc.copynumber_regularized)


def kept_columns(batch):
    """ColumnIndexer (reference src/columnindexer.cpp:8-33): variants at which some path carries a defined ALT"""
    V, H = batch.n_variants, batch.n_paths
    pa = batch.path_allele.reshape(V, H)
    cols = []
    for v in range(V):
        a0 = int(batch.allele_off[v])
        ids = batch.allele_id[a0:int(batch.allele_off[v + 1])]
        undef = {int(a) for a, f in zip(ids, batch.allele_flags[a0:a0 + ids.size]) if f & 1}
        if any(int(a) != 0 and int(a) not in undef for a in pa[v]):
            cols.append(v)
    return np.asarray(cols, np.int64)


def alleles_on_paths(batch, v):
    H = batch.n_paths
    return int(np.unique(batch.path_allele[v * H:(v + 1) * H]).size)


@dataclass
class Restated:
    cols: np.ndarray        # variant of every kept column
    states: np.ndarray      # [C] state i * H + j of the Viterbi path
    back: np.ndarray        # [C, H * H] backpointers (row 0 unused)
    zero_col: np.ndarray    # [C] every entry of the column is 0 (before the uniform fall-back)
    zero_states: np.ndarray  # [C] states whose four products are all 0
    near_rows: np.ndarray   # [C] rows of the PREVIOUS column whose maximum is below the column's by less than 2^-56 of it
    hap1: np.ndarray
    hap2: np.ndarray


def _last_argmax(a, axis):
    n = a.shape[axis]
    return n - 1 - np.argmax(np.flip(a, axis), axis=axis)


def restate(batch, table, regime) -> Restated:
    recomb, eff_n, uniform = regime
    V, H = batch.n_variants, batch.n_paths
    n = H * H
    pa = batch.path_allele.reshape(V, H)
    cols = kept_columns(batch)
    C = cols.size
    back = np.zeros((C, n), np.int64)
    zero_col = np.zeros(C, bool)
    zero_states = np.zeros(C, np.int64)
    near_rows = np.zeros(C, np.int64)
    own = np.arange(n).reshape(H, H)
    prev = None
    for c, v in enumerate(cols):
        E, _ = orc.emission_table(batch, table, int(v))
        ids = batch.allele_id[int(batch.allele_off[v]):int(batch.allele_off[v + 1])].tolist()
        slot = np.asarray([ids.index(int(a)) for a in pa[v]])
        e = E[np.ix_(slot, slot)]
        if c == 0:
            cur = e.copy()
        else:
            t = orc.transition_probs(int(batch.variant_pos[cols[c - 1]]), int(batch.variant_pos[v]), recomb, H, uniform, eff_n)
            rowidx = np.arange(H) * H + _last_argmax(prev, 1)
            colidx = _last_argmax(prev, 0) * H + np.arange(H)
            gidx = n - 1 - int(np.argmax(prev.ravel()[::-1]))
            rm, gm = prev.max(1), prev.max()
            near_rows[c] = int(((rm < gm) & (gm - rm < gm * LD(2.0) ** -56)).sum())
            cand = ((prev * t[0], own),
                    (np.broadcast_to((prev.max(1) * t[1])[:, None], (H, H)), np.broadcast_to(rowidx[:, None], (H, H))),
                    (np.broadcast_to((prev.max(0) * t[1])[None, :], (H, H)), np.broadcast_to(colidx[None, :], (H, H))),
                    (np.full((H, H), prev.max() * t[2], LD), np.full((H, H), gidx)))
            best, bi = np.zeros((H, H), LD), np.zeros((H, H), np.int64)
            for val, idx in cand:  # the reference's scan with >=: of equal values the largest index
                take = (val > best) | ((val == best) & (idx >= bi))
                best, bi = np.where(take, val, best), np.where(take, idx, bi)
            bi = np.where(best == 0, n - 1, bi)  # every product is 0: the scan ends on the last state
            zero_states[c] = int((best == 0).sum())
            back[c] = bi.ravel()
            cur = best * e
        total = np.cumsum(cur.ravel())[-1]  # (in index order, as the reference sums)
        zero_col[c] = not (total > 0)
        prev = cur / total if total > 0 else np.full((H, H), LD(1) / LD(n), LD)
    states = np.zeros(C, np.int64)
    hap1, hap2 = np.zeros(V, np.uint16), np.zeros(V, np.uint16)
    if C:
        s = n - 1 - int(np.argmax(prev.ravel()[::-1]))
        for c in range(C - 1, -1, -1):
            states[c] = s
            if c > 0:
                s = int(back[c, s])
        hap1[cols], hap2[cols] = pa[cols, states // H], pa[cols, states % H]
    return Restated(cols, states, back, zero_col, zero_states, near_rows, hap1, hap2)


# ---------------------------------------------------------------------------------------------------------------------
#  builders
# ---------------------------------------------------------------------------------------------------------------------
def cut_columns(batch, C, lo=0):
    """variants [lo, the C-th kept one at or after lo]: a chain of exactly C kept columns that ends on a kept variant"""
    cols = kept_columns(batch)
    cols = cols[cols >= lo]
    assert cols.size >= C, (cols.size, C)
    return batch.slice(lo, int(cols[C - 1]) + 1)


def with_paths(batch, pa, pos=None):
    return ContigBatch(batch.n_paths, batch.variant_pos if pos is None else pos, batch.coverage, batch.kmer_off,
                       batch.kmer_count, batch.allele_off, batch.allele_id, batch.allele_flags, batch.allele_kmer_off,
                       batch.allele_kmer_mask, np.ascontiguousarray(pa, np.uint16).reshape(-1))


def mosaic_batch(H, V, seed, switches=(), same=False, no_kmers=(), gap=None):
    """Biallelic panel of V kept variants whose sample is a mosaic of panel paths: haplotype 2 follows one path, haplotype
    1 starts on another (`same`: on the same one) and moves to a new path at every variant of `switches`.  The path
    it leaves and the one it enters differ on both sides of the switch, the read counts carry no noise (13 per copy,
    10 k-mers per allele), so the evidence for every switch is worth many recombinations.  `no_kmers`: variants
    without k-mers.  -> (batch, h1, h2)"""
    rng = np.random.default_rng(seed)
    pa = rng.integers(0, 2, size=(V, H)).astype(np.uint16)
    pa[np.arange(V), rng.integers(0, H, V)] = 1   # every variant is kept
    h2 = np.full(V, int(rng.integers(0, H)))
    x = int(h2[0]) if same else int(rng.choice([p for p in range(H) if p != h2[0]]))
    h1 = np.full(V, x)
    for s in sorted(switches):
        y = int(rng.choice([p for p in range(H) if p not in (x, int(h2[0]))]))
        pa[s - 1, y] = 1 - pa[s - 1, x]
        pa[s, x] = 1 - pa[s, y]
        h1[s:] = y
        x = y
    for v in [v for v in (0, V - 1) if v + (v == 0) in switches]:
        # a run of ONE column at either end: only the sample's own path carries its allele there, so no other path
        # can stand in for it and move the change
        a = pa[v, h1[v]]
        pa[v] = 1 - a
        pa[v, h1[v]] = a
    for v in range(V):
        if not pa[v].any():
            pa[v, [p for p in range(H) if p not in (h1[v], h2[v])][0]] = 1
    per = np.full(V, 10)
    per[list(no_kmers)] = 0
    kmer_off = np.concatenate([[0], np.cumsum(2 * per)]).astype(np.uint32)
    rows = np.arange(V)
    copies = np.stack([(pa[rows, h1] == a).astype(int) + (pa[rows, h2] == a) for a in (0, 1)], axis=1)  # [V, 2]
    counts = np.concatenate([np.repeat(13 * copies[v], per[v]) for v in range(V)]) if V else np.zeros(0)
    gaps = rng.integers(50, 1250, V) if gap is None else gap(rng, V)
    pos = 10000 + np.cumsum(gaps)
    batch = ContigBatch(H, pos.astype(np.uint64), np.full(V, 27, np.uint16), kmer_off, counts.astype(np.uint16),
                        2 * np.arange(V + 1, dtype=np.uint32), np.tile([0, 1], V).astype(np.uint16), np.zeros(2 * V, np.uint8),
                        np.stack([np.zeros(V, int), per], axis=1).reshape(-1).astype(np.uint16),
                        np.repeat(np.where(per > 0, (1 << per) - 1, 0), 2).astype(np.uint32), pa.reshape(-1))
    return batch, h1, h2


def runs_from_end(states):
    """lengths of the runs of one state, last run first"""
    s = np.asarray(states)
    cut = np.flatnonzero(np.diff(s)) + 1
    return np.diff(np.concatenate([[0], cut, [s.size]]))[::-1].tolist()


# ---- a. kept-column counts
COLUMN_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 97)


@functools.lru_cache(maxsize=None)
def _family_a_panel(H):
    return synthetic_panel(140, H, 20, seed=9100 + H, multiallelic_frac=0.2)


def family_a():
    return [Case("a_H%d_C%d" % (H, C), cut_columns(_family_a_panel(H), C), regimes=(PRODUCTION, DEFAULT), genotyping=True,
                 want={"C": C})
            for H in (7, 16, 20, 32, 40, 64) for C in COLUMN_COUNTS]


# ---- b. backtrace edges: `runs` are the run lengths of the state path from the last column down
def family_b():
    out = []
    for H in (6, 30, 64):
        for name, V, switches, runs in (("nochange_C129", 129, (), [129]),          # r == 64 twice, C - 1 = 2 * 64
                                        ("run64_last", 100, (36,), [64, 36]),        # the change is seen by lane 63
                                        ("run65_last", 100, (35,), [65, 35]),        # r == 64, then lane 0 sees the change
                                        ("ends_and_mid", 200, (1, 70, 135, 199), [1, 64, 65, 69, 1])):
            # (ends_and_mid: the first seed from 4000 on at which no other pair of paths explains the sample as well with
            # a change one column off — with 6 paths that happens)
            seed = {6: 4006, 30: 4000, 64: 4000}[H] if name == "ends_and_mid" else 4000 + 10 * H + V + len(switches)
            b, _, _ = mosaic_batch(H, V, seed, switches)
            out.append(Case("b_H%d_%s" % (H, name), b, want={"runs": runs}))
        # a span without k-mers (emission 1 everywhere) across the walk's 64-column step
        b, _, _ = mosaic_batch(H, 129, 4500 + H, (90,), no_kmers=range(40, 80))
        out.append(Case("b_H%d_nokmer_span" % H, b, want={"runs": [39, 90]}))
        # uniform transitions: every backpointer is the previous column's last maximum, the state changes wherever the
        # likeliest pair of paths does
        b, _, _ = mosaic_batch(H, 65, 4600 + H, (20, 40))
        out.append(Case("b_H%d_uniform" % H, b, regimes=(UNIFORM,), want={"changes_at_least": 2, "C": 65}))
    return out


# ---- c. exact zeros
ZERO_TABLE = {"default": False, "args": [0, 1, 11, 0.0], "modify": [[0, 10, [0.0, 1.0, 0.0]], [0, 0, [1.0, 0.0, 0.0]]]}


def zero_batch(H, kinds):
    """One variant per entry of `kinds`, over the table of the reference's emissions_zero fixture (a k-mer read 10 times
    lies on exactly one of the two haplotypes, one never read on neither).  With A = paths [0, H/2), B = [H/4, 3H/4):
      XA / XB  ALT on the paths of A / B, one ALT k-mer read 10 times: states with exactly ONE path in the set
      ZA       ALT on the paths of A, its k-mer never read: states with NO path in A (none of those XA allows)
      U        three alleles, allele 2 on no path, its k-mer read 10 times: 0 for every pair of paths, yet not an
               all-zero table (which would count as all 1): the column is 0 whatever the transitions are"""
    A, B = range(0, H // 2), range(H // 4, 3 * H // 4)
    uks = []
    for v, kind in enumerate(kinds):
        alt = B if kind == "XB" else A
        p2a = [1 if p in alt else 0 for p in range(H)]
        if kind == "U":
            u = MultiallelicUniqueKmers(1000 + 500 * v, p2a)
            u.insert_kmer(10, [2])
        else:
            u = BiallelicUniqueKmers(1000 + 500 * v, p2a)
            u.insert_kmer(0 if kind == "ZA" else 10, [1])
        u.set_coverage(0)
        uks.append(u)
    return flatten(uks)


def zero_layout(C, by_disjoint, by_table):
    """kinds of C columns: ZA right after XA at `by_disjoint` (0 when q == 0), U at `by_table` (0 always), XA / XB in
    turn elsewhere — compatible with each other, so the chain stays alive between the zero columns"""
    kinds = ["XA" if c % 2 == 0 else "XB" for c in range(C)]
    for c in by_disjoint:
        kinds[c - 1], kinds[c] = "XA", "ZA"
    for c in by_table:
        kinds[c] = "U"
    return kinds


# With q == 0 every backpointer into a zero column is the last state and the last state points to itself, so the path
# before the LAST zero column is the last state whatever the kernel computed; what the haplotypes check there is the stretch
# after it (and, in the fixture's regime, all stretches between the zero columns of the table kind).
ZERO_LAYOUTS = {  # C, zero by disjoint neighbours, zero by the table
    "mid_31_last": (40, (8, 31, 39), (10, 32)),
    "mid_32_live_tail": (39, (8, 32), (20,)),
    "table_31_last": (34, (12,), (31, 33)),
}


def family_c():
    out = []
    for H in (9, 16, 24, 32, 40, 64):
        for name, (C, dis, tab) in ZERO_LAYOUTS.items():
            out.append(Case("c_H%d_%s" % (H, name), zero_batch(H, zero_layout(C, dis, tab)), table=ZERO_TABLE,
                            regimes=(NO_RECOMB, FIXTURE), genotyping=True,
                            want={"C": C, "zero": {NO_RECOMB: sorted(dis + tab), FIXTURE: sorted(tab)}}))
    return out


# ---- d. wide columns
WIDE_V = 70
WIDE_AT = (0, 1, 31, 32, 33, 50, WIDE_V - 1)


def family_d():
    """Wide objects at the variants of columns WIDE_AT.  At those variants path p carries allele (p + column) mod A (A =
    9 .. 12 alleles in the object), so that every one of them has min(H, A) > PG_AMAX alleles on the paths whatever the draw
    of the allele frequency was; the read counts stay those of the panel's own sample."""
    out = []
    for H in (12, 16, 24, 48, 64):
        kw = dict(seed=9300 + H, multiallelic_frac=0.2, undefined_frac=0.0)
        cols = kept_columns(synthetic_panel(2 * WIDE_V, H, 20, **kw))   # (wide objects change no other draw)
        b = synthetic_panel(2 * WIDE_V, H, 20, wide_at=cols[list(WIDE_AT)], wide_alleles=(9, 12), **kw)
        pa = b.path_allele.reshape(-1, H).copy()
        for c in WIDE_AT:
            v = int(cols[c])
            pa[v] = (np.arange(H) + c) % int(b.allele_off[v + 1] - b.allele_off[v])
        out.append(Case("d_H%d_wide" % H, cut_columns(with_paths(b, pa), WIDE_V), regimes=(PRODUCTION, DEFAULT), genotyping=True,
                        want={"C": WIDE_V, "wide": WIDE_AT}))
    return out


# ---- e. ties
def windowed_gaps(H):
    """distance / H in [39.5, 41.5] under the reference's default effective_N (tests/test_viterbi_precision.py): p and q
    agree to all 53 bits of a double and differ by 35+ ulps of a long double"""
    return lambda rng, V: 314 * H + rng.integers(0, 15 * H, size=V)


def family_e():
    out = []
    dup = {"dup16_halves": (16, lambda pa: np.concatenate([pa[:, :8], pa[:, :8]], 1)),
           "dup32_halves": (32, lambda pa: np.concatenate([pa[:, :16], pa[:, :16]], 1)),
           "dup64_inlane": (64, lambda pa: np.repeat(pa[:, ::4], 4, axis=1)),             # paths 4j .. 4j+3 identical
           "dup64_plus16": (64, lambda pa: np.concatenate([pa[:, :16], pa[:, :16], pa[:, 32:48], pa[:, 32:48]], 1))}
    for name, (H, f) in dup.items():
        b = synthetic_panel(120, H, 20, seed=9500 + H + len(name), zero_kmer_frac=0.2)
        pa = np.asarray(f(b.path_allele.reshape(120, H)))
        out.append(Case("e_" + name, with_paths(b, pa), regimes=(DEFAULT, PRODUCTION), want={"dup": True}))
    for H in (16, 32, 64):
        b = synthetic_panel(70, H, 20, seed=9600 + H)
        pa = np.repeat(b.path_allele.reshape(70, H)[:, :1], H, axis=1)
        out.append(Case("e_H%d_all_identical" % H, with_paths(b, pa), regimes=(DEFAULT, PRODUCTION), want={"last_state": True}))
    for H in (10, 28, 64):
        b, _, _ = mosaic_batch(H, 70, 9700 + H, same=True)
        out.append(Case("e_H%d_diagonal" % H, b, want={"diagonal": True}))
    for H in (16, 32, 64):
        b = synthetic_panel(100, H, 20, seed=9800 + H, multiallelic_frac=0.2)
        cols = kept_columns(b)
        pos = b.variant_pos.copy()
        for lo, hi in ((31, 32), (63, 65)):  # gaps of 0 into columns 32, 64 and 65: q == 0 for those steps only
            pos[cols[lo]:cols[hi] + 1] = pos[cols[lo]]
        out.append(Case("e_H%d_equal_positions" % H, with_paths(b, b.path_allele, pos), regimes=(DEFAULT, PRODUCTION),
                        want={"gap0": (32, 64, 65)}))
    # rows whose maxima agree in the high double and differ below it (the second pass over lo of the global maximum): path
    # p + H/2 is path p from variant 1 on, so a state and its twin differ by "stayed" against "switched once"
    for H in (16, 32, 64):
        b, _, _ = mosaic_batch(H, 60, 9900 + H, (30,), gap=windowed_gaps(H))
        pa = b.path_allele.reshape(60, H).copy()
        pa[1:, H // 2:] = pa[1:, :H // 2]
        out.append(Case("e_H%d_twins_below_fp64" % H, with_paths(b, pa), regimes=(DEFAULT,), want={"near_tie": True}))
    return out


# ---- f. widths
def family_f():
    out = []
    for H in (1, 2, 15, 17, 31, 33, 48, 63):
        b = synthetic_panel(200 if H > 2 else 900, H, 20, seed=9000 + H, multiallelic_frac=0.2)
        out.append(Case("f_H%d" % H, cut_columns(b, 150), regimes=FIVE, want={"C": 150}))
    return out


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f}


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [c for f in FAMILIES.values() for c in f()]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def oracle_result(name, regime, form=1):
    """the oracle's phasing of a case, computed once per session and shared"""
    case = next(c for c in all_cases() if c.name == name)
    recomb, eff_n, uniform = regime
    return orc.viterbi_contig(case.batch, oracle_table(case.table),
                              orc.make_params(recomb, uniform, eff_n, run_genotyping=False, run_phasing=True), form=form)
