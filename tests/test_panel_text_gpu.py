"""The sampled panel's haplotype columns on the device (pg_panel_text_from_paths, pg_job_panel_text, pg_job_panel_lines and their
fetches; k_ptpanel_* of pangenie_amd/csrc/pg_panel_text.hip, the slotted joiner of pg_record_lines.hip) against the Python mirror
of the rule (tests/panel_util.py).  The unit entry point on constructed plans of 1-4 records a bubble with three-digit indices,
R in {1, 255, 256, 257, 1025} x P in {1, 2, 17, 64}, with guard bytes and the bound reached exactly; jobs over synthetic_panel
with random_plan at 16 and 30 paths before and after a run, a chain without a kept column whose lines carry the panel's own UK,
a pg_sampler_then_job chain over pg_job_fetch_panel; a sampled cohort of 3 samples x 2 contigs whose lines are the plain join of
a slotted prefix, the UK and its own text, the packed fetches and the device pointers; every refusal and staleness rule; 65
paths.  The join and the rule have no arithmetic: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib, calls, hmm
from pangenie_amd import sampler as smp
from pangenie_amd.panel import synthetic_panel, synthetic_sample_counts
from tests.panel_util import joined, mirror_text, mirror_uk
from tests.record_calls_util import random_plan

pytestmark = pytest.mark.gpu
ARGS = (6, 108, 54, 0.01)
SEED = 10400
NS, NC = 3, 2


# ---- the unit entry point ----------------------------------------------------------------------------------------------
def constructed_plan(rng, R):
    """bubbles of 1-4 records until R records are there; every fifth bubble has 130-256 alleles, all but a few defined, mapped
    one to one: indices of three digits.  Answers (plan, ids per bubble)."""
    bubbles, n_ids, left = [], [], R
    while left:
        n_rec = min(left, int(rng.integers(1, 5)))
        wide = len(bubbles) % 5 == 0
        ids = int(rng.integers(130, 257)) if wide else int(rng.integers(2, 13))
        records = []
        for j in range(n_rec):
            if wide and j == 0:
                own, nA = list(range(ids)), ids
            else:
                nA = int(rng.integers(1, min(ids, 6) + 1))
                own = [0] + rng.integers(0, nA, ids - 1).tolist()
            records.append((own, [True] + [bool(x) for x in rng.random(nA - 1) >= 0.1]))
        bubbles.append(records)
        n_ids.append(ids)
        left -= n_rec
    return calls.RecordPlan.from_records(bubbles), np.array(n_ids)


@pytest.mark.parametrize("P", [1, 2, 17, 64])
@pytest.mark.parametrize("R", [1, 255, 256, 257, 1025])
def test_the_unit_entry_point_on_constructed_plans(R, P):
    rng = np.random.default_rng(SEED + 100 * R + P)
    plan, n_ids = constructed_plan(rng, R)
    pa = (rng.random((plan.n_variants, P)) * n_ids[:, None]).astype(np.uint16)
    if R >= 255:
        pa[0, :] = n_ids[0] - 1   # (the widest index of the first bubble on every path)
    want_off, want = mirror_text(plan, P, pa)
    if R >= 255:   # three digits
        assert any(len(c) == 3 for r in range(R) for c in want[int(want_off[r]):int(want_off[r + 1])].split(b"\t"))
    # raw: guard bytes behind off[R] and behind the text
    cap = calls.panel_text_bound(R, P)
    off = np.full(R + 1 + 4, 0xABABABABABABABAB, np.uint64)
    text = np.full(cap + 64, 0xCD, np.uint8)
    c = plan.as_c()
    rc = _lib.load_hip().pg_panel_text_from_paths(0, C.addressof(c), P, pa.ctypes.data, off.ctypes.data, text.ctypes.data, cap)
    assert rc == 0
    assert off[:R + 1].astype(np.int64).tolist() == want_off.tolist()
    assert text[:len(want)].tobytes() == want
    assert (off[R + 1:] == 0xABABABABABABABAB).all() and (text[len(want):] == 0xCD).all()
    assert len(want) <= cap
    got = calls.panel_text_from_paths(plan, P, pa)
    assert got[1] == want and got[0].astype(np.int64).tolist() == want_off.tolist()


@pytest.mark.parametrize("P", [1, 17, 64])
def test_the_bound_is_reached_exactly_by_all_255_cells(P):
    R = 300
    plan = calls.RecordPlan.from_records([[(list(range(256)), [True] * 256)] for _ in range(R)])
    pa = np.full((R, P), 255, np.uint16)
    off, text = calls.panel_text_from_paths(plan, P, pa)
    assert len(text) == calls.panel_text_bound(R, P) == R * (4 * P - 1)
    assert text == b"".join([b"\t".join([b"255"] * P)] * R) and np.diff(off.astype(np.int64)).tolist() == [4 * P - 1] * R


# ---- jobs --------------------------------------------------------------------------------------------------------------
def random_prefix(rng, R, slotted=True):
    lens = rng.integers(0, 80, R)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    kind = rng.integers(0, 3, R)
    slot = np.where(kind == 0, 0, np.where(kind == 1, lens, (rng.random(R) * (lens + 1)).astype(np.int64))).astype(np.uint32)
    return off, rng.integers(0, 256, int(off[-1]), dtype=np.uint8), slot if slotted else None


def check_chain(job, c, plan, text, batch=None):
    b = batch if batch is not None else job.fetch_panel(c)
    want_off, want = mirror_text(plan, b.n_paths, b.path_allele)
    assert text[0].astype(np.int64).tolist() == want_off.tolist() and text[1] == want, ("text of chain", c)
    return want


def refused(call, *args, code=-1):
    with pytest.raises(hmm.PanGenieError) as e:
        call(*args)
    assert e.value.code == code


@pytest.mark.parametrize("H", [16, 30])
def test_a_job_before_and_after_its_run_gives_the_same_bytes(H):
    b = synthetic_panel(60, H, 20, seed=SEED + H, multiallelic_frac=0.3, zero_kmer_frac=0.1)
    plan = random_plan(np.random.default_rng(SEED + 1), b, undefined=0.3)
    job = hmm.Job([b], hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    job.record_plan(0, plan)
    before = job.panel_text(0)   # no run yet
    assert job.panel_text_ms() > 0.0
    want = check_chain(job, 0, plan, before, b)
    assert b"." in want and b"\t" in want
    job.run()
    assert calls.fetch_panel_text(job, 0)[1] == want   # a run does not make it stale
    after = job.panel_text(0)
    assert after[1] == before[1] and after[0].tolist() == before[0].tolist()
    assert len(job.record_text(0)[1]) > 0 and calls.fetch_panel_text(job, 0)[1] == want   # the record text is its own family
    job.close()


def test_a_chain_without_a_kept_column_prints_the_panels_own_uk_and_a_contig_without_a_plan_is_left_out():
    flat = synthetic_panel(60, 16, 20, seed=SEED + 20, multiallelic_frac=0.3)
    flat.path_allele[:] = 0   # every path carries the reference allele: no column is kept
    batches = [flat, synthetic_panel(60, 16, 20, seed=SEED + 21, multiallelic_frac=0.3), synthetic_panel(40, 16, 20, seed=SEED + 22)]
    job = hmm.Job(batches, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    job.run()
    res = job.fetch(0)
    assert res.n_columns == 0 and not np.asarray(res.n_kmers).any()   # pg_job_fetch's rule answers 0 ...
    rng = np.random.default_rng(SEED + 23)
    plans = [random_plan(rng, batches[0]), random_plan(rng, batches[1])]
    prefixes = [random_prefix(rng, p.n_records) for p in plans]
    for c in (0, 1):   # (contig 2 has no plan)
        job.record_plan(c, plans[c])
        job.panel_line_prefix(c, prefixes[c][0], prefixes[c][1], slot=prefixes[c][2])
    texts = job.panel_text()
    assert len(texts[2][1]) == 0 and texts[2][0].tolist() == [0]   # left out, not an error
    lines = job.panel_lines()
    assert len(lines) == 3 and len(lines[2][1]) == 0
    for c in (0, 1):
        check_chain(job, c, plans[c], texts[c], batches[c])
        uk = mirror_uk(plans[c], batches[c].kmer_off)
        want = joined(prefixes[c], uk, texts[c])
        assert lines[c][1] == want[1] and lines[c][0].astype(np.int64).tolist() == want[0].tolist(), c
    assert mirror_uk(plans[0], flat.kmer_off).max() >= 10   # ... the lines of chain 0 carry the panel's count, not 0
    assert texts[0][1].replace(b"\t", b"") == b"0" * (16 * plans[0].n_records)
    uk = calls.fetch_panel_uk_packed(job)
    assert uk.tolist() == np.concatenate([mirror_uk(plans[c], batches[c].kmer_off) for c in (0, 1)]).tolist()
    off, text, rf, tf = job.panel_text_packed()
    assert tf[2] == tf[3] == len(text) and rf.tolist() == [0, plans[0].n_records, plans[0].n_records + plans[1].n_records, plans[0].n_records + plans[1].n_records]
    assert text == texts[0][1] + texts[1][1] and int(off[-1]) == len(text)
    job.close()


@pytest.mark.parametrize("add_reference", [False, True])
def test_a_sampler_then_job_chain_against_the_panel_it_holds(add_reference):
    panels = [synthetic_panel(200, 24, 20, seed=SEED + 30 + c, multiallelic_frac=0.3, max_alleles=8, zero_kmer_frac=0.05) for c in range(2)]
    t, p = hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5)
    job, _, _ = smp.sample_then_job(panels, 7, t, p, add_reference=add_reference)
    rng = np.random.default_rng(SEED + 31)
    plans = [random_plan(rng, ix, undefined=0.3) for ix in panels]   # (over the ids of the full panels: the reduced ones keep them)
    for c in range(2):
        job.record_plan(c, plans[c])
    texts = job.panel_text()
    for c in range(2):
        held = job.fetch_panel(c)
        assert held.n_paths == 7 + int(add_reference)
        check_chain(job, c, plans[c], texts[c], held)
    job.close()


@pytest.fixture(scope="module")
def cohort():
    index = [synthetic_panel(300, 40, 20, seed=SEED + 40 + c, multiallelic_frac=0.3, max_alleles=8, zero_kmer_frac=0.05) for c in range(NC)]
    samples = []
    for s in range(NS):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=SEED + 50 + NC * s + c) for c, ix in enumerate(index)])
        samples.append((list(kcs), list(covs)))
    job, _, _ = smp.sample_cohort(index, samples, 15, hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5), add_reference=True, want_paths=False)
    assert job.n_chains == NS * NC and all(b.n_paths == 16 for b in job.batches)
    rng = np.random.default_rng(SEED + 41)
    plans = [random_plan(rng, ix, undefined=0.3) for ix in index]
    prefixes = [random_prefix(rng, p.n_records) for p in plans]
    for c in range(NC):
        job.record_plan_strided(c, NC, plans[c])
        job.panel_line_prefix_strided(c, NC, prefixes[c][0], prefixes[c][1], slot=prefixes[c][2])
    yield job, index, plans, prefixes
    job.close()


def lines_of(packed, ix):
    off, text, line_first, byte_first = packed
    l0, l1, b0, b1 = int(line_first[ix]), int(line_first[ix + 1]), int(byte_first[ix]), int(byte_first[ix + 1])
    return off[l0:l1 + 1].astype(np.int64) - b0, text[b0:b1]


def test_a_sampled_cohorts_text_lines_packed_fetches_and_device_pointers(cohort):
    job, index, plans, prefixes = cohort
    texts = job.panel_text()   # (the job has not run)
    held = [job.fetch_panel(g) for g in range(NS * NC)]
    for g in range(NS * NC):
        check_chain(job, g, plans[g % NC], texts[g], held[g])
    assert texts[0][1] != texts[NC][1]   # (the reduced panels differ per sample)
    off, text, rf, tf = job.panel_text_packed()
    assert text == b"".join(t for _, t in texts)
    assert tf.tolist() == np.concatenate([[0], np.cumsum([len(t) for _, t in texts])]).tolist()
    assert rf.tolist() == np.concatenate([[0], np.cumsum([plans[g % NC].n_records for g in range(NS * NC)])]).tolist()
    assert off.tolist() == np.concatenate([o[:-1].astype(np.int64) + int(tf[g]) for g, (o, _) in enumerate(texts)] + [[int(tf[-1])]]).tolist()
    assert len(text) <= sum(calls.panel_text_bound(plans[g % NC].n_records, 16) for g in range(NS * NC))
    # the lines: slotted prefix, the panel's own UK, the chain's own text
    packed = job.panel_lines_packed()
    assert job.panel_lines_ms() > 0.0
    uks, n_bytes = [], 0
    for g in range(NS * NC):
        uk = mirror_uk(plans[g % NC], held[g].kmer_off)
        want = joined(prefixes[g % NC], uk, texts[g])
        got = lines_of(packed, g)
        assert got[0].tolist() == want[0].tolist() and got[1] == want[1], g
        one = calls.fetch_panel_lines(job, g)
        assert one[1] == want[1] and one[0].astype(np.int64).tolist() == want[0].tolist()
        uks.append(uk)
        n_bytes += len(want[1])
    assert len(packed[1]) == n_bytes
    for c in range(NC):   # otherwise one prefix with the number in its bytes would do
        assert any((uks[c] != uks[s * NC + c]).any() for s in range(1, NS)), c
    assert calls.fetch_panel_uk_packed(job).tolist() == np.concatenate(uks).tolist()
    lib, err = job._lib, C.create_string_buffer(256)
    d0 = None
    for g in range(NS * NC):
        d_off, d_text, n_rec, n_b = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        assert lib.pg_job_device_panel_text(job.h, g, C.byref(d_off), C.byref(d_text), C.byref(n_rec), C.byref(n_b)) == 0
        assert n_rec.value == plans[g % NC].n_records and n_b.value == len(texts[g][1]) and d_off.value and d_text.value
        assert lib.pg_job_device_panel_lines(job.h, g, C.byref(d_off), C.byref(d_text), C.byref(n_rec), C.byref(n_b)) == 0
        assert n_rec.value == plans[g % NC].n_records and n_b.value == int(packed[3][g + 1] - packed[3][g]) and d_off.value
        d0 = d_text.value if g == 0 else d0
        assert d_text.value - d0 == int(packed[3][g])
    assert lib.pg_job_device_panel_text(job.h, NS * NC, None, None, None, None) == -1 and lib.pg_job_device_panel_lines(job.h, NS * NC, None, None, None, None) == -1
    buf = np.zeros(len(text) + 8, np.uint8)
    assert lib.pg_job_fetch_panel_text_packed(job.h, None, buf.ctypes.data, len(text) + 1, err, 256) == -1   # not the buffer's length
    assert lib.pg_job_fetch_panel_text(job.h, 1, None, buf.ctypes.data, len(texts[1][1]), err, 256) == 0 and buf[:len(texts[1][1])].tobytes() == texts[1][1]
    assert lib.pg_job_fetch_panel_lines_packed(job.h, None, buf.ctypes.data, len(packed[1]) + 1, err, 256) == -1
    assert lib.pg_job_fetch_panel_uk_packed(job.h, buf.ctypes.data, int(rf[-1]) + 1, err, 256) == -1
    # the run changes nothing: the same bytes, and the families of the record text stand beside these
    job.run()
    assert calls.fetch_panel_text_packed(job)[1] == text and calls.fetch_panel_lines_packed(job)[1] == packed[1]
    assert job.panel_text_packed()[1] == text and job.panel_lines_packed()[1] == packed[1]
    refused(job.record_lines)   # (no record text, and no prefixes of that family)


def test_staleness_a_new_prefix_a_text_formed_again_a_new_plan(cohort):
    job, index, plans, prefixes = cohort
    texts = job.panel_text()
    before = [lines_of(job.panel_lines_packed(), g) for g in range(NS * NC)]
    d = C.c_void_p()
    # the text formed again: the lines are stale although the bytes are the same
    job.panel_text()
    refused(calls.fetch_panel_lines, job, 0)
    refused(calls.fetch_panel_lines_packed, job)
    assert job._lib.pg_job_device_panel_lines(job.h, 0, C.byref(d), None, None, None) == -1
    assert [lines_of(job.panel_lines_packed(), g)[1] for g in range(NS * NC)] == [b[1] for b in before]
    # a new prefix on one stride: the lines alone; a plain one prints no UK
    other = random_prefix(np.random.default_rng(SEED + 60), plans[1].n_records, slotted=False)
    job.panel_line_prefix_strided(1, NC, other[0], other[1])
    refused(calls.fetch_panel_lines, job, 0)
    assert calls.fetch_panel_text(job, 1)[1] == texts[1][1]
    packed = job.panel_lines_packed()
    for g in range(NS * NC):
        want = before[g][1] if g % NC == 0 else joined(other, None, texts[g])[1]
        assert lines_of(packed, g)[1] == want, g
    # pg_job_panel_line_prefix on one member changes that member alone
    mine = random_prefix(np.random.default_rng(SEED + 61), plans[1].n_records)
    job.panel_line_prefix(NC + 1, mine[0], mine[1], slot=mine[2])
    packed = job.panel_lines_packed()
    assert lines_of(packed, NC + 1)[1] == joined(mine, mirror_uk(plans[1], job.fetch_panel(NC + 1).kmer_off), texts[NC + 1])[1]
    assert lines_of(packed, 1)[1] == joined(other, None, texts[1])[1]
    # a new plan: text and lines, and the stride's prefixes are dropped
    new = random_plan(np.random.default_rng(SEED + 62), index[1], undefined=0.3)
    job.record_plan_strided(1, NC, new)
    refused(calls.fetch_panel_text, job, 0)
    refused(calls.fetch_panel_text_packed, job)
    refused(calls.fetch_panel_uk_packed, job)
    refused(calls.form_panel_lines, job)   # (it does not form the text itself)
    assert job._lib.pg_job_device_panel_text(job.h, 0, C.byref(d), None, None, None) == -1
    again = job.panel_text()
    for g in range(NS * NC):
        check_chain(job, g, new if g % NC else plans[0], again[g])
    assert again[0][1] == texts[0][1] and again[1][1] != texts[1][1]
    packed = job.panel_lines_packed()
    assert lines_of(packed, 0)[1] == before[0][1] and len(lines_of(packed, 1)[1]) == 0   # (no prefix any more: left out)
    job.record_plan_strided(1, NC, plans[1])   # (as the other tests of the module expect it)
    job.panel_line_prefix_strided(1, NC, prefixes[1][0], prefixes[1][1], slot=prefixes[1][2])
    assert [t for _, t in job.panel_text()] == [t for _, t in texts]
    assert [lines_of(job.panel_lines_packed(), g)[1] for g in range(NS * NC)] == [b[1] for b in before]


def test_stale_after_a_new_index_and_panel():
    b = synthetic_panel(60, 16, 20, seed=SEED + 70, multiallelic_frac=0.3)
    plan = random_plan(np.random.default_rng(SEED + 71), b, undefined=0.3)
    prefix = random_prefix(np.random.default_rng(SEED + 72), plan.n_records)
    job = hmm.Job([b], hmm.ProbabilityTable(*ARGS), hmm.make_params(1.26, False, 1e-5))
    job.record_plan(0, plan)
    job.panel_line_prefix(0, prefix[0], prefix[1], slot=prefix[2])
    text = job.panel_text(0)
    lines = job.panel_lines(0)
    assert lines[1] == joined(prefix, mirror_uk(plan, b.kmer_off), text)[1]
    job.upload()   # a plain job sends every array again, the index and the panel too
    refused(calls.fetch_panel_text, job, 0)
    refused(calls.fetch_panel_lines, job, 0)
    refused(calls.form_panel_lines, job)
    assert job.panel_text(0)[1] == text[1]   # (the ids are checked again, the plan stands)
    assert len(job.panel_lines(0)[1]) == 0   # the index's prefix was dropped with it: the contig is left out ...
    job.panel_line_prefix(0, prefix[0], prefix[1], slot=prefix[2])
    assert job.panel_lines(0)[1] == lines[1]   # ... until its fixed columns are sent again
    job.close()


def test_refusals_and_the_limit_of_64_paths():
    b = synthetic_panel(40, 16, 20, seed=SEED + 80, multiallelic_frac=0.3)
    t = hmm.ProbabilityTable(*ARGS)
    plan = random_plan(np.random.default_rng(SEED + 81), b)
    job = hmm.Job([b], t, hmm.make_params(1.26, False, 1e-5))
    refused(calls.fetch_panel_text, job, 0)   # nothing formed
    refused(job.panel_lines)                  # ... and no text to join
    texts = job.panel_text()                  # no plan: every chain is left out
    assert len(texts[0][1]) == 0
    lib, err = job._lib, C.create_string_buffer(256)
    prefix = random_prefix(np.random.default_rng(SEED + 82), plan.n_records)
    assert lib.pg_job_panel_line_prefix(job.h, 0, prefix[0].ctypes.data, prefix[1].ctypes.data, err, 256) == -1   # no plan on the contig
    job.record_plan(0, plan)
    first = job.panel_text(0)
    check_chain(job, 0, plan, first, b)
    assert lib.pg_job_panel_line_prefix(job.h, 1, prefix[0].ctypes.data, prefix[1].ctypes.data, err, 256) == -1   # no such index contig
    assert lib.pg_job_panel_line_prefix(job.h, 0, None, prefix[1].ctypes.data, err, 256) == -1
    bad = prefix[0].copy()
    bad[0] = 1
    assert lib.pg_job_panel_line_prefix(job.h, 0, bad.ctypes.data, prefix[1].ctypes.data, err, 256) == -1
    far = (np.diff(prefix[0].astype(np.int64)) + 1).astype(np.uint32)
    assert lib.pg_job_panel_line_prefix_slotted(job.h, 0, prefix[0].ctypes.data, prefix[1].ctypes.data, far.ctypes.data, err, 256) == -1   # a slot behind its prefix
    assert lib.pg_job_panel_line_prefix_strided(job.h, 0, 0, prefix[0].ctypes.data, prefix[1].ctypes.data, None, err, 256) == -1
    assert lib.pg_job_panel_line_prefix_strided(job.h, 1, 1, prefix[0].ctypes.data, prefix[1].ctypes.data, None, err, 256) == -1
    job.panel_line_prefix(0, prefix[0], prefix[1], slot=prefix[2])
    assert job.panel_lines(0)[1] == joined(prefix, mirror_uk(plan, b.kmer_off), first)[1]
    # an allele id of the index outside a record's map: the id check runs before the first formation under the new plan
    job.record_plan(0, calls.RecordPlan.from_records([[([0], [True])] for _ in range(40)]))
    refused(job.panel_text)
    job.record_plan(0, plan)
    assert job.panel_text(0)[1] == first[1]
    job.close()
    # 65 paths: not formed on the device; 64 are
    for H, code in ((65, -3), (64, None)):
        w = synthetic_panel(30, H, 20, seed=SEED + 83 + H)
        job = hmm.Job([w], t, hmm.make_params(1.26, False, 1e-5))
        wp = random_plan(np.random.default_rng(SEED + 84), w)
        job.record_plan(0, wp)
        if code is not None:
            refused(job.panel_text, code=code)
            refused(calls.fetch_panel_text, job, 0)
        else:
            check_chain(job, 0, wp, job.panel_text(0), w)
        job.close()
