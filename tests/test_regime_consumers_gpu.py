"""Every per-variant consumer on the bins of the regime jobs (tests/regime_consumers.py: six families by the route the consumers
take, each under the five regimes of tests/transition_regimes.py, two of them also without regularisation, and tie_job): k_calls,
k_rcalls, k_rplan_ids, k_rgl, k_rtext_*, k_rlines_*, k_combine, k_ccalls, k_crcalls, k_crgl and their _wide forms had met job-made
bins at make_params(1.26, False, 1e-5) with the regularised table only.  Here the job route — the descriptor per chain, DevContig's
kept / allele_present / n_cols / cov / kmer_off, a cohort's chain -> index contig, one record plan per index contig, text -> lines,
combine groups — carries variants whose bins are all zero, exact ties, posteriors flat enough for a GQ of 0 .. 30, and whatever
the device leaves to the host in the middle of a chain's packed text.

Per case: the job under the family's environment, the kernels its plan must name, run() and fetch_all(); then
  2. calls() against the long-double yardstick on the job's OWN bins (tests/calls_util.py); regularisation 0: every kept variant
     whose bins are all zero is PG_CALL_NONE, and the variants the construction put them at are among them, and the variant whose
     bins lie below 2^-16300 is PG_CALL_DEFERRED; tie_job: every tie is PG_CALL_NOT_UNIQUE (or deferred), never a call;
  3. a random plan per index contig: record_calls() and record_gl() against tests/record_calls_util.py / record_gl_util.py, the
     packed fetches equal to the per-chain ones;
  4. record_text() with ignore_imputed off and on, byte for byte against tests/record_text_util.expected_text on the fetched
     fields; the records of length 0 are exactly those the fields predict (a deferred call, a deferred value, fewer than three
     values), and where a chain has a deferred call or value some record of three or more values has length 0;
  5. a random prefix per index contig: record_lines() is prefix + '\\t' + every member's text + '\\n', and — DESIGN.md 4e-7 — a line
     has length 0 exactly if any member's text of that record has;
  6. cohorts and tie_job: a combine plan with a group of three chains over one index contig and a singleton (the 40-allele cohort
     has two chains: its pair, then its singletons); the combined bins, their calls, record calls and record GLs against
     tests/combine_util.py / combined_records_util.py, PG_COMBINED_DEFERRED where the rule says;
  7. end to end, GT and GQ: the device's per-variant and per-record calls — a deferred one as the host rule finishes it on the
     device's bins — equal the yardstick's on the ORACLE's bins for everything regime_consumers.unstable does not leave out (at
     most 1 %: tests/test_regime_consumers_cpu.py); where prob_wrong is a few 2^-64 quanta, GT equal and GQ among the values
     rounding can give (regime_consumers.gq_allowed: 10000, 192, 189 ...; how many: the record of the run).  Per case 0.1 - 1.3 s.  GL values stay on
     the own-bins comparison: log10(1 - 1e-13) has no digit that survives a 1e-6 change of the bins;
  8. a second run() and a second pass over 2 - 5 give the same bytes.
Every case's census, flag counts, deferred values, empty texts and lines, left-out records and GQ histogram go through log_parity
(profiles/r30_regime_consumers.txt is one run's output).  All five regimes run for the 40-allele family: a case of it takes 0.36 s,
long-double yardstick included.
Reference: src/genotypingresult.cpp:118-210, src/graph.cpp:217-273, src/variant.cpp:357-384, src/hmm.cpp:333-380."""
import numpy as np
import pytest

from pangenie_amd import calls, hmm
from tests import regime_consumers as rc
from tests import transition_regimes as tr
from tests.calls_util import DEFERRED, NONE, NOT_UNIQUE, OK, assert_calls, yardstick_of_result
from tests.combine_util import assert_bins, calls_yardstick, combined_yardstick
from tests.combined_records_util import records_yardstick
from tests.parity_util import log_parity
from tests.record_calls_util import assert_record_calls, record_yardstick
from tests.record_gl_util import assert_record_gl, is_deferred, record_gl_yardstick
from tests.record_text_util import assert_text, expected_text
from tests.test_record_lines_gpu import joined

pytestmark = pytest.mark.gpu
CASES = rc.cases()


def _new_job(monkeypatch, case):
    e = rc.env(case)
    for var, val in (("PG_SWEEP_MODE", e.mode), ("PG_KERNELS", e.kernels), ("PG_CHUNK_COLS", e.chunk_cols), ("PG_PIECE_CHUNKS", e.piece_chunks)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    index, samples, chains = rc.job_of(case)
    table, params = rc.table_of(case, hmm.ProbabilityTable), hmm.make_params(*tr.regime_params(case[1]))
    job = hmm.Job(list(index), table, params) if samples is None else hmm.Job.cohort(list(index), samples, table, params)
    return job, index, chains


def _as_call(rec):
    """a device record as the yardstick states it: (allele_1, allele_2, gq) or None for ./."""
    return (int(rec["allele_1"]), int(rec["allele_2"]), int(rec["gq"])) if (int(rec["flags"]) & 0xFF) == OK else None


def _members(case, n_chains, k):
    return [c for c in range(n_chains) if rc.index_of_chain(case, c) == k]


def _consume(job, case, plans, prefixes, check):
    """steps 2 - 5 (and 7 when `check`): -> (every byte the consumers gave, in one list; the statistics of the pass)"""
    chains = job.batches
    n_chains = len(chains)
    out, st = [], dict(none=0, not_unique=0, deferred=0, rec_deferred=0, gl_deferred=0, empty_text=[0, 0], empty_text_beyond_few=[0, 0],
                       empty_lines=[0, 0], variants_left_out=0, records_left_out=0, gq=[0, 0, 0, 0])
    results = job.fetch_all()
    # 2. calls
    recs = job.calls()
    # 3. record calls and record GLs
    rcalls, rgl = job.record_calls(), job.record_gl()
    packed, first = job.record_calls_packed()
    assert packed.tobytes() == b"".join(r.tobytes() for r in rcalls) and first.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rcalls])]).tolist()
    packed, first = job.record_gl_packed()
    assert packed.tobytes() == b"".join(g.tobytes() for g in rgl) and first.tolist() == np.concatenate([[0], np.cumsum([len(g) for g in rgl])]).tolist()
    out += [r.tobytes() for r in recs] + [r.tobytes() for r in rcalls] + [g.tobytes() for g in rgl]
    has_deferred = [False] * n_chains
    for c, (b, res) in enumerate(zip(chains, results)):
        plan = plans[rc.index_of_chain(case, c)]
        fl = recs[c]["flags"]
        has_deferred[c] = bool((fl == DEFERRED).any() or ((rcalls[c]["flags"] & 0xFF) == DEFERRED).any() or is_deferred(rgl[c]).any())
        st["none"], st["not_unique"], st["deferred"] = st["none"] + int((fl == NONE).sum()), st["not_unique"] + int((fl == NOT_UNIQUE).sum()), st["deferred"] + int((fl == DEFERRED).sum())
        st["rec_deferred"] += int(((rcalls[c]["flags"] & 0xFF) == DEFERRED).sum())
        st["gl_deferred"] += int(is_deferred(rgl[c]).sum())
        if not check:
            continue
        what = (rc.case_id(case), "chain", c)
        want = yardstick_of_result(b, res)
        assert_calls(recs[c], want, what)
        go = b.geno_off.astype(np.int64)
        nonzero = np.add.reduceat(np.concatenate([res.lik != 0, [False]]).astype(np.int64), go[:-1])[:b.n_variants] > 0
        all_zero = np.asarray(res.kept, bool) & ~nonzero
        assert (fl[all_zero] == NONE).all(), what
        oa = rc.oracle_answers(case)[c]
        assert np.array_equal(all_zero, oa.all_zero), what
        if case[2] == 0.0:
            targets = [t - 1 for t in rc.zero_targets(job.index[rc.index_of_chain(case, c)])]
            assert all_zero[targets].all() and int(all_zero.sum()) >= 5, what
        if case[0] == rc.TIE:
            ties = list(rc.tie_job()[4][c])
            assert np.isin(fl[ties], (NOT_UNIQUE, DEFERRED)).all(), (what, fl[ties])
        args = (b.allele_off, b.allele_id, res.kept, res.allele_present, res.lik, res.lik_exp, plan)
        want_r = record_yardstick(*args)
        assert_record_calls(rcalls[c], want_r, what)
        assert_record_gl(rgl[c], calls.record_gl_offsets(plan), record_gl_yardstick(*args), what)
        # 7. end to end: the oracle's bins decide; a deferred record is the host's, finished on the device's bins
        mine = [want[v] if int(fl[v]) == DEFERRED else _as_call(recs[c][v]) for v in range(b.n_variants)]
        bad = [(v, mine[v], oa.calls[v], oa.gq_allowed[v]) for v in range(b.n_variants) if not oa.unstable[v] and not rc.same_call(mine[v], oa.calls[v], oa.gq_allowed[v])]
        assert not bad, (what, "per variant, against the oracle's bins", bad[:10])
        mine_r = [(want_r[r] and want_r[r][:3]) if (int(rcalls[c]["flags"][r]) & 0xFF) == DEFERRED else _as_call(rcalls[c][r]) for r in range(plan.n_records)]
        bad = [(r, mine_r[r], oa.rec_calls[r], oa.rec_gq_allowed[r]) for r in range(plan.n_records)
               if not oa.rec_unstable[r] and not rc.same_call(mine_r[r], oa.rec_calls[r], oa.rec_gq_allowed[r])]
        assert not bad, (what, "per record, against the oracle's bins", bad[:10])
        st["variants_left_out"] += int(oa.unstable.sum())
        st["records_left_out"] += int(oa.rec_unstable.sum())
        st["gq"] = [x + y for x, y in zip(st["gq"], rc.gq_histogram(mine))]
    # 4. the text, 5. the lines
    for i, ignore_imputed in enumerate((False, True)):
        texts = job.record_text(ignore_imputed=ignore_imputed)
        off, text, first = job.record_text_packed(ignore_imputed)
        assert text == b"".join(t for _, t in texts)
        out += [np.asarray(o).tobytes() for o, _ in texts] + [t for _, t in texts]
        for c, (b, res) in enumerate(zip(chains, results)):
            plan = plans[rc.index_of_chain(case, c)]
            empty = np.diff(np.asarray(texts[c][0]).astype(np.int64)) == 0
            few = np.diff(calls.record_gl_offsets(plan).astype(np.int64)) < 3
            st["empty_text"][i] += int(empty.sum())
            st["empty_text_beyond_few"][i] += int((empty & ~few).sum())
            if not check:
                continue
            what = (rc.case_id(case), "chain", c, "ignore_imputed", ignore_imputed)
            rec_var = np.repeat(np.arange(plan.n_variants), np.diff(plan.rec_off.astype(np.int64)))
            kc, uk = res.coverage[rec_var], res.n_kmers[rec_var]
            want_off, want_text, hosts = expected_text(rcalls[c], calls.record_gl_offsets(plan), rgl[c], kc, (uk == 0).astype(np.uint8) if ignore_imputed else None)
            assert_text(texts[c][0], texts[c][1], want_off, want_text, what)
            gl_off = calls.record_gl_offsets(plan).astype(np.int64)
            rec_of_value = np.repeat(np.arange(plan.n_records), np.diff(gl_off))
            predicted = few | ((rcalls[c]["flags"] & 0xFF) == DEFERRED)
            predicted[rec_of_value[is_deferred(rgl[c])]] = True
            assert np.array_equal(empty, predicted) and np.array_equal(empty, hosts), what
            if has_deferred[c]:
                assert (empty & ~few).any(), what
        lines = job.record_lines()
        assert len(lines) == len(job.index)
        out += [np.asarray(o).tobytes() for o, _ in lines] + [t for _, t in lines]
        for k in range(len(job.index)):
            members = _members(case, n_chains, k)
            line_len = np.diff(np.asarray(lines[k][0]).astype(np.int64))
            st["empty_lines"][i] += int((line_len == 0).sum())
            if not check:
                continue
            want_off, want_bytes, hosts = joined(prefixes[k], [texts[c] for c in members])
            assert np.asarray(lines[k][0]).tolist() == want_off.tolist() and lines[k][1] == want_bytes, (rc.case_id(case), "index contig", k, ignore_imputed)
            any_empty = np.zeros(plans[k].n_records, bool)
            for c in members:
                any_empty |= np.diff(np.asarray(texts[c][0]).astype(np.int64)) == 0
            assert np.array_equal(line_len == 0, any_empty) and np.array_equal(hosts, any_empty), (rc.case_id(case), "index contig", k)
    return out, st


def _combined(job, case, plans, groups):
    """step 6 over one combine plan: -> (keys, deferred keys, deferred calls, records, deferred GL values)"""
    results = job.fetch_all()
    job.combine_plan(groups)
    job.combine()
    bins, ccalls = job.combined(), job.combined_calls()
    crec, cgl = job.combined_record_calls(), job.combined_record_gl()
    n = [0, 0, 0, 0, 0]
    for g, grp in enumerate(groups):
        b, plan = job.batches[grp[0]], plans[rc.index_of_chain(case, grp[0])]
        what = (rc.case_id(case), "group", g, grp)
        want, deferred = combined_yardstick(b.allele_off, b.allele_id, [results[c].kept for c in grp], [results[c].allele_present for c in grp],
                                            [results[c].lik for c in grp], [results[c].lik_exp for c in grp])
        keys, n_def = assert_bins(b.allele_off, b.allele_id, bins[g], want, deferred, what)
        left = assert_calls(ccalls[g], calls_yardstick(want), what)
        assert set(left) <= {v for v, d in enumerate(deferred) if d}, what   # a deferred call only where a key is deferred
        calls_want, gl_want = records_yardstick(plan, want)
        left_r = assert_record_calls(crec[g], calls_want, what)
        assert all(deferred[int(np.searchsorted(plan.rec_off, r, "right")) - 1] for r in left_r), what
        gl_def = assert_record_gl(cgl[g], calls.record_gl_offsets(plan), gl_want, what)
        if len(grp) == 1:   # a group of one chain is that chain: its own record calls and GLs, byte for byte
            assert crec[g].tobytes() == calls.fetch_record_calls(job, grp[0]).tobytes() and cgl[g].tobytes() == calls.fetch_record_gl(job, grp[0]).tobytes(), what
        n = [x + y for x, y in zip(n, (keys, n_def, len(left), len(crec[g]), len(gl_def)))]
    return n


@pytest.mark.parametrize("case", CASES, ids=rc.case_id)
def test_regime_job_through_every_consumer(case, monkeypatch):
    e = rc.env(case)
    plans, prefixes = rc.plans_of(case[0]), rc.prefixes_of(case[0])
    job, index, chains = _new_job(monkeypatch, case)
    try:
        plan_text = job.plan()
        assert e.mode is None or job.sweep_mode()[0] == e.mode, plan_text
        for name in e.want:
            assert name in plan_text, (name, plan_text)
        for name in e.unwanted:
            assert name not in plan_text, (name, plan_text)
        assert job.n_chains == len(chains)
        job.run()
        for k, p in enumerate(plans):
            job.record_plan(k, p)
            job.line_prefix(k, *prefixes[k])
        first, st = _consume(job, case, plans, prefixes, True)
        combined = [_combined(job, case, plans, groups) for groups in rc.combine_plans(case)]
        job.run()
        again, st2 = _consume(job, case, plans, prefixes, False)
        assert len(first) == len(again) and all(x == y for x, y in zip(first, again))   # 8. the same bits twice
        assert all(st[k] == st2[k] for k in ("none", "not_unique", "deferred", "rec_deferred", "gl_deferred", "empty_text", "empty_lines"))
    finally:
        job.close()
    cen = rc.census(case)
    if case[0] == rc.TIE:
        assert st["not_unique"] + st["deferred"] >= 4 * rc.N_TIES
    if case[2] == 0.0:
        assert st["none"] >= 5 * len(chains)
        # deep_target: a deferred variant a chain, its records' calls and values deferred, their text — three values or more — the host's
        assert st["deferred"] >= len(chains) and st["rec_deferred"] >= len(chains) and st["gl_deferred"] >= 3 * len(chains)
        assert min(st["empty_text_beyond_few"]) >= 1
    assert st["records_left_out"] == cen["records_left_out"] <= rc.LEFT_OUT_MAX * cen["records"]
    log_parity(f"regime consumers, {rc.case_id(case)}: census {cen}; device calls NONE {st['none']} NOT_UNIQUE {st['not_unique']} DEFERRED {st['deferred']}; "
               f"deferred record calls {st['rec_deferred']}, deferred GL values {st['gl_deferred']}; length-0 texts {st['empty_text']} "
               f"(of three values or more: {st['empty_text_beyond_few']}), length-0 lines {st['empty_lines']} (ignore_imputed off, on); "
               f"GQ compared within rounding (variants, records): {cen['gq_within_quanta']}; "
               f"left out of the end-to-end comparison: {st['variants_left_out']} variants, {st['records_left_out']} records "
               f"({100.0 * st['records_left_out'] / cen['records']:.3f} %); GQ {dict(zip(rc.GQ_CLASSES, st['gq']))}"
               + "".join(f"; combine plan {groups}: keys {n[0]}, deferred keys {n[1]}, deferred calls {n[2]}, records {n[3]}, deferred GL values {n[4]}"
                         for groups, n in zip(rc.combine_plans(case), combined)))
