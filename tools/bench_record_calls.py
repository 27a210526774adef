#!/usr/bin/env python3
"""Calls per VCF record from the device against the same calls formed on the host, on the cohort_h16m shape of bench.py (the
shape is imported; bench.py is not touched), under a random record plan of 1-3 records per bubble with a tenth of the record
alleles undefined.  One process, after a warm-up, several repeats with their spread:

  (a) the route of a caller who forms them on the host: pg_job_fetch_all of the bins, then per record normalise / fold onto the
      record's alleles / restrict to the defined alleles and renormalise / likeliest genotype / genotype quality in long double
      on 16 host threads (vectorised numpy over the records of one (bubble alleles, record alleles) shape at a time — the same
      operations in the same order as GenotypingResult and Variant::records, whole arrays at once; what depends on the index
      alone is prepared once, outside the timing);
  (b) pg_job_record_calls + pg_job_fetch_record_calls_all.

Prints pg_job_record_calls_ms beside pg_job_calls_ms and asserts that the two routes give the same call for every record.
Sets no threshold on time.

    python tools/bench_record_calls.py --shape small|full [--repeats N]
"""
import argparse
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402  (the shapes)
from pangenie_amd import calls, hmm  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402

LD = np.longdouble
THREADS = 16


def random_plan(rng, batch, max_records=3, undefined=0.1):
    bubbles = []
    aoff, aid = batch.allele_off.astype(np.int64), batch.allele_id
    for v in range(batch.n_variants):
        n_ids = int(aid[aoff[v]:aoff[v + 1]].max()) + 1
        records = []
        for _ in range(int(rng.integers(1, max_records + 1))):
            nA = int(rng.integers(1, min(n_ids, 6) + 1))
            own = rng.integers(0, nA, n_ids)
            own[0] = 0
            records.append((own.tolist(), [True] + [bool(x) for x in (rng.random(nA - 1) >= undefined)]))
        bubbles.append(records)
    return calls.RecordPlan.from_records(bubbles)


def prepare(batch, plan):
    """what the index alone decides, per group of records with the same (bubble alleles A, record alleles nA): the records, their
    bubbles, for every bin the key of the folded map it falls onto, for every key whether both alleles are defined and its GT"""
    aoff = batch.allele_off.astype(np.int64)
    rec_var = np.repeat(np.arange(batch.n_variants), np.diff(plan.rec_off.astype(np.int64)))
    A_of = np.diff(aoff)[rec_var]
    nA_of = plan.n_alleles[:plan.n_records].astype(np.int64)
    groups = []
    for A, nA in sorted(set(zip(A_of.tolist(), nA_of.tolist()))):
        recs = np.flatnonzero((A_of == A) & (nA_of == nA))
        var = rec_var[recs]
        sa, sb = np.triu_indices(A)      # bin order
        ka, kb = np.triu_indices(nA)     # key order of the folded map
        key_of = np.zeros((nA, nA), np.int64)
        key_of[ka, kb] = np.arange(len(ka))
        ids = batch.allele_id[aoff[var][:, None] + np.arange(A)].astype(np.int64)
        own = plan.map[plan.map_off[recs].astype(np.int64)[:, None] + ids].astype(np.int64)            # [n, A] record allele of every slot
        oa, ob = own[:, sa], own[:, sb]
        kidx = key_of[np.minimum(oa, ob), np.maximum(oa, ob)]                                           # [n, bins]
        vcf = plan.vcf_index[plan.vcf_off[recs].astype(np.int64)[:, None] + np.arange(nA)].astype(np.int64)   # [n, nA]
        defined = (vcf[:, ka] != 0xFFFF) & (vcf[:, kb] != 0xFFFF)                                       # [n, keys]
        groups.append(dict(A=A, recs=recs, var=var, sa=sa, sb=sb, kidx=kidx, defined=defined, gt1=vcf[:, ka], gt2=vcf[:, kb],
                           undef=(vcf == 0xFFFF).any(axis=1)))
    return groups


def host_record_calls(batch, plan, groups, res):
    out = np.zeros(plan.n_records, calls.CALL_DTYPE)
    out["allele_1"] = out["allele_2"] = 0xFFFF
    out["flags"] = calls.PG_CALL_NONE
    if plan.n_records == 0:
        return out
    aoff, goff = batch.allele_off.astype(np.int64), batch.geno_off.astype(np.int64)
    lik = np.ldexp(res.lik.astype(LD), res.lik_exp.astype(np.int64))
    for g in groups:
        A, var, sa, sb, kidx = g["A"], g["var"], g["sa"], g["sb"], g["kidx"]
        n, rows = len(var), np.arange(len(var))
        P = (res.allele_present[aoff[var][:, None] + np.arange(A)] != 0) & (res.kept[var][:, None] != 0)
        K = P[:, sa] & P[:, sb]
        L = np.where(K, lik[goff[var][:, None] + np.arange(len(sa))], LD(0))
        s = np.zeros(n, LD)
        for j in range(len(sa)):                      # GenotypingResult::normalize
            s = s + L[:, j]
        Q = np.where((s > 0)[:, None], L / np.where(s > 0, s, LD(1))[:, None], L)
        F = np.zeros(g["defined"].shape, LD)          # Variant::records: the fold, bin after bin
        for j in range(len(sa)):
            F[rows, kidx[:, j]] = F[rows, kidx[:, j]] + np.where(K[:, j], Q[:, j], LD(0))
        empty = ~K.any(axis=1)
        F[empty, 0] = LD(1)                           # genotype_field: an empty map is 0/0 with likelihood 1
        D = g["defined"]
        s2 = np.zeros(n, LD)
        for k in range(F.shape[1]):                   # get_specific_likelihoods
            s2 = s2 + np.where(D[:, k], F[:, k], LD(0))
        renorm = g["undef"] & (s2 > 0)
        F = np.where(renorm[:, None], F / np.where(renorm, s2, LD(1))[:, None], F)
        best = np.zeros(n, LD)
        bk = np.zeros(n, np.int64)
        for k in range(F.shape[1]):                   # get_likeliest_genotype
            up = D[:, k] & (F[:, k] >= best)
            best = np.where(up, F[:, k], best)
            bk = np.where(up, k, bk)
        tie = np.zeros(n, bool)
        for k in range(F.shape[1]):
            tie |= D[:, k] & (bk != k) & (np.abs(F[:, k] - best) < 0.0000000001)
        ok = (best > 0) & ~tie
        pw = LD(1) - best
        with np.errstate(divide="ignore"):
            gq = np.where(pw > 0, (-10 * np.log10(np.where(pw > 0, pw, LD(1)))).astype(np.int64), 10000)
        sel = g["recs"][ok]
        out["allele_1"][sel] = g["gt1"][ok, bk[ok]]
        out["allele_2"][sel] = g["gt2"][ok, bk[ok]]
        out["gq"][sel] = gq[ok]
        out["flags"][sel] = np.where(empty[ok], calls.PG_CALL_OK | calls.PG_CALL_EMPTY, calls.PG_CALL_OK)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["small", "full"], default="small")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    c = dict(bench.COHORTS_MORE["cohort_h16m"])
    if args.shape == "small":
        c.update(samples=64, V=2_000)   # 512 chains: still the kernels of the full shape
    index = [synthetic_panel(c["V"], c["H"], c["K"], seed=777 + i, multiallelic_frac=c["multi"]) for i in range(c["contigs"])]
    pool = []
    for s in range(min(c["samples"], c["distinct"])):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=100_100 + 100 * s + i) for i, ix in enumerate(index)])
        pool.append((list(kcs), list(covs)))
    samples = [pool[s % len(pool)] for s in range(c["samples"])]
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*default_table_args()), hmm.make_params(1.26, False, 1e-5))
    rng = np.random.default_rng(20261019)
    plans = [random_plan(rng, ix) for ix in index]
    prepared = [prepare(ix, p) for ix, p in zip(index, plans)]
    for i, p in enumerate(plans):   # once per index contig
        job.record_plan(i, p)
    nc = len(index)
    n_var = sum(b.n_variants for b in job.batches)
    n_rec = sum(plans[i % nc].n_records for i in range(len(job.batches)))
    for _ in range(2):
        job.run()
    bufs = job.fetch_all()
    job.calls()
    t_a, t_fetch, t_host, t_b, ms_k = [], [], [], [], []
    want = got = None
    chain_plans = [plans[i % nc] for i in range(len(job.batches))]
    chain_groups = [prepared[i % nc] for i in range(len(job.batches))]
    with ThreadPoolExecutor(THREADS) as tp:
        for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
            t0 = time.perf_counter()
            job.fetch_all(into=bufs)
            t1 = time.perf_counter()
            want = list(tp.map(host_record_calls, job.batches, chain_plans, chain_groups, bufs))
            t2 = time.perf_counter()
            got = job.record_calls()
            t3 = time.perf_counter()
            if rep:
                t_fetch.append(t1 - t0); t_host.append(t2 - t1); t_a.append(t2 - t0); t_b.append(t3 - t2); ms_k.append(job.record_calls_ms())
    deferred = called = 0
    for w, g in zip(want, got):
        d = g["flags"] == calls.PG_CALL_DEFERRED
        deferred += int(d.sum())
        called += int(((g["flags"] & 0xFF) == calls.PG_CALL_OK).sum())
        no_call = np.isin(g["flags"], (calls.PG_CALL_NONE, calls.PG_CALL_NOT_UNIQUE))
        assert np.array_equal(no_call[~d], (w["flags"] == calls.PG_CALL_NONE)[~d])
        assert np.array_equal((g["flags"] & calls.PG_CALL_EMPTY)[~d], (w["flags"] & calls.PG_CALL_EMPTY)[~d])
        for f in ("allele_1", "allele_2", "gq"):
            assert np.array_equal(g[f][~d], w[f][~d]), f
    calls_ms = job.calls_ms()
    job.close()
    sp = lambda xs: {"median_ms": round(1e3 * float(np.median(xs)), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}
    print(json.dumps({
        "shape": args.shape, "chains": len(job.batches), "variants": n_var, "records": n_rec, "repeats": args.repeats,
        "called": called, "deferred": deferred, "calls_equal": True,
        "a_fetch_bins_then_host_record_calls": sp(t_a), "a_fetch_all": sp(t_fetch), "a_host_loop_16_threads": sp(t_host),
        "b_device_record_calls_and_fetch": sp(t_b),
        "pg_job_record_calls_ms": {"median": round(float(np.median(ms_k)), 4), "min": round(min(ms_k), 4), "max": round(max(ms_k), 4)},
        "pg_job_calls_ms": round(calls_ms, 4),
    }))


if __name__ == "__main__":
    main()
